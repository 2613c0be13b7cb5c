"""resample / resize / fit without a GPU: the float64 restatement (tests/f64_resample.py) against mathematics - analytic cosines, the
Nyquist rule, the mean, the round trip - the resize rules against brute force, pyp_amd/csrc/ppm_resample_plan.h compiled alone under
AddressSanitizer and UBSan against the model and against what the rule promises, the parsers on the scripts the reference produces
(tests/golden/resample_scripts.json), the mains with a float64 backend, every refusal, and the ABI of ppm_fit_info / ppm_fit_plan."""
import ctypes
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest

import f64_resample as FR
from pyp_amd.abi import FitInfo
from pyp_amd.formats import mrc
from pyp_amd.surface import cli, prompts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRIPTS = {c["case"]: c for c in json.load(open(os.path.join(GOLDEN, "resample_scripts.json")))["scripts"]}
PAIRS = [(64, 32), (32, 64), (48, 36), (36, 48), (96, 70), (56, 42), (50, 40)]


# ------------------------------------------------------------------------------------------ the model against mathematics
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n, m", PAIRS)
def test_cosines_come_back_as_their_analytic_samples(n, m, d):
    if d == 3:
        n, m = n // 2 * 2, m // 2 * 2
    src, want = FR.cosines(n, m, d)
    got = FR.resample(src, m)
    assert got.shape == (m,) * d
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert abs(got.mean() - src.mean()) <= 1e-12


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n, m", PAIRS)
def test_nyquist_pattern(n, m, d):
    """cos(pi x + phi) of the smaller grid comes back as cos(phi) cos(pi t): a wrong Nyquist rule is of the order of the amplitude."""
    src, want = FR.nyquist(n, m, d)
    got = FR.resample(src, m)
    assert np.abs(want).max() > 0.05
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n, m", PAIRS)
def test_mean_round_trip_and_identity(n, m, d):
    shape = (n,) * d
    x = np.random.default_rng(n * 1000 + m).standard_normal(shape) + 0.7
    y = FR.resample(x, m)
    assert abs(y.mean() - x.mean()) <= 1e-12
    if m > n:
        assert np.abs(FR.resample(y, n) - x).max() <= 1e-12
    assert np.abs(FR.resample(x, n) - x).max() <= 1e-13                  # M = N: Y = X
    # a stack: only the last two axes move, every image as if alone
    if d == 2:
        st = np.stack([x, 2 * x + 1])
        ys = FR.resample(st, m, dims=2)
        assert np.abs(ys[0] - y).max() <= 1e-12 and np.abs(ys[1] - (2 * y + 1)).max() <= 1e-11


def test_rule_is_complex_linear_and_hermitian():
    """What lets the kernel carry two real lines as z = a + i b: the rule applied to z gives resample(a) + i resample(b)."""
    rng = np.random.default_rng(2)
    for n, m in PAIRS:
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        z = FR.resample_axis(a + 1j * b, m, 0)
        ya, yb = FR.resample_axis(a, m, 0), FR.resample_axis(b, m, 0)
        assert np.abs(ya.imag).max() <= 1e-13 and np.abs(yb.imag).max() <= 1e-13
        assert np.abs(z.real - ya.real).max() <= 1e-13 and np.abs(z.imag - yb.real).max() <= 1e-13


# ------------------------------------------------------------------------------------------ resize
def _brute_face_mean(a):
    n, d = a.shape[0], a.ndim
    tot, cnt = 0.0, 0
    for idx in np.ndindex(*a.shape):
        if any(i == 0 or i == n - 1 for i in idx):
            tot += float(a[idx]); cnt += 1
    assert cnt == n ** d - (n - 2) ** d
    return tot / cnt


@pytest.mark.parametrize("n, b, d", [(9, 14, 3), (12, 7, 3), (10, 16, 2), (11, 8, 2), (8, 8, 3)])
def test_resize_rules(n, b, d):
    x = np.random.default_rng(n + b).standard_normal((n,) * d) + 2.0
    out, pad = FR.resize_item(x, b)
    assert abs(pad - _brute_face_mean(x)) <= 1e-13
    for idx in np.ndindex(*out.shape):                                   # out[i] = in[i - b // 2 + n // 2], the pad value elsewhere
        src = tuple(i - b // 2 + n // 2 for i in idx)
        want = x[src] if all(0 <= s < n for s in src) else pad
        assert out[idx] == want
    back, _ = FR.resize_item(out, n)                                     # crop and pad are inverse on the kept region
    k = min(n, b)
    lo = n // 2 - k // 2
    sl = (slice(lo, lo + k),) * d
    assert np.array_equal(back[sl], x[sl])
    nrm, npad = FR.resize_item(x, b, normalize=True)
    kept = nrm[(slice(max(0, b // 2 - n // 2), max(0, b // 2 - n // 2) + k),) * d] if b >= n else None
    if kept is not None:
        assert abs(kept.mean()) <= 1e-12 and abs(kept.var() - 1.0) <= 1e-12
        assert abs(npad - _brute_face_mean((x - x.mean()) / x.std())) <= 1e-12
    with pytest.raises(FR.Refused):
        FR.resize_item(np.ones((n,) * d), b, normalize=True)


def test_resize_stack_is_per_image():
    st = np.random.default_rng(4).standard_normal((3, 10, 10))
    out, pads = FR.resize(st, 14)
    for i in range(3):
        o, p = FR.resize_item(st[i], 14)
        assert np.array_equal(out[i], o) and pads[i] == p
    v, pv = FR.resize(st[0], 12)
    assert v.shape == (12, 12) and pv.shape == (1,) and np.array_equal(v, FR.resize_item(st[0], 12)[0])


# ------------------------------------------------------------------------------------------ the plan header
PLAN_MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "ppm_resample_plan.h"
int main(int argc, char **argv) {
    // lines of "n_in pixel_in pixel_out box" on stdin -> "n_c P M ok rel_error pixel_achieved" (hex floats: no rounding on the way)
    int n, b; double a, c;
    while (scanf("%d %lf %lf %d", &n, &a, &c, &b) == 4) {
        const ppm::FitPlan f = ppm::fit_plan(n, a, c, b);
        printf("%d %d %d %d %a %a\n", f.n_c, f.P, f.M, f.ok ? 1 : 0, f.rel_error, f.pixel_achieved);
    }
    for (int k = 0; k <= 600; k++) { int lo, hi; ppm::resample_nearest_ok(k, &lo, &hi); printf("L %d %d %d %d\n", k, ppm::resample_len_ok(k) ? 1 : 0, lo, hi); }
    for (int p = 32; p <= 512; p += 32) for (int q = 32; q <= 512; q += 96) {
        const int L = ppm::resample_lines_per_block(p, q, 48 * 1024);
        printf("B %d %d %d %ld\n", p, q, L, ppm::resample_lines_lds(p, q, L));
    }
    return 0;
}
'''

PLAN_TABLE = ([(100, 1.06, 2.1, 64), (64, 2.0, 1.35, 96), (48, 3.0, 2.0, 32), (512, 1.0, 1.0 / 0.45, 256), (8, 1.0, 1.0, 64), (33, 1.7, 1.7, 33),
               (256, 0.8, 0.8, 256), (256, 1.0, 1.005, 256), (300, 1.0, 3.0, 64), (64, 4.0, 1.0, 512)] +
              [(n, 1.0, 1.0 / s, b) for n in (64, 100, 128, 192, 256, 320, 384, 448) for s in (0.25, 0.45, 0.5, 0.77, 1.0, 1.3, 2.0, 3.0) for b in (64, 256)])


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """ppm_resample_plan.h compiled alone with the host compiler under AddressSanitizer and UBSan; returns (plans, lengths, blocks)."""
    d = tmp_path_factory.mktemp("resample_plan")
    (d / "t.cpp").write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(d / "t"), str(d / "t.cpp")])
    text = "".join("%d %r %r %d\n" % row for row in PLAN_TABLE)
    out = subprocess.run([str(d / "t")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    plans = [ln.split() for ln in out if ln[0] not in "LB"]
    lengths = [[int(v) for v in ln.split()[1:]] for ln in out if ln.startswith("L ")]
    blocks = [[int(v) for v in ln.split()[1:]] for ln in out if ln.startswith("B ")]
    assert len(plans) == len(PLAN_TABLE)
    return plans, lengths, blocks


def test_plan_header_against_the_model_and_the_rule(plan_program):
    plans, lengths, blocks = plan_program
    for (n, a, c, b), got in zip(PLAN_TABLE, plans):
        want = FR.fit_plan(n, a, c, b)
        n_c, P, M, ok = (int(v) for v in got[:4])
        err, px = float.fromhex(got[4]), float.fromhex(got[5])
        assert (n_c, P, M, bool(ok)) == (want["n_c"], want["P"], want["M"], want["ok"]), (n, a, c, b, got, want)
        assert err == want["rel_error"] and px == want["pixel_achieved"]
        # what the rule promises, whatever the model says
        s = a / c
        assert n_c == min(n, 2 * math.ceil(b / (2 * s)) + 2) and P >= n_c and FR.box_ok(P) and FR.box_ok(M)
        errs = {(p, m): abs(m / (p * s) - 1.0) for p in FR.SIZES if p >= n_c for m in FR.SIZES}
        best = min(errs.values())
        assert err == best
        ties = sorted((p * m, p, m) for (p, m), e in errs.items() if e == best)
        assert (P, M) == ties[0][1:]
        assert ok == (best <= 0.01) and abs(px - a * P / M) <= 1e-15 * px
    for k, ok, lo, hi in lengths:
        assert bool(ok) == FR.box_ok(k)
        assert lo == max([s for s in FR.SIZES if s <= k], default=0) and hi == min([s for s in FR.SIZES if s >= k], default=0)
    for p, q, L, lds in blocks:                                         # a block's lines: even, at least two, inside the LDS share asked for
        assert L >= 2 and L % 2 == 0 and L <= 32 and lds <= 48 * 1024 and (L % 4 == 0 or L == 2)
        assert lds == 8 * (p + q) + 8 * (L // 2) * (p + q + 2)


def test_plan_sweep():
    """Inputs of 64 .. 448 voxels with s from 0.25 to 3 stay within 1 % (the worst of this sweep is recorded); a 512 input has no room to pad
    and is refused at s = 0.45."""
    worst = 0.0
    for n in range(64, 449, 32):
        for s in np.arange(0.25, 3.0001, 0.05):
            for b in (64, 128, 256):
                p = FR.fit_plan(n, 1.0, 1.0 / float(s), b)
                assert p["ok"] and p["P"] >= p["n_c"], (n, s, b, p)
                worst = max(worst, p["rel_error"])
    assert worst <= 0.0063 + 1e-4, worst
    p = FR.fit_plan(512, 1.0, 1.0 / 0.45, 512)
    assert p["n_c"] == 512 and p["P"] == 512 and not p["ok"] and p["rel_error"] > 0.01
    with pytest.raises(FR.Refused):
        FR.fit(np.zeros((512, 512, 512), np.float32), 1.0, 1.0 / 0.45, 512)          # refused before the (untouched) pages are read


def test_fit_chain_properties():
    v = FR.make_items((48, 48, 48)).astype(np.float64)
    out, info = FR.fit(v, 3.0, 2.0, 32)
    assert out.shape == (32, 32, 32) and info["P"] >= info["n_c"] and abs(info["pixel_achieved"] / 2.0 - 1) <= 0.01
    # the centre voxel of the input is the centre voxel of the output (sample 0 maps to sample 0 through every stage)
    d = np.zeros((48, 48, 48)); d[24, 24, 24] = 1.0
    o, _ = FR.fit(d, 3.0, 2.0, 32)
    assert np.unravel_index(np.argmax(o), o.shape) == (16, 16, 16)


# ------------------------------------------------------------------------------------------ parsers
def test_parsers_on_the_reference_scripts():
    for case in ("rescale", "resample_and_resize", "resample_and_resize_same_size"):
        prog, log, answers = prompts.split_heredoc(SCRIPTS[case]["commands"][0])
        assert prog == "/opt/pyp/external/cistem2/resample"
        d = prompts.parse_resample(answers)
        assert d["volume"] is True and d["size"] == 36 and d["notes"] == [] and d["input"].endswith("model_48.mrc")
    d = prompts.parse_resample(prompts.split_heredoc(SCRIPTS["resample_and_resize_fraction"]["commands"][0])[2])
    assert d["size"] == 34 and len(d["notes"]) == 3 and "rounded to 34" in d["notes"][0]          # 48 x 0.7 = 33.599999999999994
    for case, norm in (("resize", False), ("resize_normalize", True)):
        prog, _, answers = prompts.split_heredoc(SCRIPTS[case]["commands"][0])
        assert prog == "/opt/pyp/external/cistem2/resize"
        d = prompts.parse_resize(answers)
        assert d["volume"] is True and d["size"] == 32 and d["normalize"] is norm
    d = prompts.parse_resize(prompts.split_heredoc(SCRIPTS["resample_and_resize"]["commands"][1])[2])
    assert d["input"].endswith("model_48.mrc~") and d["output"].endswith("out.mrc") and d["size"] == 32 and d["normalize"] is False
    for case in ("downsample_stack", "bin_stack"):
        prog, _, answers = prompts.split_heredoc(SCRIPTS[case]["commands"][0])
        assert prog == "/opt/pyp/external/frealign_v9.11/bin/resample_mp.exe"
        d = prompts.parse_resample_mp(answers)
        assert d["volume"] is False and d["real_space_binning"] is False and d["size"] == 32


@pytest.mark.parametrize("parse, answers, word", [
    (prompts.parse_resample, ["a.mrc", "b.mrc", "Yes", "36", "36"], "answers"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "No", "36"], "answers"),
    (prompts.parse_resample, ["a.mrc", "b.mrc"], "answers"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "Yes", "36", "40", "36"], "equal"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "No", "36", "abc"], "number"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "perhaps", "36", "36"], "yes or no"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "No", "0", "0"], "positive"),
    (prompts.parse_resample, ["a.mrc", "b.mrc", "No", "nan", "nan"], "finite"),
    (prompts.parse_resample, ["", "b.mrc", "No", "36", "36"], "empty"),
    (prompts.parse_resize, ["a.mrc", "b.mrc", "Yes", "36", "36", "36"], "answers"),
    (prompts.parse_resize, ["a.mrc", "b.mrc", "No", "36", "36", "maybe"], "yes or no"),
    (prompts.parse_resample_mp, ["a.mrc", "b.mrc", "no", "yes", "32", "32"], "real-space"),
    (prompts.parse_resample_mp, ["a.mrc", "b.mrc", "no", "no", "32"], "answers"),
    (prompts.parse_resample_mp, ["a.mrc", "b.mrc", "no", "no", "32", "64"], "equal"),
])
def test_parse_refusals(parse, answers, word):
    with pytest.raises(prompts.PromptError) as e:
        parse(answers)
    assert str(e.value).startswith("ERROR: ") and word in str(e.value)


def test_size_answers_round():
    d = prompts.parse_resample(["a.mrc", "b.mrc", "No", "35.6", "36.4"])
    assert d["size"] == 36 and len(d["notes"]) == 2
    assert prompts.parse_resample(["a.mrc", "b.mrc", "No", "36.0", "36"])["notes"] == []
    assert prompts.resample_nearest_ok(34) == [32, 36] and prompts.resample_nearest_ok(600) == [512] and prompts.resample_nearest_ok(8) == [32]
    assert [n for n in range(0, 600) if prompts.resample_len_ok(n)] == FR.SIZES


# ------------------------------------------------------------------------------------------ the mains with a float64 backend
def f64_backend(kind, seen):
    def run(x, n_out, volume, normalize):
        seen.append((x.shape, n_out, volume, normalize))
        if kind == "resize":
            return FR.resize(x, n_out, normalize=normalize, volume=volume)[0].astype(np.float32)
        return FR.resample(x, n_out, dims=3 if volume else 2).astype(np.float32)
    return run


def _stdin(answers):
    return io.StringIO("\n".join(answers) + "\n")


def test_resize_main_on_the_small_fixtures(tmp_path, capsys):
    rng = np.random.default_rng(8)
    vol = rng.standard_normal((8, 8, 8)).astype(np.float32)
    mrc.write(vol, str(tmp_path / "v8.mrc"), pixel_size=1.7)
    seen = []
    assert cli.resize_main(stdin=_stdin([str(tmp_path / "v8.mrc"), str(tmp_path / "v12.mrc"), "Yes", "12", "12", "12", "N"]), backend=f64_backend("resize", seen)) == 0
    out = capsys.readouterr().out
    assert out.rstrip().endswith("Resize: Normal termination") and "Build-defined" in out
    assert seen == [((8, 8, 8), 12, True, False)]
    got = mrc.read(str(tmp_path / "v12.mrc"))
    assert np.array_equal(got, FR.resize(vol, 12, volume=True)[0].astype(np.float32))
    assert abs(mrc.read_header(str(tmp_path / "v12.mrc"))["pixel_size"] - 1.7) < 1e-6            # the pixel size stays
    stack = mrc.read(os.path.join(GOLDEN, "stack_4x8x8.mrc"))
    src = os.path.join(GOLDEN, "stack_4x8x8.mrc")
    assert cli.resize_main(stdin=_stdin([src, str(tmp_path / "s10.mrc"), "No", "10.0", "10", "Y"]), backend=f64_backend("resize", seen)) == 0
    got = mrc.read(str(tmp_path / "s10.mrc"))
    want = FR.resize(stack, 10, normalize=True)[0].astype(np.float32)
    assert got.shape == (4, 10, 10) and np.array_equal(got, want)
    h = mrc.read_header(str(tmp_path / "s10.mrc"))
    assert abs(h["amean"] - want.mean()) < 1e-5 and abs(h["amin"] - want.min()) < 1e-6 and abs(h["amax"] - want.max()) < 1e-6
    assert sorted(os.listdir(tmp_path)) == ["s10.mrc", "v12.mrc", "v8.mrc"]
    capsys.readouterr()


def test_resample_mains_stream_and_set_the_pixel_size(tmp_path, capsys, monkeypatch):
    st = FR.make_items((5, 32, 32))
    mrc.write(st, str(tmp_path / "s32.mrc"), pixel_size=1.5)
    monkeypatch.setattr(cli, "RESAMPLE_CHUNK_BYTES", 2 * 4 * 32 * 32)                            # two images at a time: 2 + 2 + 1
    seen = []
    a = [str(tmp_path / "s32.mrc"), str(tmp_path / "s48.mrc"), "no", "no", "48", "48"]
    assert cli.resample_mp_main(stdin=_stdin(a), backend=f64_backend("resample", seen)) == 0
    assert capsys.readouterr().out.rstrip().endswith("Resample_mp: Normal termination")
    assert [s[0][0] for s in seen] == [2, 2, 1]
    got = mrc.read(str(tmp_path / "s48.mrc"))
    assert np.array_equal(got, FR.resample(st, 48, dims=2).astype(np.float32))
    assert abs(mrc.read_header(str(tmp_path / "s48.mrc"))["pixel_size"] - 1.0) < 1e-6           # 1.5 x 32 / 48
    vol = FR.make_items((32, 32, 32))
    mrc.write(vol, str(tmp_path / "v32.mrc"), pixel_size=2.0)
    a = [str(tmp_path / "v32.mrc"), str(tmp_path / "v36.mrc"), "Yes", "36.0", "36.0", "36.0"]
    assert cli.resample_main(stdin=_stdin(a), backend=f64_backend("resample", seen)) == 0
    assert capsys.readouterr().out.rstrip().endswith("Resample: Normal termination")
    assert np.array_equal(mrc.read(str(tmp_path / "v36.mrc")), FR.resample(vol, 36).astype(np.float32))
    assert abs(mrc.read_header(str(tmp_path / "v36.mrc"))["pixel_size"] - 2.0 * 32 / 36) < 1e-6
    a = [str(tmp_path / "v32.mrc"), str(tmp_path / "i36.mrc"), "No", "36", "36"]                # `No`: every slice as an image
    assert cli.resample_main(stdin=_stdin(a), backend=f64_backend("resample", seen)) == 0
    assert np.array_equal(mrc.read(str(tmp_path / "i36.mrc")), FR.resample(vol, 36, dims=2).astype(np.float32))
    capsys.readouterr()


def _refused(main, tmp_path, answers, capsys, word, kind="resample"):
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        main(stdin=_stdin(answers), backend=f64_backend(kind, []))
    assert e.value.code != 0
    out = capsys.readouterr().out
    assert "ERROR" in out and word in out, out
    assert sorted(os.listdir(tmp_path)) == before


def test_main_refusals_leave_the_directory_as_it_was(tmp_path, capsys):
    mrc.write(FR.make_items((32, 32, 32)), str(tmp_path / "v32.mrc"), pixel_size=2.0)
    mrc.write(np.zeros((8, 8, 8), np.float32), str(tmp_path / "v8.mrc"))
    mrc.write(np.zeros((2, 34, 34), np.float32), str(tmp_path / "s34.mrc"))
    mrc.write(np.zeros((1, 600, 800), np.float32), str(tmp_path / "mic.mrc"))
    mrc.write(np.zeros((2, 768, 768), np.float32), str(tmp_path / "big.mrc"))
    mrc.write(np.ones((2, 16, 16), np.float32), str(tmp_path / "flat.mrc"))
    v, o = str(tmp_path / "v32.mrc"), str(tmp_path / "out.mrc")
    _refused(cli.resample_main, tmp_path, [v, o, "Yes", "34", "34", "34"], capsys, "32 and 36")            # nearest supported sizes
    _refused(cli.resample_main, tmp_path, [str(tmp_path / "v8.mrc"), o, "Yes", "32", "32", "32"], capsys, "nearest: 32")
    _refused(cli.resample_main, tmp_path, [str(tmp_path / "s34.mrc"), o, "No", "32", "32"], capsys, "32 and 36")
    _refused(cli.resample_main, tmp_path, [v, o, "Yes", "36", "40", "36"], capsys, "equal")
    _refused(cli.resample_main, tmp_path, [v, o, "Yes", "36", "36"], capsys, "answers")
    _refused(cli.resample_main, tmp_path, [str(tmp_path / "absent.mrc"), o, "Yes", "36", "36", "36"], capsys, "does not exist")
    _refused(cli.resample_main, tmp_path, [str(tmp_path / "s34.mrc"), o, "Yes", "36", "36", "36"], capsys, "cubic")
    _refused(cli.resample_mp_main, tmp_path, [v, o, "no", "yes", "36", "36"], capsys, "real-space")
    _refused(cli.resample_mp_main, tmp_path, [str(tmp_path / "mic.mrc"), o, "no", "no", "400", "300"], capsys, "equal")
    _refused(cli.resample_mp_main, tmp_path, [str(tmp_path / "mic.mrc"), o, "no", "no", "300", "300"], capsys, "micrographs")
    _refused(cli.resample_mp_main, tmp_path, [str(tmp_path / "big.mrc"), o, "no", "no", "384", "384"], capsys, "micrographs")
    _refused(cli.resize_main, tmp_path, [v, o, "Yes", "600", "600", "600", "N"], capsys, "8..512", kind="resize")
    _refused(cli.resize_main, tmp_path, [v, o, "Yes", "36", "36", "36"], capsys, "answers", kind="resize")
    _refused(cli.resize_main, tmp_path, [str(tmp_path / "flat.mrc"), o, "No", "20", "20", "Y"], capsys, "standard deviation", kind="resize")


def test_fit_reference_main(tmp_path, capsys):
    vol = FR.make_items((48, 48, 48))
    mrc.write(vol, str(tmp_path / "ref.mrc"), pixel_size=3.0)

    def backend(v, a, c, b):
        out, info = FR.fit(v, a, c, b)
        return out.astype(np.float32), FitInfo(n_in=v.shape[0], box_out=b, **{k: info[k] for k in ("n_c", "P", "M", "scale", "pixel_achieved", "rel_error", "pad_value_1", "pad_value_2")})
    assert cli.fit_reference_main([str(tmp_path / "ref.mrc"), str(tmp_path / "fit.mrc"), "--pixel", "2.0", "--box", "32"], backend=backend) == 0
    out = capsys.readouterr().out
    assert out.rstrip().endswith("FitReference: Normal termination") and "Pixel size achieved" in out
    want, info = FR.fit(vol, 3.0, 2.0, 32)
    assert np.array_equal(mrc.read(str(tmp_path / "fit.mrc")), want.astype(np.float32))
    assert abs(mrc.read_header(str(tmp_path / "fit.mrc"))["pixel_size"] - info["pixel_achieved"]) < 1e-6
    before = sorted(os.listdir(tmp_path))

    def refusing(v, a, c, b):
        FR.fit(v, a, c, b)
    mrc.write(np.zeros((2, 34, 34), np.float32), str(tmp_path / "s34.mrc"))
    before = sorted(os.listdir(tmp_path))
    for argv in ([str(tmp_path / "absent.mrc"), str(tmp_path / "o.mrc"), "--pixel", "2", "--box", "32"],
                 [str(tmp_path / "s34.mrc"), str(tmp_path / "o.mrc"), "--pixel", "2", "--box", "32"],
                 [str(tmp_path / "ref.mrc"), str(tmp_path / "o.mrc"), "--pixel", "0", "--box", "32"],
                 [str(tmp_path / "ref.mrc"), str(tmp_path / "o.mrc"), "--pixel", "2", "--box", "4"],
                 [str(tmp_path / "ref.mrc"), str(tmp_path / "o.mrc"), "--box", "32"]):
        with pytest.raises(SystemExit) as e:
            cli.fit_reference_main(argv, backend=backend)
        assert e.value.code != 0 and "ERROR" in capsys.readouterr().out
        assert sorted(os.listdir(tmp_path)) == before


# ------------------------------------------------------------------------------------------ the ABI
def test_fit_info_matches_the_header(tmp_path):
    fields = [f for f, _ in FitInfo._fields_]
    fmt = " ".join(["%zu"] * (1 + len(fields)))
    args = ", ".join(["sizeof(ppm_fit_info)"] + [f"offsetof(ppm_fit_info, {f})" for f in fields])
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ppm.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n' % (fmt, args)
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert got == [ctypes.sizeof(FitInfo)] + [getattr(FitInfo, f).offset for f in fields]


def test_fit_plan_through_ctypes_equals_the_model():
    """ppm_fit_plan touches no device: it runs wherever the library loads."""
    from pyp_amd import host, lib
    for n, a, c, b in PLAN_TABLE[:12]:
        want = FR.fit_plan(n, a, c, b)
        if want["ok"]:
            info = host.fit_plan(n, a, c, b)
            assert (info.n_in, info.box_out, info.n_c, info.P, info.M) == (n, b, want["n_c"], want["P"], want["M"])
            assert (info.scale, info.pixel_achieved, info.rel_error) == (want["scale"], want["pixel_achieved"], want["rel_error"])
        else:
            with pytest.raises(lib.PpmError, match=r"ERROR: fit: .*best is %d -> %d" % (want["P"], want["M"])):
                host.fit_plan(n, a, c, b)
    for bad in ((4, 1.0, 1.0, 64), (64, 1.0, 1.0, 600), (64, 0.0, 1.0, 64), (64, 1.0, -2.0, 64)):
        with pytest.raises(lib.PpmError, match="ERROR"):
            host.fit_plan(*bad)
