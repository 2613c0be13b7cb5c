"""Post-processing without a GPU: the command line of PYP's Post-processing block (prompts.parse_postprocessing), every refusal, the
conditions of the inputs that the bounds of tests/test_gpu_post.py rest on, and bin/postprocessing.py's main with the float64
restatement (tests/f64_post.py) as its backend.

The command lines are written out from src/pyp_main.py:6638-6737, one per branch, with the blanks that code leaves between the parts.
"""
import functools
import os
import types

import numpy as np
import pytest

import f64_post as P
from pyp_amd.abi import PostCfg
from pyp_amd.formats import mrc
from pyp_amd.surface import cli, prompts

PX = P.PIXEL
H1, H2 = "/p/frealign/maps/t20s_r01_half1.mrc", "/p/frealign/maps/t20s_r01_half2.mrc"
OUT = "t20s_r01_postprocessing"

# (command line after the program's name, what the parser must make of it)
LINES = [
    # the tutorial: external mask, ad-hoc B of -50, randomisation below FSC 0.8
    (f"{H1} {H2} --mask /p/mask.mrc  --angpix 1.08 --out {OUT} --xml --adhoc_bfac -50 --lowpass auto --highpass 0   --randomize_below_fsc 0.80  ",
     dict(mask_mode="external", mask="/p/mask.mrc", angpix=1.08, out=OUT, bfactor="adhoc", adhoc_bfac=-50.0, lowpass="auto", highpass=0.0,
          randomize="fsc", randomize_value=0.8, gaussian=False, flip_x=False, flip_y=False, flip_z=False, xml=True, refine_res_lim=None)),
    # automatic mask by intensity, automatic B, Gaussian filters, randomisation beyond a resolution, two flips, the plot limit
    (f"{H1} {H2}  --angpix 1.08 --out {OUT} --flip_x --flip_z --refine_res_lim 4.0 --xml --auto_bfac 10.0,0.0 --gaussian --lowpass 3.5 --highpass 100.0  "
     "--automask --automask_input 0 --automask_lp 15.0 --automask_threshold 0.02 --randomize_beyond 6.00  ",
     dict(mask_mode="auto", mask=None, automask_lp=15.0, threshold_method="intensity", threshold_value=0.02, bfactor="auto", fit_low=10.0,
          fit_high=0.0, gaussian=True, lowpass=3.5, highpass=100.0, randomize="resolution", randomize_value=6.0, flip_x=True, flip_y=False,
          flip_z=True, refine_res_lim=4.0)),
    # automatic mask by volume, no B-factor, no FSC weighting
    (f"{H1} {H2}  --angpix 2.16 --out {OUT} --flip_y --xml --lowpass auto --highpass 0 --skip_fsc_weighting  "
     "--automask --automask_input 0 --automask_lp 20 --automask_fraction 0.10 --randomize_below_fsc 0.75  ",
     dict(mask_mode="auto", threshold_method="volume", threshold_value=0.10, automask_lp=20.0, bfactor="none", adhoc_bfac=0.0,
          skip_fsc_weighting=True, apply_fsc2=False, flip_y=True, randomize="fsc", randomize_value=0.75)),
    # automatic mask by sigma, FSC squared
    (f"{H1} {H2}  --angpix 1.08 --out {OUT} --xml --adhoc_bfac 25 --lowpass 4 --highpass 0  --apply_fsc2 "
     "--automask --automask_input 0 --automask_lp 15.0 --automask_sigma 1.5 --randomize_below_fsc 0.80  ",
     dict(mask_mode="auto", threshold_method="sigma", threshold_value=1.5, bfactor="adhoc", adhoc_bfac=25.0, apply_fsc2=True,
          skip_fsc_weighting=False, lowpass=4.0)),
    # no mask, no B-factor, no randomisation method
    (f"{H1} {H2}  --angpix 1.35 --out {OUT} --xml --lowpass auto --highpass 0    ",
     dict(mask_mode="none", mask=None, bfactor="none", randomize="fsc", randomize_value=prompts.POSTPROCESSING_RANDOMIZE_FSC, half1=H1, half2=H2)),
]


@pytest.mark.parametrize("k", range(len(LINES)))
def test_parser_on_pyp_command_lines(k):
    line, want = LINES[k]
    d = prompts.parse_postprocessing(line.split())
    for key, v in want.items():
        assert d[key] == v, (key, d[key], v)
    cfg = cli.post_cfg_from_options(d)
    assert cfg.mask_mode == PostCfg.MASK[d["mask_mode"]] and cfg.pixel_size == d["angpix"]
    assert cfg.lowpass_auto == (1 if d["lowpass"] == "auto" else 0) and cfg.bfactor_method == PostCfg.BFACTOR[d["bfactor"]]
    assert (cfg.flip_x, cfg.flip_y, cfg.flip_z) == tuple(int(d[f]) for f in ("flip_x", "flip_y", "flip_z"))


def test_parser_takes_equals_signs():
    d = prompts.parse_postprocessing([H1, H2, "--angpix=1.5", "--out=o", "--adhoc_bfac=-50"])
    assert d["angpix"] == 1.5 and d["adhoc_bfac"] == -50.0 and d["out"] == "o"


BASE = f"{H1} {H2} --angpix 1.08 --out {OUT} "
REFUSED = [
    (BASE + "--mtf /p/mtf.star", "MTF"),
    (BASE + "--automask --automask_input 1 --automask_lp 15 --automask_threshold 0.02", "automask_input"),
    (BASE + "--skip_fsc_weighting --apply_fsc2", "exclude"),
    (BASE + "--sharpen", "unknown option"),
    (BASE + "-x", "positional"),
    (f"{H1} --angpix 1.08 --out o", "positional"),
    (f"{H1} {H2} --out o", "required"),
    (f"{H1} {H2} --angpix 1.08", "required"),
    (BASE + "--angpix 2", "twice"),
    (f"{H1} {H2} --angpix 0 --out o", "positive"),
    (f"{H1} {H2} --angpix abc --out o", "number"),
    (BASE + "--automask --automask_input 0 --automask_lp 15", "needs one of"),
    (BASE + "--automask --automask_lp 15 --automask_threshold 0.02 --automask_sigma 1", "needs one of"),
    (BASE + "--automask --automask_lp 15 --automask_fraction 1.5", "fraction"),
    (BASE + "--automask --automask_lp -1 --automask_sigma 1", "negative"),
    (BASE + "--mask m.mrc --automask --automask_threshold 0.02", "exclude"),
    (BASE + "--automask_threshold 0.02", "need --automask"),
    (BASE + "--auto_bfac 10,0 --adhoc_bfac -50", "exclude"),
    (BASE + "--auto_bfac 10", "LOW,HIGH"),
    (BASE + "--auto_bfac 4,10", "LOW > 0"),
    (BASE + "--randomize_below_fsc 0.8 --randomize_beyond 6", "exclude"),
    (BASE + "--randomize_beyond 0", "positive"),
    (BASE + "--lowpass -3", "lowpass"),
    (BASE + "--lowpass", "needs a value"),
    (BASE + "--xml=1", "takes no value"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_parser_refuses(k):
    line, what = REFUSED[k]
    with pytest.raises(prompts.PromptError, match="ERROR.*" + what):
        prompts.parse_postprocessing(line.split())


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests
@functools.lru_cache(maxsize=None)
def model(n, seed=None, **kw):
    h1, h2 = P.make_halves(n, P.SEEDS[n] if seed is None else seed)
    return P.curves(h1, h2, PX, P.options(mask="external", **kw), mask=P.make_mask(n))


def first_below(curve):
    return int(np.flatnonzero(curve[1:] < P.CUT)[0]) + 1


def test_generator_at_seed_one():
    """The curves the inputs were designed for: at 32 and 48 the unmasked FSC falls below 0.143 at shells 11 and 14, the masked one at
    13 and 17, and no shell is weaker than the average by more than 3.2 in amplitude."""
    for n, u, m in ((32, 11, 13), (48, 14, 17)):
        c = model(n, seed=1)
        assert (first_below(c["U"]), first_below(c["Mk"])) == (u, m)
        assert max(c["rho"]) <= 3.2


@pytest.mark.parametrize("n", sorted(P.SEEDS))
def test_input_conditions(n):
    c = model(n)
    gu, gc = P.gaps(n, c, 0.8)
    print("GAPS", n, "s_r", c["s_r"], "U", gu, "C", gc, "rho", c["rho"], "Rd max", c["Rd"][c["s_r"] + 2:].max(), "imag", c["imag"])
    assert max(c["rho"]) <= 4.0
    assert c["Rd"][c["s_r"] + 2:].max() <= 0.5
    assert gu >= 100.0 and gc >= 100.0
    assert c["imag"] <= 1e-12
    assert int(c["shell_count"].sum()) == int((P.shell_cube(n) >= 0).sum()) and c["shell_count"][0] == 1 and c["shell_count"][1] == 18
    assert 1 < c["s_r"] < n // 2 - 2 and not np.array_equal(c["C"], c["Mk"])
    s, f_res, _ = P.resolution(c["C"], n, PX)
    idx = P.fit_shells(c["C"], n, PX, P.options(bfactor="auto", fit_low=10.0), f_res)
    assert len(idx) >= 3 and idx[-1] == s - 1 and (c["C"][idx] >= P.CUT).all()


@pytest.mark.parametrize("n", [32, 48])
def test_automask_thresholds_have_room(n):
    a = P.automask_case(n)
    assert a["t_gap"] >= 4 and a["b_gap"] >= 4 and 0 < a["info"]["mask_voxels"] < n ** 3
    assert ((a["soft"] > 0) & (a["soft"] < 1)).any() and np.array_equal(a["soft"] == 1.0, a["body"].astype(bool))


def test_nothing_is_corrected_when_nothing_is_randomised():
    n = 32
    c = model(n, randomize="resolution", randomize_value=0.5)
    assert c["s_r"] == n // 2 and np.array_equal(c["C"], c["Mk"])


def test_shells_and_hash():
    sh = P.shell_cube(32)
    assert sh[0, 0, 0] == 0 and sh[0, 0, 16] == 16 and sh[16, 16, 16] == -1 and sh[0, 1, 1] == 1 and sh[1, 1, 1] == 2 and sh[0, 2, 31] == 2
    assert int(P.mix32(np.array([0], np.uint32))[0]) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    assert int(P.mix32(np.array([1], np.uint32))[0]) == x


def test_refusals_of_the_definition():
    h1, h2 = P.make_halves(32)
    v33 = np.zeros((33, 33, 33), np.float32)
    with pytest.raises(P.Refused, match="box"):
        P.curves(v33, v33, PX, P.options())
    with pytest.raises(P.Refused, match="exclude"):
        P.curves(h1, h2, PX, P.options(skip_fsc_weighting=True, apply_fsc2=True))
    with pytest.raises(P.Refused, match="three shells"):
        P.postprocess(h1, h2, PX, P.options(bfactor="auto", fit_low=10.0, fit_high=9.9))


# ------------------------------------------------------------------------------------------ the program with a float64 backend
def f64_backend(h1, h2, cfg, mask):
    inv = lambda table, v: [k for k, x in table.items() if x == v][0]      # noqa: E731
    opt = P.options(mask=inv(PostCfg.MASK, cfg.mask_mode), automask_lp=cfg.automask_lp, threshold_method=inv(PostCfg.THRESHOLD, cfg.threshold_method),
                    threshold_value=cfg.threshold_value, randomize=inv(PostCfg.RANDOMIZE, cfg.randomize_method), randomize_value=cfg.randomize_value,
                    seed=cfg.seed, bfactor=inv(PostCfg.BFACTOR, cfg.bfactor_method), adhoc_bfac=cfg.adhoc_bfac, fit_low=cfg.fit_low, fit_high=cfg.fit_high,
                    lowpass="auto" if cfg.lowpass_auto else cfg.lowpass, highpass=cfg.highpass, gaussian=bool(cfg.gaussian),
                    skip_fsc_weighting=bool(cfg.skip_fsc_weighting), apply_fsc2=bool(cfg.apply_fsc2), flip_x=bool(cfg.flip_x), flip_y=bool(cfg.flip_y),
                    flip_z=bool(cfg.flip_z))
    r = P.postprocess(h1, h2, cfg.pixel_size, opt, mask=mask)
    info = types.SimpleNamespace(s_r=r["s_r"], resolution=r["resolution"], bfactor=r["bfactor"], transforms=0, threshold=r.get("threshold", 0.0),
                                 mask_voxels=int(r.get("body", r["mask"] >= 0.5).sum()))
    return dict(unmasked=r["unmasked"], masked=r["masked"], mask=r["mask"], curves=np.stack([r["U"], r["Mk"], r["Rd"], r["C"]]), info=info, model=r)


def write_inputs(tmp_path, n=32):
    h1, h2 = P.make_halves(n, P.SEEDS[n])
    paths = [str(tmp_path / k) for k in ("x_r01_half1.mrc", "x_r01_half2.mrc", "mask.mrc")]
    for p, v in zip(paths, (h1, h2, P.make_mask(n))):
        mrc.write(v, p, pixel_size=PX)
    return paths, (h1, h2)


def test_program_writes_its_files(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    n = 32
    (p1, p2, pm), (h1, h2) = write_inputs(tmp_path, n)
    kept = {}

    def backend(*a):
        kept.update(f64_backend(*a))
        return kept

    line = f"{p1} {p2} --mask {pm}  --angpix {PX} --out {OUT} --flip_z --refine_res_lim 4.0 --xml --auto_bfac 10.0,0.0 --lowpass auto --highpass 0   --randomize_below_fsc 0.80  "
    assert cli.postprocessing_main(line.split(), backend=backend) == 0
    log = capsys.readouterr().out
    r = kept["model"]
    assert "Postprocessing: Normal termination" in log and "--xml: nothing in PYP reads such a file" in log
    assert ("FINAL RESOLUTION (corrected FSC = 0.143) : %.3f A" % r["resolution"]) in log and ("%.2f A^2" % r["bfactor"]) in log
    assert sorted(os.listdir(tmp_path)) == sorted([OUT + "-masked.mrc", OUT + "-unmasked.mrc", OUT + "_data.fsc", "mask.mrc", "x_r01_half1.mrc", "x_r01_half2.mrc"])
    for k in ("masked", "unmasked"):
        path = OUT + f"-{k}.mrc"
        assert np.array_equal(mrc.read(path), r[k].astype(np.float32)) and abs(mrc.read_header(path)["pixel_size"] - PX) < 1e-6
    assert np.array_equal(mrc.read(OUT + "-unmasked.mrc"), np.flip(P.maps(h1, h2, r["mask"], r["W"], P.options())[0], 0).astype(np.float32))
    # as the caller reads it (pyp_main.py:6811-6813): column 0 in A, the last column crosses 0.143
    text = open(OUT + "_data.fsc").read()
    assert text.startswith("#") and "refine_res_lim: 4" in text
    table = np.loadtxt(OUT + "_data.fsc", comments="#")[:, [0, 2, 3, 4, 5]]
    assert table.shape == (n // 2, 5) and np.allclose(table[:, 0], n * PX / np.arange(1, n // 2 + 1), rtol=1e-6)
    for col, key in enumerate(("U", "Mk", "Rd", "C"), 1):
        assert np.abs(table[:, col] - r[key][1:]).max() < 1e-8
    i = int(np.flatnonzero(np.diff(np.sign(table[:, -1] - 0.143)))[0])
    fa, fb, ya, yb = 1 / table[i, 0], 1 / table[i + 1, 0], table[i, -1], table[i + 1, -1]
    assert abs(fa + (ya - 0.143) / (ya - yb) * (fb - fa) - 1 / r["resolution"]) < 1e-6


def test_program_writes_the_automatic_mask(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    a = P.automask_case(32)
    for p, v in (("a_half1.mrc", a["h1"]), ("a_half2.mrc", a["h2"])):
        mrc.write(v, p, pixel_size=PX)
    line = f"a_half1.mrc a_half2.mrc  --angpix {PX} --out o --xml --adhoc_bfac -50 --lowpass auto --highpass 0   --automask --automask_input 0 --automask_lp {P.AUTOMASK_LP} --automask_threshold {a['t']!r} "
    assert cli.postprocessing_main(line.split(), backend=f64_backend) == 0
    assert "Automatic mask" in capsys.readouterr().out
    assert np.array_equal(mrc.read("o-automask.mrc"), a["soft"].astype(np.float32)) and os.path.exists("o-masked.mrc")


def test_program_refusals_leave_no_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    (p1, p2, pm), _ = write_inputs(tmp_path)
    before = sorted(os.listdir(tmp_path))
    mrc.write(np.zeros((33, 33, 33), np.float32), "b33.mrc", pixel_size=PX)
    mrc.write(np.zeros((32, 32, 40), np.float32), "slab.mrc", pixel_size=PX)
    mrc.write(np.zeros((48, 48, 48), np.float32), "b48.mrc", pixel_size=PX)
    tail = f" --angpix {PX} --out o --xml --lowpass auto --highpass 0"
    for line, what in ((f"{p1} {p2} --mtf m.star" + tail, "MTF"), (f"{p1} {p2} --skip_fsc_weighting --apply_fsc2" + tail, "exclude"),
                       (f"{p1} {p2} --frobnicate" + tail, "unknown option"), (f"{p1} b48.mrc" + tail, "b48.mrc is"),
                       (f"{p1} {p2} --mask b48.mrc" + tail, "b48.mrc is"), ("slab.mrc slab.mrc" + tail, "cubic"), ("b33.mrc b33.mrc" + tail, "box must be"),
                       (f"{p1} missing.mrc" + tail, "does not exist"), (f"{p1} {p2} --auto_bfac 10.0,9.9" + tail, "three shells"),
                       (f"{p1} {p2} --automask --automask_input 1 --automask_lp 15 --automask_sigma 1" + tail, "automask_input")):
        with pytest.raises(SystemExit) as e:
            cli.postprocessing_main(line.split(), backend=f64_backend)
        assert e.value.code not in (0, None)
        out = capsys.readouterr().out
        assert "ERROR:" in out and what in out and "Normal termination" not in out, (line, out)
        assert sorted(os.listdir(tmp_path)) == sorted(before + ["b33.mrc", "b48.mrc", "slab.mrc"])


def test_launcher_is_executable():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "postprocessing.py")
    assert os.access(path, os.X_OK) and "cli.postprocessing_main()" in open(path).read()
