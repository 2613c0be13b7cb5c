"""CTF estimation without a GPU: the float64 model tests/f64_ctf.py against the fixture the reference's own
periodogram_averaging produced (tests/golden/periodogram_cases.npz, gen_golden_ctf.py) and against mathematics - the spectrum's rules,
and the estimator held to the truth on exact and noisy synthetic data by the bound 1 / (2 lambda s_max^2) - and the plan header
ppm_ctf_plan.h, compiled alone, against the model's rules.

Errors measured by the model (printed as CASE lines; CHANGELOG.md records them): exact spectra 33 .. 79 A against bounds of 635 and
1625 A, the noisy 320 x 288 micrograph at tile 64 86 A against 914 A.
"""
import os
import subprocess

import numpy as np
import pytest

import f64_ctf as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "periodogram_cases.npz"))
CASES = [(GOLD["image_%d" % k], int(GOLD["tile_%d" % k]), GOLD["power_%d" % k]) for k in range(3)]


# ------------------------------------------------------------------------------------------ 1: the reference-run fixture
def test_fixture_holds_the_named_cases():
    assert [(c[0].shape, c[1]) for c in CASES] == [((96, 80), 32), ((70, 100), 32), ((64, 64), 64)]
    for image, tile, power in CASES:
        assert power.dtype == np.float64 and power.shape == (tile, tile // 2 + 1)
        assert power[0, 0] == 0.0 and power.max() == 1.0


@pytest.mark.parametrize("k", [0, 1, 2])
def test_model_equals_the_reference_run(k):
    """Limit: float64 rounding of the summed tiles (f64_ctf.bound_fixture), relative to the largest element, which is 1."""
    image, tile, want = CASES[k]
    got = FC.periodogram(image, tile, normalise=True)
    n_tiles = FC.plan(image.shape, tile)["tiles"]
    err = float(np.abs(got - want).max())
    print("CASE", dict(case=k, tiles=n_tiles, err=err, bound=FC.bound_fixture(n_tiles)))
    assert got.shape == want.shape and err <= FC.bound_fixture(n_tiles)


# ------------------------------------------------------------------------------------------ 2: the model against mathematics
def test_tile_walk():
    assert FC.axis_origins(96, 32) == [0, 16, 32, 48, 64, 64]          # the half tile divides the axis: the last tile repeats
    assert FC.axis_origins(70, 32) == [0, 16, 32, 38]                   # pulled back inside
    assert FC.axis_origins(100, 32) == [0, 16, 32, 48, 64, 68]
    assert FC.axis_origins(64, 64) == [0, 0] and FC.axis_origins(63, 64) == []
    for n in range(32, 200):
        for t in (32, 36, 64):
            o = FC.axis_origins(n, t)
            assert all(0 <= x and x + t <= n for x in o) and len(o) == (n // (t // 2) if n >= t else 0)


def test_power_of_a_plane_wave_and_parseval():
    """A cosine of an integer tile frequency has all its power in that bin whatever the tile's origin; the mean over the full plane of
    the power is T^2 times the mean square of the tiles (Parseval), the half plane counted with its Hermitian weights."""
    t, ky, kx = 32, 5, 3
    y, x = np.mgrid[0:80, 0:112]
    img = np.cos(2 * np.pi * (ky * y + kx * x) / t + 0.3)
    p = FC.periodogram(img, t, normalise=False)
    assert abs(p[ky, kx] - (t * t / 2) ** 2) <= 1e-9 * p[ky, kx]
    q = p.copy()
    q[ky, kx] = 0
    assert q.max() <= 1e-18 * p[ky, kx]
    rng = np.random.default_rng(2)
    img = rng.standard_normal((70, 100))
    p = FC.periodogram(img, t, normalise=False)
    w = np.full(t // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    tiles = FC.tile_stack(img, t)
    assert abs((p * w).sum() - t * t * (tiles ** 2).sum() / len(tiles)) <= 1e-12 * (p * w).sum()


def test_movie_groups():
    rng = np.random.default_rng(3)
    mv = rng.standard_normal((5, 40, 48))
    g = FC.group_means(mv, 2)
    assert len(g) == 3 and np.allclose(g[0], (mv[0] + mv[1]) / 2, atol=1e-15) and np.array_equal(g[2], mv[4])
    p = FC.periodogram(mv, 32, normalise=False, group=2)
    parts = [FC.periodogram(im, 32, normalise=False) for im in g]
    assert np.allclose(p, sum(parts) / 3, rtol=1e-13, atol=0)
    assert np.array_equal(FC.periodogram(mv[:1], 32), FC.periodogram(mv[0], 32))


def test_bound_spectrum_is_small_and_scales():
    img = FC.make_image((70, 100))
    b = FC.bound_spectrum(img, 32, normalise=False)
    p = FC.periodogram(img, 32, normalise=False)
    assert b.shape == p.shape and (b > 0).all() and (b[1:] <= 0.05 * p.max()).all()
    b4 = FC.bound_spectrum(4 * img, 32, normalise=False)
    assert np.allclose(b4, 16 * b, rtol=1e-9)                            # a power: quadratic in the image
    assert np.allclose(FC.bound_spectrum(4 * img, 32), FC.bound_spectrum(img, 32), rtol=1e-6)      # normalised: scale-free


# ------------------------------------------------------------------------------------------ 4: the plan header
PLAN_MAIN = r'''
#include <cstdio>
#include "ppm_ctf_plan.h"
int main() {
    // lines of "nx ny nframes group tile" on stdin -> the plan's fields, or "R <why>"
    int nx, ny, nf, g, t;
    while (scanf("%d %d %d %d %d", &nx, &ny, &nf, &g, &t) == 5) {
        const ppm::CtfSpectrumPlan p = ppm::ctf_spectrum_plan(nx, ny, nf, g, t);
        if (!p.ok) { printf("R %s\n", p.why); continue; }
        printf("P %d %d %d %d %ld %ld %ld %ld %ld %ld %d %ld %ld", p.half_w, p.tiles_x, p.tiles_y, p.groups, p.tiles, p.chunks, p.pass_tiles,
               p.half_floats2, p.part_floats, p.out_floats, p.vec, ppm::ctf_rows_lds(t), ppm::ctf_cols_lds(t));
        for (int i = 0; i < p.tiles_x; i++) printf(" %d", ppm::ctf_tile_origin(i, nx, t));
        printf("\n");
    }
    return 0;
}
'''

PLAN_OK = [(80, 96, 1, 1, 32), (100, 70, 1, 1, 32), (64, 64, 1, 1, 64), (288, 320, 1, 1, 64), (48, 40, 5, 2, 32), (48, 40, 2, 2, 36),
           (4096, 4096, 1, 1, 512), (5760, 4092, 40, 4, 512), (126, 126, 1, 1, 126), (1000, 36, 3, 1, 36)]
PLAN_REFUSED = [((80, 96, 1, 1, 34), "tile"), ((80, 96, 1, 1, 30), "tile"), ((80, 96, 1, 1, 1024), "tile"), ((63, 96, 1, 1, 64), "smaller"),
                ((96, 63, 1, 1, 64), "smaller"), ((96, 96, 3, 4, 32), "frames"), ((96, 96, 3, 0, 32), "frames"), ((0, 96, 1, 1, 32), "empty"),
                ((50000, 50000, 1, 1, 64), "2^31")]


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """ppm_ctf_plan.h compiled alone with the host compiler under AddressSanitizer and UBSan."""
    d = tmp_path_factory.mktemp("ctf_plan")
    (d / "t.cpp").write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(d / "t"), str(d / "t.cpp")])
    rows = PLAN_OK + [r for r, _ in PLAN_REFUSED]
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    out = subprocess.run([str(d / "t")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    return out


def test_plan_header_against_the_model_and_the_rule(plan_program):
    for (nx, ny, nf, g, t), line in zip(PLAN_OK, plan_program):
        assert line.startswith("P "), line
        v = [int(s) for s in line.split()[1:]]
        half_w, tx, ty, groups, tiles, chunks, pass_tiles, half2, part, out, vec, lds_r, lds_c = v[:13]
        want = FC.plan((nf, ny, nx), t, g)
        assert (tx, ty, groups, tiles, chunks) == (want["tiles_x"], want["tiles_y"], want["groups"], want["tiles"], want["chunks"])
        assert v[13:] == FC.axis_origins(nx, t)
        per = t * (t // 2 + 1)
        assert half_w == t // 2 + 1 and out == per and part == chunks * per and half2 == pass_tiles * per
        # a trip holds whole chunks, at least one, and stays inside 256 MB unless one chunk alone is larger; the grid's y stays legal
        assert pass_tiles % FC.CHUNK_TILES == 0 and FC.CHUNK_TILES <= pass_tiles <= chunks * FC.CHUNK_TILES and pass_tiles < 65536
        assert half2 * 8 <= 256 << 20 or pass_tiles == FC.CHUNK_TILES
        assert vec == (1 if nx % 4 == 0 and t % 8 == 0 else 0)
        if vec:
            assert all(o % 4 == 0 for o in v[13:])
        assert lds_r <= 64 * 1024 and lds_c <= 64 * 1024
    for (row, word), line in zip(PLAN_REFUSED, plan_program[len(PLAN_OK):]):
        assert line.startswith("R ") and word in line, (row, line)
        if word in ("tile", "smaller", "frames"):                          # the rules the model states too
            with pytest.raises(FC.Refused):
                FC.plan((row[2], row[1], row[0]), row[4], row[3])


# ------------------------------------------------------------------------------------------ 2b: the estimator against the truth
def _est_tuple(e):
    return (e["df1"], e["df2"], e["angle"])


EXACT = {
    "no astigmatism": (FC.CFG_BOXES, 64, (7000.0, 7000.0, 0.0), None, 0.0),
    "astigmatism": (FC.CFG_BOXES, 64, (7400.0, 6800.0, 35.0), None, 0.0),
    "pixel below 1.4 (crop)": (FC.CFG_CROP, 64, (6400.0, 6000.0, -20.0), None, 0.0),
    "window of +- 500": (FC.CFG_BOXES, 64, (7400.0, 6800.0, 35.0), (6600.0, 7600.0), 0.0),
    "radix 7 box": (FC.CFG_BOXES, 126, (5600.0, 5100.0, 70.0), None, 0.0),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_spectrum_is_recovered(name):
    """|df_est(phi) - df_true(phi)| < 1 / (2 lambda s_max^2) over all directions: the defocus change that moves the phase at max_res by
    pi / 2 (f64_ctf.truth_bound); with no astigmatism the angle is undetermined and only this criterion applies."""
    base, box, truth, window, tol = EXACT[name]
    cfg = FC.make_cfg(**dict(base, tol=tol))
    e = FC.estimate(FC.synthetic_power(box, cfg, *truth), cfg, *(window or (None, None)))
    err = FC.df_direction_error(_est_tuple(e), truth)
    print("CASE", dict(case=name, err=err, bound=FC.truth_bound(cfg), score=e["score"], est=_est_tuple(e)))
    assert e["df1"] >= e["df2"] and -90.0 < e["angle"] <= 90.0 and e["score"] >= e["grid_score"]
    assert err < FC.truth_bound(cfg)
    if window:
        assert window[0] - 1e-9 <= FC.candidate(cfg, FC.fit_plan(box, cfg, *window), e["grid_index"], window[0])[0] <= window[1] + 1e-9


def test_a_restraint_that_binds():
    truth = (7500.0, 6700.0, 35.0)
    free = FC.make_cfg(**FC.CFG_BOXES)
    tied = FC.make_cfg(**dict(FC.CFG_BOXES, tol=100.0))
    p = FC.synthetic_power(64, free, *truth)
    a, b = FC.estimate(p, free), FC.estimate(p, tied)
    err = FC.df_direction_error(_est_tuple(b), truth)
    print("CASE", dict(case="restraint", free=a["df1"] - a["df2"], tied=b["df1"] - b["df2"], err=err, bound=FC.truth_bound(tied)))
    assert 0 <= b["df1"] - b["df2"] < a["df1"] - a["df2"]                 # the restraint pulls the astigmatism in
    assert FC.fit_plan(64, tied)["nj"] == 0 and FC.fit_plan(64, free)["nj"] == 2
    assert err < FC.truth_bound(tied)


def test_noisy_micrograph_is_recovered():
    cfg = FC.make_cfg(**FC.CFG_MICROGRAPH)
    img = FC.synthetic_micrograph((320, 288), cfg, *FC.MICROGRAPH_TRUTH)
    e = FC.estimate(FC.periodogram(img, 64), cfg)
    err = FC.df_direction_error(_est_tuple(e), FC.MICROGRAPH_TRUTH)
    print("CASE", dict(case="noisy 320 x 288, tile 64", err=err, bound=FC.truth_bound(cfg), est=_est_tuple(e)))
    assert err < FC.truth_bound(cfg)


def test_score_rules():
    cfg = FC.make_cfg(**FC.CFG_BOXES)
    cond = FC.condition(FC.synthetic_power(48, cfg, 7400.0, 6800.0, 35.0), cfg)
    pl = cond["plan"]
    assert abs(cond["v"].sum()) <= 1e-9 * np.abs(cond["v"]).sum() and cond["n"] == len(cond["v"]) == 486
    assert (pl["B"], pl["a"], pl["bg_w"], pl["nj"], pl["nc"]) == (48, 3.0, 4, 2, 25)
    # the angle has period 180 degrees, and means nothing without astigmatism
    assert abs(FC.score(cond, cfg, 7000.0, 600.0, 35.0) - FC.score(cond, cfg, 7000.0, 600.0, 215.0)) <= 1e-12
    assert FC.score(cond, cfg, 7000.0, 0.0, 35.0) == FC.score(cond, cfg, 7000.0, 0.0, 80.0)
    # the spectrum's scale does not reach the score
    c2 = FC.condition(9.0 * FC.synthetic_power(48, cfg, 7400.0, 6800.0, 35.0), cfg)
    assert abs(FC.score(c2, cfg, 7100.0, 600.0, 35.0) - FC.score(cond, cfg, 7100.0, 600.0, 35.0)) <= 1e-12
    # candidate indexing and the crop
    assert FC.candidate(cfg, pl, 0) == (4000.0, 0.0, 0.0) and FC.candidate(cfg, pl, 25 + 1 + 12 + 3) == (4500.0, 1000.0, 45.0)
    assert FC.fit_box(64, 1.0) == (44, 64 / 44) and FC.fit_box(64, 1.4) == (64, 1.4) and FC.fit_box(256, 0.83)[0] == 150
    assert [FC.reduce_angle(t) for t in (0.0, 90.0, 91.0, -90.0, 270.0, -135.0)] == [0.0, 90.0, -89.0, 90.0, 90.0, 45.0]


FIT_MAIN = r'''
#include <cstdio>
#include "ppm_ctf_plan.h"
int main() {
    int t; double px, r0, r1, st, tol, lo, hi;
    while (scanf("%d %lf %lf %lf %lf %lf %lf %lf", &t, &px, &r0, &r1, &st, &tol, &lo, &hi) == 8) {
        const ppm::CtfFitPlan p = ppm::ctf_fit_plan(t, px, r0, r1, st, tol);
        if (!p.ok) { printf("R %s\n", p.why); continue; }
        printf("P %d %a %d %d %d %d %d %ld %ld\n", p.B, p.a, p.k2lo, p.k2hi, p.bg_w, p.nj, p.nc, p.max_samples, ppm::ctf_window_steps(lo, hi, st));
    }
    return 0;
}
'''
FIT_OK = [(64, 3.0, 40.0, 8.0, 500.0, 0.0, 4000.0, 9000.0), (64, 1.0, 30.0, 5.0, 500.0, 0.0, 3000.0, 8000.0), (126, 3.0, 40.0, 8.0, 500.0, 500.0, 6600.0, 7600.0),
          (256, 0.83, 30.0, 3.5, 250.0, 0.0, 3500.0, 50000.0), (512, 1.08, 15.0, 3.5, 250.0, 200.0, 3500.0, 50000.0), (32, 2.0, 40.0, 4.1, 100.0, 0.0, 7000.0, 7000.0)]
FIT_REFUSED = [(63, 3.0, 40.0, 8.0, 500.0, 0.0, 1.0, 2.0), (64, 0.1, 40.0, 8.0, 500.0, 0.0, 1.0, 2.0), (64, 3.0, 8.0, 40.0, 500.0, 0.0, 1.0, 2.0),
               (64, 3.0, 40.0, 8.0, 0.0, 0.0, 1.0, 2.0), (64, 3.0, 400.0, 390.0, 500.0, 0.0, 1.0, 2.0), (64, 3.0, 40.0, 8.0, 1.0, 0.0, 1.0, 2.0)]


def test_fit_plan_header_against_the_model(tmp_path):
    (tmp_path / "t.cpp").write_text(FIT_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp")])
    rows = FIT_OK + FIT_REFUSED
    text = "".join("%d %r %r %r %r %r %r %r\n" % r for r in rows)
    out = subprocess.run([str(tmp_path / "t")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    for (t, px, r0, r1, st, tol, lo, hi), line in zip(FIT_OK, out):
        assert line.startswith("P "), line
        f = line.split()[1:]
        want = FC.fit_plan(t, FC.make_cfg(px, min_res=r0, max_res=r1, step=st, tol=tol), lo, hi)
        assert (int(f[0]), float.fromhex(f[1])) == (want["B"], want["a"])
        assert [int(x) for x in f[2:7]] == [want["k2lo"], want["k2hi"], want["bg_w"], want["nj"], want["nc"]]
        assert int(f[7]) == (want["B"] // 2 + 1) * want["B"] and int(f[8]) == want["ni"]
    assert all(line.startswith("R ") for line in out[len(FIT_OK):]), out[len(FIT_OK):]


# ------------------------------------------------------------------------------------------ 3: parser and writers of bin/ctffind
import io
import json

from pyp_amd.formats import mrc
from pyp_amd.surface import ctffind_cli as CLI

SCRIPTS = {c["case"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "ctffind_scripts.json")))["scripts"]}


def _parsed(case):
    argv, answers = CLI.split_command(SCRIPTS[case]["commands"][0])
    return CLI.parse_script(answers, CLI.parse_args(argv)), argv, answers


@pytest.mark.parametrize("case", sorted(SCRIPTS))
def test_every_reference_script_parses_to_what_went_in(case):
    rec = SCRIPTS[case]
    p = rec["parameters"]
    d, argv, _ = _parsed(case)
    power = rec["function"] == "ctffind4_power"
    assert d["spectrum"] == power == ("--amplitude-spectrum-input" in argv)
    assert (d["input"], d["output"]) == ("ctffind4.mrc", "power.mrc")
    assert d["pixel"] == p["scope_pixel"] * (p["extract_bin"] if power else p["data_bin"])
    assert (d["kv"], d["cs"], d["wgh"], d["tile"]) == (p["scope_voltage"], p["scope_cs"], p["scope_wgh"], p["ctf_tile"])
    assert (d["min_res"], d["max_res"], d["step"]) == (p["ctf_min_res"], p["ctf_max_res"], p["ctf_fstep"])
    window = (20500.0, 21500.0) if case == "power_meandef" else (p["ctf_min_def"], p["ctf_max_def"])
    assert (d["min_def"], d["max_def"]) == window
    movie = rec["frames"] > 2
    assert d["movie"] == movie and d["average"] == ({"movie": 4, "movie_use_ast": 2}[case] if movie else 1)
    # the restraint: ctffind4_power always sends ctf_dast; the image form sends it with ctf_use_ast and 0 (= none) without; the movie form none
    assert d["tol"] == (p["ctf_dast"] if power or (p["ctf_use_ast"] and not movie) else 0.0)


def _mutate(case, index, *new):
    _, argv, answers = _parsed(case)
    return argv, answers[:index] + list(new) + answers[index + 1:]


REFUSED = {
    "astigmatism known": (lambda: _mutate("image", 12, "yes", "300", "20"), "know what astigmatism"),
    "phase shift": (lambda: _mutate("image", 16, "yes", "0.0", "3.15", "0.5"), "phase-shift search"),
    "phase shift (4.1.5 form)": (lambda: _mutate("power", 16, "yes"), "phase-shift search"),
    "tilt": (lambda: _mutate("image", 17, "yes"), "tilt / thickness"),
    "expert options": (lambda: _mutate("image", 18, "yes"), "expert options"),
    "old-school input": (lambda: (["--old-school-input"], _parsed("image")[2]), "--old-school-input"),
    "ctffind5 sequence": (lambda: _mutate("image", 18, "no", "Yes", "Yes", "1.4", "No", "7"), "ctffind5 prompt sequence"),
    "tile the transforms do not take": (lambda: _mutate("image", 6, "34"), "not a size the transforms take"),
    "image smaller than one tile": (lambda: _mutate("image", 6, "128"), "smaller than one tile"),
    "unknown flag": (lambda: (["--fast"], _parsed("image")[2]), "not supported"),
    "too few answers": (lambda: ([], _parsed("image")[2][:9]), "at least 16"),
}


def _model_backend(d, data):
    cfg = FC.make_cfg(d["pixel"], kv=d["kv"], cs=d["cs"], wgh=d["wgh"], min_res=d["min_res"], max_res=d["max_res"], min_def=d["min_def"],
                      max_def=d["max_def"], step=d["step"], tol=d["tol"])
    p = CLI.half_power_from_amplitude(data) if d["spectrum"] else FC.periodogram(data, d["tile"], normalise=False, group=d["average"])
    e = FC.estimate(p, cfg)
    avrot, res, diag = FC.profile(p, cfg, 0.5 * (e["df1"] + e["df2"]), e["df1"] - e["df2"], e["angle"])
    return [e["df1"], e["df2"], e["angle"], e["score"], e["grid_index"], e["grid_score"], e["n"], res], avrot, diag


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_answers_say_why_and_leave_no_file(name, tmp_path, monkeypatch, capsys):
    make, word = REFUSED[name]
    argv, answers = make()
    monkeypatch.chdir(tmp_path)
    mrc.write(FC.make_image((96, 80)), "ctffind4.mrc", pixel_size=1.08)
    rc = CLI.main(argv, io.StringIO("\n".join(answers) + "\n"), backend=_model_backend)
    out = capsys.readouterr().out
    assert rc != 0 and "ERROR:" in out and word in out, out
    assert sorted(os.listdir(tmp_path)) == ["ctffind4.mrc"]


def test_output_files_read_back_the_way_the_caller_reads_them(tmp_path):
    d = dict(input="in.mrc", output=str(tmp_path / "power.mrc"), pixel=1.08, kv=300.0, cs=2.7, wgh=0.07, tile=64, min_res=15.0, max_res=3.5,
             min_def=3500.0, max_def=50000.0)
    row = [21234.5678, 19876.25, -35.5, 0.123456, 17.0, 0.12, 698.0, 4.25]
    avrot = np.arange(6 * 33, dtype=np.float64).reshape(6, 33) / 7.0
    diag = np.arange(64 * 64, dtype=np.float32).reshape(64, 64)
    CLI.write_outputs(d, row, avrot, diag)
    assert sorted(os.listdir(tmp_path)) == ["power.mrc", "power.txt", "power_avrot.txt"]
    got = np.loadtxt(str(tmp_path / "power.txt"), comments="#", dtype="f")[[1, 2, 3, 5, 6]]
    assert np.allclose(got, [row[0], row[1], row[2], row[3], row[7]], rtol=1e-6)
    back = np.loadtxt(str(tmp_path / "power_avrot.txt"), comments="#")
    assert back.shape == (6, 33) and np.allclose(back, avrot, atol=1e-6)
    assert np.array_equal(mrc.read(str(tmp_path / "power.mrc")).reshape(64, 64), diag)


@pytest.mark.parametrize("case", ["image", "movie", "power"])
def test_front_end_on_the_model(case, tmp_path, monkeypatch, capsys):
    """The whole front end with the float64 model in the GPU's place: the scripts of the fixture at a tile the small image holds."""
    cfg = FC.make_cfg(**FC.CFG_MICROGRAPH)
    img = FC.synthetic_micrograph((320, 288), cfg, *FC.MICROGRAPH_TRUTH)
    monkeypatch.chdir(tmp_path)
    argv, answers = CLI.split_command(SCRIPTS[case]["commands"][0])
    k = 2 if case == "movie" else 0
    answers[2 + k:12 + k] = ["2.0", "300.0", "2.7", "0.07", "64", "40.0", "6.0", "3000.0", "15000.0", "250.0"]
    if case == "power":
        half = np.sqrt(FC.periodogram(img, 64, normalise=False))
        full = np.zeros((64, 64))
        a = np.fft.fftshift(half, axes=0)
        full[:, 32:] = a[:, :-1]
        full[1:, 1:32] = a[:, :-1][::-1, ::-1][:-1, :-1]
        mrc.write(full.astype(np.float32), "ctffind4.mrc")
    else:
        mrc.write(np.stack([img] * 8) if case == "movie" else img, "ctffind4.mrc", pixel_size=2.0)
    assert CLI.main(argv, io.StringIO("\n".join(answers) + "\n"), backend=_model_backend) == 0, capsys.readouterr().out
    got = np.loadtxt("power.txt", comments="#", dtype="f")[[1, 2, 3, 5, 6]]
    assert FC.df_direction_error(tuple(got[:3]), FC.MICROGRAPH_TRUTH) < FC.truth_bound(cfg) and 4.0 <= got[4] <= 40.0
    av = np.loadtxt("power_avrot.txt", comments="#")
    assert av.shape == (6, 33) and av[0, 0] == 0.0 and abs(av[0, -1] - 0.25) < 1e-6 and mrc.read("power.mrc").size == 64 * 64
    assert "Normal termination" in capsys.readouterr().out


def test_an_output_named_like_an_answer(tmp_path, monkeypatch):
    """The program asks "Input is a movie" only of a file with several sections: with the header read, an output file named `no` is an
    output file."""
    _, argv, answers = _parsed("image")
    answers[1] = "no"
    assert CLI.parse_script(answers, False, frames=1)["output"] == "no" and not CLI.parse_script(answers, False, frames=1)["movie"]
    _, _, movie = _parsed("movie")
    d = CLI.parse_script(movie, False, frames=8)
    assert d["movie"] and d["average"] == 4 and d["output"] == "power.mrc"
