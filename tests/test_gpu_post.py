"""ppm_postprocess / bin/postprocessing.py on the GPU against the float64 restatement tests/f64_post.py.

Integer logic must be equal: shell counts, s_r, the shell at which the corrected curve falls below 0.143, the intensity-threshold
automatic mask, masked == float32(unmasked x mask), flips, repeated calls.  The curves are held shell by shell, every shell 0 .. N/2, to
f64_post.curve_tolerances (about 1e-4 for U and Mk at these boxes); the decisions taken from them lie in gaps of 100 tolerances at
f64_post.SEEDS (asserted in tests/test_post_cpu.py).  The maps are held to MAP_K x f64_mask.floor_model_mask on every voxel: (a) with a
filter that depends on no measured curve, (b) on the default path, the float64 map computed from the curves, B and resolution the GPU
returned, so that a decision is not counted twice.  At 160 the seed is not chosen, so s_r comes from the resolution method there.
Measured floors: CHANGELOG.md.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 - before libpypmatch.so is loaded: the two must end up on one HIP runtime

import f64_mask as FM
import f64_post as P
import f64_ref as R
from pyp_amd.abi import PostCfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = P.PIXEL
BOXES = (32, 48, 70, 160)


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


def cfg_of(opt):
    return PostCfg.make(PX, **opt)


def default_opt(n):
    """The default path: external mask, FSC weighting, automatic B between 10 A and the resolution, low-pass at the resolution."""
    kw = dict(randomize="resolution", randomize_value=7.5) if n not in P.SEEDS else {}
    return P.options(mask="external", bfactor="auto", fit_low=10.0, **kw)


@functools.lru_cache(maxsize=None)
def inputs(n):
    h1, h2 = P.make_halves(n, P.SEEDS.get(n, 1))
    return h1, h2, P.make_mask(n), P.shell_cube(n)


@functools.lru_cache(maxsize=None)
def model(n):
    """The float64 curves of the default path, computed once."""
    h1, h2, m, sh = inputs(n)
    return P.curves(h1, h2, PX, default_opt(n), mask=m, sh=sh)


_gpu = {}


def gpu_default(H, n):
    if n not in _gpu:
        h1, h2, m, _ = inputs(n)
        _gpu[n] = H.postprocess(h1, h2, cfg_of(default_opt(n)), mask=m)
    return _gpu[n]


def map_bound(n, want):
    return R.MAP_K * FM.floor_model_mask(n) * float(np.abs(want).max())


# ------------------------------------------------------------------------------------------ 1: curves and what is decided from them
@pytest.mark.parametrize("n", BOXES)
def test_curves(H, n):
    c, g = model(n), gpu_default(H, n)
    gi = g["info"]
    tol_u, tol_m, tol_r, tol_c = P.curve_tolerances(n, c)
    err = [float(np.abs(g["curves"][k] - c[key]).max()) for k, key in enumerate(("U", "Mk", "Rd", "C"))]
    print("FLOOR", json.dumps(dict(box=n, what="curves", dU=err[0], dMk=err[1], dRd=err[2], dC=err[3], tol_U=tol_u, tol_Mk=tol_m, tol_Rd=tol_r,
                                   tol_C_max=float(tol_c.max()), dC_over_tol=float((np.abs(g["curves"][3] - c["C"]) / tol_c).max()), rho=c["rho"],
                                   s_r=[gi.s_r, c["s_r"]])))
    assert np.array_equal(g["shell_count"], c["shell_count"]) and int(g["shell_count"].sum()) == int((inputs(n)[3] >= 0).sum())
    assert gi.s_r == c["s_r"] and gi.transforms == 5
    assert g["curves"].shape == (4, n // 2 + 1)
    assert (np.abs(g["curves"][0] - c["U"]) <= tol_u).all()
    assert (np.abs(g["curves"][1] - c["Mk"]) <= tol_m).all()
    assert (np.abs(g["curves"][2] - c["Rd"]) <= tol_r).all()
    assert (np.abs(g["curves"][3] - c["C"]) <= tol_c).all()
    assert gi.mask_voxels == int((inputs(n)[2] >= np.float32(0.5)).sum())


@pytest.mark.parametrize("n", sorted(P.SEEDS))
def test_resolution_and_bfactor(H, n):
    c, g = model(n), gpu_default(H, n)
    gi = g["info"]
    opt = default_opt(n)
    s, f_res, res = P.resolution(c["C"], n, PX)
    tol_c = P.curve_tolerances(n, c)[3]
    df = 1.0 / (n * PX)
    res_bound = 3.0 * max(tol_c[s - 1], tol_c[s]) / (c["C"][s - 1] - c["C"][s])
    idx = P.fit_shells(c["C"], n, PX, opt, f_res)
    B = P.bfactor(c["C"], c["sums_m"], n, PX, opt, f_res)
    b_bound = P.bfactor_bound(n, c, idx, PX)
    print("FLOOR", json.dumps(dict(box=n, what="decisions", res_shell=[gi.res_shell, s], resolution=[gi.resolution, res],
                                   d_res_in_shells=abs(1.0 / gi.resolution - f_res) / df, res_bound=res_bound, B=[gi.bfactor, B],
                                   dB=abs(gi.bfactor - B), B_bound=b_bound, fit_shells=[gi.fit_shells, len(idx)])))
    assert gi.res_shell == s and s >= 1
    assert abs(1.0 / gi.resolution - f_res) / df <= res_bound
    assert (c["C"][idx] >= P.CUT).all() and gi.fit_shells == len(idx) >= 3
    assert abs(gi.bfactor - B) <= b_bound


def test_randomise_shell_by_resolution(H):
    n = 32
    h1, h2, m, sh = inputs(n)
    for value, want in ((6.0, 8), (1000.0, 1), (0.5, 16), (48.0 / 6.6, 7)):      # a 48 A box: 6.6 shells round to 7
        opt = P.options(mask="external", randomize="resolution", randomize_value=value, lowpass=0.0)
        g = H.postprocess(h1, h2, cfg_of(opt), mask=m)
        assert g["info"].s_r == want == P.curves(h1, h2, PX, opt, mask=m, sh=sh)["s_r"]
        if want == 16:                                                             # s_r = N/2: nothing is corrected
            assert np.array_equal(g["curves"][3], g["curves"][1])


# ------------------------------------------------------------------------------------------ 2: maps
@pytest.mark.parametrize("n", BOXES)
def test_maps_fixed_filter(H, n):
    """(a) ad-hoc B, no FSC weighting, a numeric low-pass and a high-pass: W depends on no measured curve."""
    h1, h2, m, sh = inputs(n)
    opt = P.options(mask="external", bfactor="adhoc", adhoc_bfac=-50.0, skip_fsc_weighting=True, lowpass=5.0, highpass=40.0,
                    randomize="resolution", randomize_value=7.5)
    g = H.postprocess(h1, h2, cfg_of(opt), mask=m)
    W = np.exp(50.0 * (np.arange(n // 2 + 1) / (n * PX)) ** 2 / 4.0) * P.band_pass(n, PX, opt, None)
    un, ma = P.maps(h1, h2, m.astype(np.float64), W, opt, sh=sh)
    bound = map_bound(n, un)
    e_un, e_ma = float(np.abs(g["unmasked"] - un).max()), float(np.abs(g["masked"] - ma).max())
    print("FLOOR", json.dumps(dict(box=n, what="maps (a)", unmasked=e_un / np.abs(un).max(), masked=e_ma / np.abs(un).max(),
                                   model=FM.floor_model_mask(n), bound=bound / np.abs(un).max())))
    assert g["info"].bfactor == -50.0 and W[0] < 1e-12 and W.max() > 1.0
    assert e_un <= bound and e_ma <= bound
    assert np.array_equal(g["masked"], g["unmasked"] * m)                          # the float32 product of the stored value
    assert np.array_equal(g["mask"], m)


@pytest.mark.parametrize("n", sorted(P.SEEDS))
def test_maps_default_path(H, n):
    """(b) the float64 map from the corrected curve, B and resolution the GPU returned."""
    h1, h2, m, sh = inputs(n)
    g = gpu_default(H, n)
    W, _, _ = P.filter_table(g["curves"][3], None, n, PX, default_opt(n), res=g["info"].resolution, B=g["info"].bfactor)
    un, ma = P.maps(h1, h2, m.astype(np.float64), W, default_opt(n), sh=sh)
    bound = map_bound(n, un)
    e_un, e_ma = float(np.abs(g["unmasked"] - un).max()), float(np.abs(g["masked"] - ma).max())
    print("FLOOR", json.dumps(dict(box=n, what="maps (b)", unmasked=e_un / np.abs(un).max(), masked=e_ma / np.abs(un).max(),
                                   model=FM.floor_model_mask(n), bound=bound / np.abs(un).max(), B=g["info"].bfactor)))
    assert g["info"].bfactor < 0 and W.max() > 1.0                                  # it sharpens
    assert e_un <= bound and e_ma <= bound
    assert np.array_equal(g["masked"], g["unmasked"] * m)


def test_flips(H):
    n = 32
    h1, h2, m, _ = inputs(n)
    base = dict(mask="external", bfactor="adhoc", adhoc_bfac=-50.0)
    plain = H.postprocess(h1, h2, cfg_of(P.options(**base)), mask=m)
    for axes in ((2,), (1,), (0,), (0, 1, 2)):
        kw = {"flip_" + "zyx"[a]: True for a in axes}
        g = H.postprocess(h1, h2, cfg_of(P.options(**base, **kw)), mask=m)
        for k in ("unmasked", "masked"):
            assert np.array_equal(g[k], np.flip(plain[k], axes)), (axes, k)
        assert np.array_equal(g["curves"], plain["curves"]) and np.array_equal(g["mask"], plain["mask"])
    assert not np.array_equal(plain["unmasked"], np.flip(plain["unmasked"], 2))


def test_two_calls_agree(H):
    n = 48
    h1, h2, m, _ = inputs(n)
    cfg = cfg_of(default_opt(n))
    a, b = H.postprocess(h1, h2, cfg, mask=m), H.postprocess(h1, h2, cfg, mask=m)
    t = [torch.from_numpy(np.array(x)).cuda() for x in (h1, h2, m)]
    c, d = H.postprocess(t[0], t[1], cfg, mask=t[2]), H.postprocess(t[0], t[1], cfg, mask=t[2])
    for other in (b, c, d):
        for k in ("unmasked", "masked", "mask"):
            o = other[k].cpu().numpy() if hasattr(other[k], "is_cuda") else other[k]
            assert np.array_equal(a[k], o), k
        assert np.array_equal(a["curves"], other["curves"]) and np.array_equal(a["shell_count"], other["shell_count"])
        assert bytes(a["info"]) == bytes(other["info"])
    assert c["unmasked"].is_cuda and np.array_equal(t[0].cpu().numpy(), h1) and np.array_equal(t[2].cpu().numpy(), m)


def test_no_mask(H):
    n = 32
    h1, h2, _, _ = inputs(n)
    g = H.postprocess(h1, h2, cfg_of(P.options(bfactor="adhoc", adhoc_bfac=-50.0)))
    assert np.array_equal(g["curves"][1], g["curves"][0])
    assert np.array_equal(g["masked"], g["unmasked"]) and (g["mask"] == 1.0).all() and g["info"].mask_voxels == n ** 3


# ------------------------------------------------------------------------------------------ 3: the automatic mask
@functools.lru_cache(maxsize=None)
def auto_case(n):
    return P.automask_case(n)


@pytest.mark.parametrize("n", [32, 48])
def test_automask_intensity(H, n):
    a = auto_case(n)
    g = H.postprocess(a["h1"], a["h2"], cfg_of(a["opt"]))
    gi = g["info"]
    print("CASE", json.dumps(dict(box=n, t=a["t"], t_gap=a["t_gap"], b_gap=a["b_gap"], voxels=[gi.mask_voxels, a["info"]["mask_voxels"]],
                                  differing=int((g["mask"] != a["soft"].astype(np.float32)).sum()))))
    assert gi.threshold == a["t"] and gi.mask_voxels == a["info"]["mask_voxels"] and gi.transforms == 9
    assert np.array_equal(g["mask"] == 1.0, a["body"].astype(bool))
    assert np.array_equal(g["mask"], a["soft"].astype(np.float32))
    assert np.array_equal(g["masked"], g["unmasked"] * g["mask"])
    assert 0 < gi.mask_voxels < int((g["mask"] > 0).sum()) < n ** 3


@pytest.mark.parametrize("n", [32, 48])
def test_automask_sigma_and_volume(H, n):
    a = auto_case(n)
    sph = P.CM.sphere(n, 0.5 * n * PX, PX)
    v = a["L"][sph]
    band = R.MAP_K * FM.floor_model_mask(n) * float(np.abs(a["L"]).max())
    for sigma in (1.5, -0.25):
        opt = P.options(mask="auto", automask_lp=P.AUTOMASK_LP, threshold_method="sigma", threshold_value=sigma)
        g = H.postprocess(a["h1"], a["h2"], cfg_of(opt))
        want = P.automask(a["h1"], a["h2"], PX, opt)[2]
        print("FLOOR", json.dumps(dict(box=n, what="sigma threshold", sigma=sigma, t=[g["info"].threshold, want], bound=(1 + abs(sigma)) * band)))
        assert abs(g["info"].threshold - want) <= (1.0 + abs(sigma)) * band
        assert g["info"].transforms == 11
    for f in (0.05, 0.3):
        opt = P.options(mask="auto", automask_lp=P.AUTOMASK_LP, threshold_method="volume", threshold_value=f)
        g = H.postprocess(a["h1"], a["h2"], cfg_of(opt))
        t = g["info"].threshold
        share, near = float((v >= t).mean()), float((np.abs(v - t) <= band).mean())
        print("FLOOR", json.dumps(dict(box=n, what="volume threshold", f=f, t=t, share=share, near=near)))
        assert abs(share - f) <= near
        assert t == float(np.float32(t))


def _same(a, b):
    for k in ("unmasked", "masked", "mask"):
        x, y = (r[k].cpu().numpy() if hasattr(r[k], "is_cuda") else r[k] for r in (a, b))
        assert np.array_equal(x, y), k
    assert np.array_equal(a["curves"], b["curves"]) and np.array_equal(a["shell_count"], b["shell_count"])
    assert bytes(a["info"]) == bytes(b["info"])


def test_automask_host_and_device_agree(H):
    """Host arrays and CUDA tensors give the same bits with the automatic mask by sigma (test_two_calls_agree holds the two kinds to each
    other with an external mask)."""
    a = auto_case(32)
    cfg = cfg_of(P.options(mask="auto", automask_lp=P.AUTOMASK_LP, threshold_method="sigma", threshold_value=1.5))
    t = [torch.from_numpy(np.array(x)).cuda() for x in (a["h1"], a["h2"])]
    host, dev = H.postprocess(a["h1"], a["h2"], cfg), H.postprocess(t[0], t[1], cfg)
    assert dev["mask"].is_cuda and host["info"].transforms == 11
    _same(host, dev)


def test_tracing_changes_no_bit(H, monkeypatch, capfd):
    """PPM_TRACE=1 times the stages with events on the call's stream; with the automatic mask by volume fraction the two histogram passes
    and the low-pass run inside the first stage.  Maps, curves and info stay what they are without it, and stderr gets one line of
    ppm_postprocess that names the six stages."""
    a = auto_case(32)
    cfg = cfg_of(P.options(mask="auto", automask_lp=P.AUTOMASK_LP, threshold_method="volume", threshold_value=0.3))
    plain = H.postprocess(a["h1"], a["h2"], cfg)
    capfd.readouterr()
    monkeypatch.setenv("PPM_TRACE", "1")
    traced = H.postprocess(a["h1"], a["h2"], cfg)
    monkeypatch.delenv("PPM_TRACE")
    assert plain["info"].transforms == 11
    _same(plain, traced)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("ppm_postprocess:")]
    assert len(lines) == 1, lines
    for stage in ("mask", "unmasked sums", "randomised sums", "masked sums", "filter", "outputs"):
        assert f" {stage} " in lines[0] and " ms" in lines[0], (stage, lines[0])


# ------------------------------------------------------------------------------------------ 4: refusals
def test_refusals(H):
    from pyp_amd import lib
    h1, h2, m, _ = inputs(32)
    v33 = np.ones((33, 33, 33), np.float32)
    with pytest.raises(lib.PpmError, match="ERROR.*box"):
        H.postprocess(v33, v33, cfg_of(P.options()))
    with pytest.raises(lib.PpmError, match="ERROR.*exclude"):
        H.postprocess(h1, h2, cfg_of(P.options(skip_fsc_weighting=True, apply_fsc2=True)))
    with pytest.raises(lib.PpmError, match="ERROR.*three shells"):
        H.postprocess(h1, h2, cfg_of(P.options(mask="external", bfactor="auto", fit_low=10.0, fit_high=9.9)), mask=m)
    with pytest.raises(lib.PpmError, match="ERROR.*mask"):
        H.postprocess(h1, h2, cfg_of(P.options(mask="external")))
    with pytest.raises(lib.PpmError, match="ERROR.*mask"):
        H.postprocess(h1, h2, cfg_of(P.options()), mask=m)
    with pytest.raises(ValueError, match="ERROR"):
        H.postprocess(h1, h2[:, :, :31], cfg_of(P.options()))


# ------------------------------------------------------------------------------------------ 5: the program
def test_program(H, tmp_path, monkeypatch):
    """The command line of pyp_main.py:6735-6736 with the tutorial's settings (external mask, ad-hoc B of -50, FSC randomisation below 0.8)."""
    from pyp_amd.formats import mrc
    monkeypatch.setenv("PPM_LOCK_DIR", str(tmp_path))
    n = 32
    h1, h2, m, _ = inputs(n)
    p1, p2, pm = (str(tmp_path / k) for k in ("t20s_r01_half1.mrc", "t20s_r01_half2.mrc", "mask.mrc"))
    for p, v in ((p1, h1), (p2, h2), (pm, m)):
        mrc.write(v, p, pixel_size=PX)
    exe = os.path.join(ROOT, "bin", "postprocessing.py") + " "
    out = "t20s_r01_postprocessing"
    basic = f"{p1} {p2} --mask {pm}  --angpix {PX} --out {out} --flip_x --refine_res_lim 4.0 --xml "
    comm = exe + basic + "--adhoc_bfac -50 " + "--lowpass auto --highpass 0 " + " " + "" + "--randomize_below_fsc 0.80  "
    r = subprocess.run(comm, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Postprocessing: Normal termination" in r.stdout, r.stdout + r.stderr
    names = sorted(f for f in os.listdir(tmp_path) if f.startswith(out))
    assert names == sorted([out + "-masked.mrc", out + "-unmasked.mrc", out + "_data.fsc"])
    opt = P.options(mask="external", bfactor="adhoc", adhoc_bfac=-50.0, randomize="fsc", randomize_value=0.8, flip_x=True)
    g = H.postprocess(h1, h2, cfg_of(opt), mask=m)
    for k in ("masked", "unmasked"):
        path = str(tmp_path / f"{out}-{k}.mrc")
        assert np.array_equal(mrc.read(path), g[k]), k
        assert abs(mrc.read_header(path)["pixel_size"] - PX) < 1e-6
    table = np.loadtxt(str(tmp_path / (out + "_data.fsc")), comments="#")[:, [0, 2, 3, 4, 5]]          # as pyp_main.py:6811 reads it
    assert table.shape == (n // 2, 5)
    assert np.allclose(table[:, 0], n * PX / np.arange(1, n // 2 + 1), rtol=1e-6)
    assert np.abs(table[:, 1:] - g["curves"][:, 1:].T).max() < 1e-8
    assert "refine_res_lim: 4" in open(tmp_path / (out + "_data.fsc")).read()
    assert ("FINAL RESOLUTION (corrected FSC = 0.143) : %.3f A" % g["info"].resolution) in r.stdout and "--xml" in r.stdout
    bad = comm.replace(out, "refused") + "--skip_fsc_weighting --apply_fsc2"
    r = subprocess.run(bad, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ERROR" in r.stdout and not [f for f in os.listdir(tmp_path) if f.startswith("refused")]


# ------------------------------------------------------------------------------------------ 6: the in-memory iteration
def test_iteration_postprocesses_its_half_maps(H):
    from pyp_amd import pipeline, synth
    from pyp_amd.abi import RefineCfg
    n, px = 32, 2.0
    vol, stack, rows = synth.make_dataset(n, 8, pixel=px, snr=0.5)
    imgs = stack.numpy()
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 12.0, global_search=0, res_signed_cc=30.0)
    kw = dict(pixel_size=px, molecular_mass_kda=50.0)
    pcfg = PostCfg.make(px, bfactor="adhoc", adhoc_bfac=-50.0)
    plain = pipeline.iteration(vol, imgs, rows, cfg, **kw)
    none = pipeline.iteration(vol, imgs, rows, cfg, postprocess=None, **kw)
    post = pipeline.iteration(vol, imgs, rows, cfg, postprocess=pcfg, **kw)
    assert sorted(plain) == sorted(none) == ["filtered", "half1", "half2", "rows", "stats"] and sorted(post) == sorted(list(plain) + ["post"])
    assert np.array_equal(plain["rows"], none["rows"]) and np.array_equal(plain["rows"], post["rows"])
    for k in ("half1", "half2", "filtered", "stats"):                               # the insertion adds with float32 atomics in arrival order
        assert np.abs(plain[k] - none[k]).max() <= 64 * R.EPS32 * np.abs(plain[k]).max(), k
    want = H.postprocess(post["half1"], post["half2"], pcfg)
    for k in ("unmasked", "masked", "mask", "curves", "shell_count"):
        assert np.array_equal(post["post"][k], want[k]), k
    assert bytes(post["post"]["info"]) == bytes(want["info"])
    with pytest.raises(ValueError, match="ERROR"):
        pipeline.iteration(vol, imgs, rows, cfg, postprocess=PostCfg.make(px, mask="external"), **kw)
