"""ppm_create_mask / bin/create_mask on the GPU against the float64 restatement tests/f64_create_mask.py.

Without a low-pass the result is integer logic: the mask and every number of `info` must be equal to the model's.  With one, the
thresholds come from f64_create_mask.pick_threshold (tests/test_create_mask_cpu.py holds the gaps to four bands), and the mask must
still be equal in every voxel; the density range is held to one band (f64_mask.bound_filtered).  The 512^3 input is built from bodies
whose voxels are known by construction.
"""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 - before libpypmatch.so is loaded: the two must end up on one HIP runtime

import f64_create_mask as CM
import f64_mask as FM
import f64_ref as R
from pyp_amd.abi import CreateMaskCfg, MaskCfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = json.load(open(os.path.join(ROOT, "tests", "golden", "create_mask_scripts.json")))["scripts"]
COUNTS = ("above", "components", "largest", "mask_voxels")


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@functools.lru_cache(maxsize=None)
def exact(name, n):
    vol, radius, known = CM.crafted(name, n)
    mask, info = CM.create_mask(vol, 1.0, radius, 0.5)
    mask = mask.astype(np.float32)
    vol.setflags(write=False); mask.setflags(write=False)
    return vol, radius, mask, info, known


@functools.lru_cache(maxsize=None)
def lowpass(n):
    c = CM.lowpass_case(n)
    mask, info = CM.create_mask(c["vol"], c["pixel"], c["radius_A"], c["t"], c["lowpass_A"], c["edge"], c["b"], L=c["L"])
    return c, mask.astype(np.float32), info


def cfg_of(c):
    return CreateMaskCfg.make(c["pixel"], c["radius_A"], c["t"], lowpass_A=c["lowpass_A"], lowpass_edge_px=c["edge"], rebin=c["b"])


# ------------------------------------------------------------------------------------------ 1: integer logic
@pytest.mark.parametrize("name", CM.CASES)
@pytest.mark.parametrize("n", CM.BOXES)
def test_exact_cases(H, n, name):
    vol, radius, want, info, known = exact(name, n)
    got, gi = H.create_mask(vol, CreateMaskCfg.make(1.0, radius, 0.5))
    print("CASE", json.dumps(dict(box=n, case=name, gpu={k: getattr(gi, k) for k in COUNTS}, model={k: info[k] for k in COUNTS})))
    for k in COUNTS:
        assert getattr(gi, k) == info[k], (k, getattr(gi, k), info[k])
    for k, v in known.items():
        if k != "first":
            assert getattr(gi, k) == v, (k, getattr(gi, k), v)
    assert (gi.density_min, gi.density_max) == (info["density_min"], info["density_max"])
    assert got.dtype == np.float32 and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("n", [8, 65])
def test_empty_threshold_is_refused(H, n):
    from pyp_amd import lib
    vol, radius, _, _, _ = exact("equal_bodies", n)
    out = np.full_like(vol, 7.0)
    with pytest.raises(lib.PpmError, match="ERROR.*ranges from 0 to 1"):
        H.create_mask(vol, CreateMaskCfg.make(1.0, radius, 1.5), out=out)
    assert (out == 7.0).all()
    tv, to = torch.from_numpy(vol.copy()).cuda(), torch.full((n, n, n), 7.0, device="cuda")
    with pytest.raises(lib.PpmError, match="ranges from"):
        H.create_mask(tv, CreateMaskCfg.make(1.0, radius, 1.5), out=to)
    assert bool((to == 7.0).all())
    plane = np.zeros_like(vol)
    plane[0] = 1.0                                                          # reaches the threshold, but only outside the sphere
    with pytest.raises(lib.PpmError, match="ranges from 0 to 0"):
        H.create_mask(plane, CreateMaskCfg.make(1.0, n / 4.0, 0.5))


# ------------------------------------------------------------------------------------------ 2: with the low-pass
@pytest.mark.parametrize("n", [32, 48])
def test_lowpass_cases(H, n):
    c, want, info = lowpass(n)
    got, gi = H.create_mask(c["vol"], cfg_of(c))
    band = FM.bound_filtered(n, c["L"])
    print("CASE", json.dumps(dict(box=n, t=c["t"], t_gap=c["t_gap"], b=c["b"], b_gap=c["b_gap"], gpu={k: getattr(gi, k) for k in COUNTS},
                                  model={k: info[k] for k in COUNTS}, differing=int((got != want).sum()),
                                  range_err_over_band=max(abs(gi.density_min - info["density_min"]), abs(gi.density_max - info["density_max"])) / band)))
    for k in COUNTS:
        assert getattr(gi, k) == info[k], (k, getattr(gi, k), info[k])
    assert abs(gi.density_min - info["density_min"]) <= band and abs(gi.density_max - info["density_max"]) <= band
    assert np.array_equal(got, want), int((got != want).sum())
    assert info["components"] >= 3 and info["mask_voxels"] > info["largest"]


# ------------------------------------------------------------------------------------------ 3: 512^3
def test_at_size(H):
    """A serpentine (planes 0..198), a ball of radius 110 around (330, 256, 256), a slab (planes 470..489) and isolated specks between
    them, at least two voxels apart: 3 + specks bodies, the serpentine the largest by construction.  The second call low-passes that
    map to 10 A at 1.35 A / pixel (r_c = 69 Fourier pixels) with t = 0.5: the serpentine averages to a density of a quarter and drops
    out, the ball (5.6 M voxels against the slab's 4.8 M) is the largest body, and its low-passed indicator re-binned at 0.35 covers
    the ball's interior (voxels whose 26 neighbours are all in the ball; the model's margin is in CHANGELOG.md)."""
    N = 512
    b = np.zeros((N, N, N), dtype=bool)
    serp = CM.serpentine(N, nz=200)
    b[:200] = serp
    z, y, x = np.ogrid[220:441, 0:N, 0:N]
    ball = (z - 330) ** 2 + (y - 256) ** 2 + (x - 256) ** 2 <= 110 ** 2
    b[220:441] = ball
    b[470:490, 10:500, 10:500] = True
    specks = 0
    for zs in (205, 212, 455):
        b[zs, 8::16, 8::16] = True
        specks += 32 * 32
    n_serp, n_ball, n_slab = int(serp.sum()), int(ball.sum()), 20 * 490 * 490
    assert n_serp > n_ball > n_slab
    vol = b.astype(np.float32)
    del b
    got, gi = H.create_mask(vol, CreateMaskCfg.make(1.0, 1000.0, 0.5))
    assert (gi.above, gi.components, gi.largest, gi.mask_voxels) == (n_serp + n_ball + n_slab + specks, 3 + specks, n_serp, n_serp)
    assert (gi.density_min, gi.density_max) == (0.0, 1.0)
    assert np.array_equal(got[:200], serp.astype(np.float32)) and not got[200:].any()
    got, gi = H.create_mask(vol, CreateMaskCfg.make(1.35, 1000.0 * 1.35, 0.5, lowpass_A=10.0, lowpass_edge_px=4.0, rebin=0.35), out=got)
    print("CASE", json.dumps(dict(box=N, lowpass={k: getattr(gi, k) for k in COUNTS}, range=[gi.density_min, gi.density_max], ball=n_ball)))
    assert gi.mask_voxels == int(np.count_nonzero(got)) and np.array_equal(np.unique(got), [0.0, 1.0])
    assert 0 < gi.largest <= gi.above and 1 <= gi.components <= gi.above and gi.density_min < 0.5 < gi.density_max
    assert abs(gi.largest - n_ball) < 0.05 * n_ball                      # the ball, give or take its surface
    inner = np.ones((219, N - 2, N - 2), dtype=bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                inner &= ball[dz:dz + 219, dy:dy + N - 2, dx:dx + N - 2]
    assert inner.sum() > 0.9 * n_ball
    assert (got[221:440, 1:N - 1, 1:N - 1][inner] == 1.0).all()


# ------------------------------------------------------------------------------------------ 4: device pointers, reproducibility
def test_device_tensors_and_reproducibility(H):
    c, want, info = lowpass(48)
    cfg = cfg_of(c)
    a, ai = H.create_mask(c["vol"], cfg)
    b, bi = H.create_mask(c["vol"], cfg)
    assert np.array_equal(a, b) and bytes(ai) == bytes(bi)
    tv = torch.from_numpy(c["vol"].copy()).cuda()
    t, ti = H.create_mask(tv, cfg)
    assert t.is_cuda and t.data_ptr() != tv.data_ptr() and np.array_equal(t.cpu().numpy(), a) and bytes(ti) == bytes(ai)
    assert np.array_equal(tv.cpu().numpy(), c["vol"])
    res, _ = H.create_mask(tv, cfg, out=tv)                                  # the mask may take the map's place
    assert res is tv and np.array_equal(tv.cpu().numpy(), a)
    vol, radius, want, _, _ = exact("dense", 130)                            # the busiest labelling of the crafted set, twice
    cfg = CreateMaskCfg.make(1.0, radius, 0.5)
    a, ai = H.create_mask(vol, cfg)
    b, bi = H.create_mask(vol, cfg)
    assert np.array_equal(a, b) and bytes(ai) == bytes(bi) and np.array_equal(a, want)


def test_tracing_changes_no_bit(H, monkeypatch, capfd):
    """PPM_TRACE=1 times the stages with events on the call's stream: the mask and every number of info stay what they are without it,
    and stderr gets one line that names the four stages."""
    c, _, _ = lowpass(32)
    cfg = cfg_of(c)
    a, ai = H.create_mask(c["vol"], cfg)
    capfd.readouterr()
    monkeypatch.setenv("PPM_TRACE", "1")
    b, bi = H.create_mask(c["vol"], cfg)
    monkeypatch.delenv("PPM_TRACE")
    assert np.array_equal(a, b) and bytes(ai) == bytes(bi)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("ppm_create_mask:")]
    assert len(lines) == 1, lines
    for stage in ("low-pass", "threshold", "labelling", "re-bin"):
        assert f" {stage} " in lines[0] and " ms" in lines[0], (stage, lines[0])


def test_empty_threshold_is_refused_under_tracing(H, monkeypatch):
    """The refusal of test_empty_threshold_is_refused leaves the call between two stages: the text is the same with PPM_TRACE=1, and the
    next call of the process gives what it gives without tracing."""
    from pyp_amd import lib
    c, _, _ = lowpass(32)
    want, wi = H.create_mask(c["vol"], cfg_of(c))
    monkeypatch.setenv("PPM_TRACE", "1")
    vol, radius, _, _, _ = exact("equal_bodies", 65)
    out = np.full_like(vol, 7.0)
    with pytest.raises(lib.PpmError, match="ERROR.*ranges from 0 to 1"):
        H.create_mask(vol, CreateMaskCfg.make(1.0, radius, 1.5), out=out)
    assert (out == 7.0).all()
    got, gi = H.create_mask(c["vol"], cfg_of(c))
    assert np.array_equal(got, want) and bytes(gi) == bytes(wi)


def test_refusals(H):
    from pyp_amd import lib
    v4, v33, v32 = (np.ones((k, k, k), np.float32) for k in (4, 33, 32))
    ok = dict(pixel_size=2.0, outer_radius_A=40.0, threshold=0.5)
    for vol, kw in [(v4, {}), (v33, dict(lowpass_A=12.0)), (v32, dict(pixel_size=0.0)), (v32, dict(pixel_size=-1.0)), (v32, dict(outer_radius_A=0.0)),
                    (v32, dict(outer_radius_A=-3.0)), (v32, dict(lowpass_A=-1.0)), (v32, dict(lowpass_A=12.0, lowpass_edge_px=-1.0)),
                    (v32, dict(lowpass_A=12.0, rebin=0.0)), (v32, dict(lowpass_A=12.0, rebin=1.0)), (v32, dict(threshold=float("nan")))]:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(lib.PpmError, match="ERROR"):
            H.create_mask(vol, CreateMaskCfg.make(**args))
    m, i = H.create_mask(v33, CreateMaskCfg.make(**ok))                       # no low-pass: any box, and the re-bin value is not looked at
    assert m.shape == (33, 33, 33) and i.largest == i.above == int(m.sum())
    assert H.create_mask(v32, CreateMaskCfg.make(rebin=7.0, **ok))[1].components == 1
    with pytest.raises(ValueError, match="ERROR"):
        H.create_mask(np.ones((8, 8, 9), np.float32), CreateMaskCfg.make(**ok))


# ------------------------------------------------------------------------------------------ 5: the executables, one after the other
def test_executables_in_sequence(H, tmp_path, monkeypatch):
    """PYP's masking block on a fixture record: bin/create_mask on the second command, bin/apply_mask.exe on the fourth.  The map
    is f64_create_mask.script_case: scaled so that no voxel lies within two bands of the script's own thresholds (0.42 and 0.35;
    tests/test_create_mask_cpu.py::test_script_case_has_room).  The mask must equal the model's, the masked map the float64 chain within
    apply_mask's bound."""
    from pyp_amd.formats import mrc
    monkeypatch.setenv("PPM_LOCK_DIR", str(tmp_path))
    case = [c for c in SCRIPTS if c["case"] == "absolute_threshold"][0]
    n, px = 32, case["pixel_size"]
    p = case["parameters"]
    sc = CM.script_case(n, px, p["particle_rad"], p["mask_lowpass"], p["mask_threshold"], 0.35)
    vol = sc["vol"]
    work = tmp_path / "project"
    os.makedirs(work / "frealign" / "maps")
    os.makedirs(tmp_path / "models")
    model = tmp_path / "models" / "t20s_r01_02.mrc"
    mrc.write(vol, str(model), pixel_size=px)
    script = case["commands"][1].replace("@TMP@", str(tmp_path)).replace("/opt/pyp/external/frealignx/create_mask", os.path.join(ROOT, "bin", "create_mask"))
    script = script.replace(">> /dev/null 2>&1", "")
    r = subprocess.run(script, shell=True, cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CreateMask: Normal termination" in r.stdout, r.stdout + r.stderr
    mask = mrc.read(str(work / "frealign" / "maps" / "mask.mrc"))
    assert abs(mrc.read_header(str(work / "frealign" / "maps" / "mask.mrc"))["pixel_size"] - px) < 1e-6
    want, wi = CM.create_mask(vol, px, p["particle_rad"], p["mask_threshold"], p["mask_lowpass"], sc["edge"], 0.35, L=sc["L"])
    assert np.array_equal(mask, want.astype(np.float32)), int((mask != want).sum())
    assert ("Voxels of the mask             : %d" % wi["mask_voxels"]) in r.stdout and ("Connected components           : %d" % wi["components"]) in r.stdout
    shutil.copy2(model, work / "t20s_r01_02.mrc")                             # what shape_mask_reference does before it calls the program
    script = case["commands"][3].replace("/opt/pyp/external/frealign_v9.11/bin/apply_mask.exe", os.path.join(ROOT, "bin", "apply_mask.exe"))
    r = subprocess.run(script, shell=True, cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ApplyMask: Normal termination" in r.stdout, r.stdout + r.stderr
    masked = mrc.read(str(work / case["output"]))
    hpx = float(mrc.read_header(str(model))["pixel_size"])
    chain = FM.mask_volume(vol, want, hpx, p["mask_edge_width"], p["mask_outside_weight"], 2, 10.0, 10.0)
    assert np.abs(masked - chain).max() <= FM.bound_unfiltered(vol, p["mask_outside_weight"])          # weight 0: the filter drops out
    bad = case["commands"][1].replace("@TMP@", str(tmp_path)).replace("/opt/pyp/external/frealignx/create_mask", os.path.join(ROOT, "bin", "create_mask"))
    bad = bad.replace(">> /dev/null 2>&1", "").replace("\n0.42\n", "\n1000\n").replace("frealign/maps/mask.mrc", "frealign/maps/none.mrc")
    r = subprocess.run(bad, shell=True, cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ERROR" in r.stdout and "ranges from" in r.stdout
    assert sorted(os.listdir(work / "frealign" / "maps")) == ["mask.mrc", "t20s_r01_02_masked.mrc"]


# ------------------------------------------------------------------------------------------ 6: the in-memory iteration
def test_iteration_makes_its_mask(H):
    """pipeline.iteration(auto_mask=cfg) against the explicit two steps: rows bit for bit, maps to 64 eps32 of their maximum (the
    insertion adds with float32 atomics in arrival order: tests/test_gpu_mask.py::test_iteration_masks_its_reference)."""
    from pyp_amd import pipeline, synth
    from pyp_amd.abi import RefineCfg
    n, px = 32, 2.0
    vol, stack, rows = synth.make_dataset(n, 8, pixel=px, snr=0.5)
    imgs = stack.numpy()
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 12.0, global_search=0, res_signed_cc=30.0)
    ccfg = CreateMaskCfg.make(px, 0.45 * n * px, 0.3 * float(np.max(vol)), lowpass_A=12.0, lowpass_edge_px=4.0, rebin=0.35)
    mcfg = MaskCfg.make(px, edge_width=4, outside_weight=0.25, filter=2, filter_radius_A=10.0, filter_edge_px=4.0)
    kw = dict(pixel_size=px, molecular_mass_kda=50.0)
    mask, info = H.create_mask(vol, ccfg)
    assert 0 < info.mask_voxels < n ** 3
    auto = pipeline.iteration(vol, imgs, rows, cfg, auto_mask=ccfg, mask_cfg=mcfg, **kw)
    two = pipeline.iteration(vol, imgs, rows, cfg, mask=mask, mask_cfg=mcfg, **kw)
    plain = pipeline.iteration(vol, imgs, rows, cfg, **kw)
    assert np.array_equal(auto["rows"], two["rows"]) and not np.array_equal(auto["rows"], plain["rows"])
    for k in ("half1", "half2", "filtered", "stats"):
        assert np.abs(auto[k] - two[k]).max() <= 64 * R.EPS32 * np.abs(two[k]).max(), k
    with pytest.raises(ValueError, match="ERROR"):
        pipeline.iteration(vol, imgs, rows, cfg, auto_mask=ccfg, mask=mask, **kw)
