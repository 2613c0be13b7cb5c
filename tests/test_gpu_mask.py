"""ppm_mask_volume / bin/apply_mask.exe on the GPU against the float64 restatement tests/f64_mask.py.

The soft mask must come out bit for bit (integer distances, a float64-built table rounded once), the unfiltered blend within
1e-6 max|V| (1 + |g|) (f64_mask.bound_unfiltered), the filtered one within f64_ref.MAP_K x f64_mask.floor_model_mask x max|O|.  Every
voxel of every case is compared; the 512^3 case compares a seeded sample of 2e5 voxels and the six faces.  Measured floors are
printed as `FLOOR {json}` lines (figures: CHANGELOG.md).
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 - before libpypmatch.so is loaded: the two must end up on one HIP runtime

import f64_mask as FM
import f64_ref as R
from pyp_amd.abi import MaskCfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = json.load(open(os.path.join(ROOT, "tests", "golden", "apply_mask_scripts.json")))["scripts"]
PX = 2.0


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


def report(kind, N, **kw):
    print("FLOOR " + json.dumps(dict(kind=kind, box=N, **kw)))


@functools.lru_cache(maxsize=None)
def inputs(N):
    v, m = FM.make_map(N), FM.make_mask(N)
    v.setflags(write=False); m.setflags(write=False)
    return v, m


@functools.lru_cache(maxsize=None)
def soft64(N, w):
    s = FM.soft_mask(inputs(N)[1], w)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def outside64(N, radius, edge):
    o = FM.outside_fft(inputs(N)[0], PX, radius, edge)
    o.setflags(write=False)
    return o


# ------------------------------------------------------------------------------------------ 1-3: no filter
@pytest.mark.parametrize("N, w, g", [(32, 1, 0.0), (32, 1, 0.3), (32, 3, 0.0), (32, 3, 0.3), (32, 8, 0.0), (32, 8, 0.3),
                                     (31, 8, 0.3),        # an odd box: line tails
                                     (32, 31, 0.3)])      # a window wider than half the box
def test_unfiltered(H, N, w, g):
    v, m = inputs(N)
    s64 = soft64(N, w)
    ones = np.ones_like(v)
    s_gpu = H.mask_volume(ones, m, MaskCfg.make(PX, edge_width=w, outside_weight=0.0, filter=0))     # out = s 1 + (1 - s) 0 = s
    assert np.array_equal(s_gpu, s64.astype(np.float32)), int((s_gpu != s64.astype(np.float32)).sum())
    got = H.mask_volume(v, m, MaskCfg.make(PX, edge_width=w, outside_weight=g, filter=0))
    want = FM.mask_volume(v, m, PX, w, g, 0, s=s64)
    err, bound = float(np.abs(got - want).max()), FM.bound_unfiltered(v, g)
    report("mask_unfiltered", N, w=w, g=g, err=err, bound=bound, edge_voxels=int(((s64 > 0) & (s64 < 1)).sum()))
    assert w == 1 or ((s64 > 0) & (s64 < 1)).any()                  # w = 1: the edge is the core itself
    assert err <= bound, (N, w, g, err, bound)


def test_edge_width_zero_keeps_a_soft_mask(H):
    N = 32
    v, _ = inputs(N)
    soft = (np.random.default_rng(5).random((N, N, N), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    s_gpu = H.mask_volume(np.ones_like(v), soft, MaskCfg.make(PX, edge_width=0, outside_weight=0.0))
    assert np.array_equal(s_gpu, np.clip(soft, 0, 1))
    got = H.mask_volume(v, soft, MaskCfg.make(PX, edge_width=0, outside_weight=0.3))
    assert np.abs(got - FM.mask_volume(v, soft, PX, 0, 0.3, 0)).max() <= FM.bound_unfiltered(v, 0.3)


# ------------------------------------------------------------------------------------------ 4: the outside filter
@pytest.mark.parametrize("N, radius, edge", [(32, 10.0, 0.0), (32, 10.0, 10.0), (32, 8.0, 4.0), (48, 10.0, 0.0), (48, 10.0, 10.0)])
def test_filtered(H, N, radius, edge):
    v, m = inputs(N)
    g, w = 0.5, 3
    o64 = outside64(N, radius, edge)
    want = FM.mask_volume(v, m, PX, w, g, 2, radius, edge, outside=o64, s=soft64(N, w))
    got = H.mask_volume(v, m, MaskCfg.make(PX, edge_width=w, outside_weight=g, filter=2, filter_radius_A=radius, filter_edge_px=edge))
    model = FM.floor_model_mask(N)
    err, omax = float(np.abs(got - want).max()), float(np.abs(o64).max())
    report("mask_filtered", N, r_c=N * PX / radius, e=edge, model=model, err_over_model=err / (model * omax), max_outside=omax)
    assert np.abs(o64 - v).max() > 0.1 * omax                       # the filter did something
    assert err <= FM.bound_filtered(N, o64), (N, radius, edge, err / (model * omax))


# ------------------------------------------------------------------------------------------ 5: 512^3
def test_filtered_512(H):
    """r_c = 12 Fourier pixels, e = 4: the float64 side is f64_mask.outside_dft (test_mask_cpu.py holds it to the float64 transforms).
    The core is a ball in planes 300..340 plus single voxels at two opposite corners and on the face x = 0."""
    import ctypes
    from pyp_amd import lib
    N, w, g, radius, edge = 512, 8, 0.5, 512.0 / 12.0, 4.0
    lib.init(0)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    lib.check(lib.load().ppm_device_mem_info(ctypes.byref(free), ctypes.byref(total)))
    if free.value < (6 << 30):
        pytest.skip("needs 6 GB of free device memory")
    rng = np.random.default_rng(512)
    v = rng.random((N, N, N), dtype=np.float32)
    v -= np.float32(0.5)
    ax = np.exp(-(np.arange(N, dtype=np.float32) - 230.0) ** 2 / (2 * 60.0 ** 2)).astype(np.float32)
    v += (np.float32(3.0) * ax)[:, None, None] * ax[None, :, None] * ax[None, None, :]
    m = np.zeros((N, N, N), np.float32)
    z, y, x = np.meshgrid(np.arange(300, 341), np.arange(N), np.arange(N), indexing="ij")
    m[300:341] = (x - 200) ** 2 + (y - 300) ** 2 + (z - 320) ** 2 <= 400
    m[0, 0, 0] = m[N - 1, N - 1, N - 1] = m[N // 2, N // 2, 0] = 1.0
    got = H.mask_volume(v, m, MaskCfg.make(1.0, edge_width=w, outside_weight=g, filter=2, filter_radius_A=radius, filter_edge_px=edge))
    o64 = FM.outside_dft(v, 1.0, radius, edge)
    d2 = FM.sqdist_windowed(FM.core_of(m), w)
    near = np.flatnonzero(d2.ravel() < w * w)
    face = np.zeros((N, N, N), bool)
    face[0] = face[-1] = face[:, 0] = face[:, -1] = face[:, :, 0] = face[:, :, -1] = True
    idx = np.unique(np.concatenate([rng.choice(N ** 3, 200000, replace=False), np.flatnonzero(face.ravel()),
                                    rng.choice(near, 20000, replace=False)]))        # the edge is thin: part of the sample is taken there
    tab = np.concatenate([FM.edge_table(w), [0.0]])
    s = np.maximum(np.clip(m.ravel()[idx], 0, 1).astype(np.float64), tab[d2.ravel()[idx]])
    vv, oo = v.ravel()[idx].astype(np.float64), o64.ravel()[idx]
    want = s * vv + (1.0 - s) * (g * oo)
    model, omax = FM.floor_model_mask(N), float(np.abs(o64).max())
    err = float(np.abs(got.ravel()[idx] - want).max())
    report("mask_filtered", N, r_c=12.0, e=edge, model=model, err_over_model=err / (model * omax), max_outside=omax, compared=int(idx.size),
           edge_voxels_compared=int(((s > 0) & (s < 1)).sum()))
    assert ((s > 0) & (s < 1)).sum() > 1000
    assert err <= R.MAP_K * model * omax, err / (model * omax)


# ------------------------------------------------------------------------------------------ 6: exact cases
def test_exact_cases(H):
    N = 32
    v, m = inputs(N)
    cfg = MaskCfg.make(PX, edge_width=3, outside_weight=0.5, filter=2, filter_radius_A=10.0, filter_edge_px=10.0)
    assert np.array_equal(H.mask_volume(v, np.ones_like(v), cfg), v)                                 # M = 1: out = V
    cfg0 = MaskCfg.make(PX, edge_width=0, outside_weight=0.0, filter=2)
    assert not H.mask_volume(v, np.zeros_like(v), cfg0).any()                                        # M = 0, g = 0: out = 0
    want = H.mask_volume(v, m, cfg)
    buf = v.copy()
    assert H.mask_volume(buf, m, cfg, out=buf) is buf and np.array_equal(buf, want)                  # out aliasing map


def test_refusals(H):
    from pyp_amd import lib
    v4, v33 = np.zeros((4, 4, 4), np.float32), np.zeros((33, 33, 33), np.float32)
    v32 = np.zeros((32, 32, 32), np.float32)
    for vol, kw in [(v4, {}), (v33, dict(filter=2)), (v32, dict(edge_width=65)), (v32, dict(edge_width=-1)), (v32, dict(filter=1)),
                    (v32, dict(filter=2, filter_radius_A=0.0)), (v32, dict(filter=2, filter_edge_px=-1.0)), (v32, dict(pixel_size=0.0))]:
        args = dict(pixel_size=PX)
        args.update(kw)
        with pytest.raises(lib.PpmError, match="ERROR"):
            H.mask_volume(vol, vol, MaskCfg.make(**args))
    assert H.mask_volume(v33, v33, MaskCfg.make(PX, edge_width=3)).shape == (33, 33, 33)             # no filter: any box


# ------------------------------------------------------------------------------------------ 7: device pointers
def test_device_tensors_and_reproducibility(H):
    N = 48
    v, m = inputs(N)
    cfg = MaskCfg.make(PX, edge_width=8, outside_weight=0.5, filter=2, filter_radius_A=10.0, filter_edge_px=10.0)
    a = H.mask_volume(v, m, cfg)
    assert np.array_equal(H.mask_volume(v, m, cfg), a)
    tv, tm = torch.from_numpy(v.copy()).cuda(), torch.from_numpy(m.copy()).cuda()
    t = H.mask_volume(tv, tm, cfg)
    assert t.is_cuda and t.data_ptr() != tv.data_ptr() and np.array_equal(t.cpu().numpy(), a)
    assert np.array_equal(tv.cpu().numpy(), v)
    assert H.mask_volume(tv, tm, cfg, out=tv) is tv and np.array_equal(tv.cpu().numpy(), a)


def test_tracing_changes_no_bit(H, monkeypatch, capfd):
    """PPM_TRACE=1 times the call with events on its stream: the masked map stays what it is without it, and stderr gets one line."""
    v, m = inputs(32)
    cfg = MaskCfg.make(PX, edge_width=3, outside_weight=0.5, filter=2, filter_radius_A=8.0, filter_edge_px=4.0)
    a = H.mask_volume(v, m, cfg)
    capfd.readouterr()
    monkeypatch.setenv("PPM_TRACE", "1")
    b = H.mask_volume(v, m, cfg)
    monkeypatch.delenv("PPM_TRACE")
    assert np.array_equal(a, b)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("ppm_mask_volume:")]
    assert len(lines) == 1, lines
    assert "box 32, edge 3, filter 2" in lines[0] and " on the device " in lines[0] and " ms" in lines[0], lines[0]


# ------------------------------------------------------------------------------------------ 8: the executable
def test_executable_overwrites_its_input(H, tmp_path, monkeypatch):
    from pyp_amd.formats import mrc
    monkeypatch.setenv("PPM_LOCK_DIR", str(tmp_path))
    N, px = 32, 1.35
    v, m = inputs(N)
    mrc.write(v, str(tmp_path / "map.mrc"), pixel_size=px)
    mrc.write(m, str(tmp_path / "mask.mrc"), pixel_size=px)
    case = SCRIPTS[3]                                                    # binary mask, edge 8, weight 0.5, filter 2 / 10 / 10
    exe = os.path.join(ROOT, "bin", "apply_mask.exe")
    script = case["script"].replace(case["script"].split(" << ")[0].strip(), exe).replace(case["previous"], "map.mrc").replace(
        case["parameters"]["refine_maskth"], "mask.mrc")
    r = subprocess.run(script, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ApplyMask: Normal termination" in r.stdout, r.stdout + r.stderr
    want = H.mask_volume(v, m, MaskCfg.make(np.float32(N * px) / N, edge_width=8, outside_weight=0.5, filter=2, filter_radius_A=10.0,
                                            filter_edge_px=10.0))
    assert np.array_equal(mrc.read(str(tmp_path / "map.mrc")), want)
    assert abs(mrc.read_header(str(tmp_path / "map.mrc"))["pixel_size"] - px) < 1e-6
    bad = script.replace("\n2\n10\n10\n", "\n1\n10\n10\n").replace("\nmap.mrc\neot", "\nout.mrc\neot")
    r = subprocess.run(bad, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ERROR" in r.stdout and not os.path.exists(tmp_path / "out.mrc")
    assert sorted(os.listdir(tmp_path)) == sorted(["map.mrc", "mask.mrc"] + [f for f in os.listdir(tmp_path) if f.endswith(".lock")])


# ------------------------------------------------------------------------------------------ 9: the in-memory iteration
def test_iteration_masks_its_reference(H):
    """pipeline.iteration(mask=...) against iteration on a pre-masked map, and mask=None against the call without the argument.  The
    refined rows are equal bit for bit.  The maps cannot be: the insertion adds with float32 atomics in whatever order the blocks
    arrive, so two identical calls already differ in the last bit (measured: 3e-8 of a map with maximum 0.25).  With 8 particles and 8
    trilinear taps each, an accumulator voxel is a sum of at most 64 terms; reordering them moves it by at most 64 eps32 of the sum of
    their magnitudes, and the finalisation is linear in the accumulators up to the Wiener weights: maps and statistics are held to
    64 eps32 of their maximum."""
    from pyp_amd import pipeline, synth
    from pyp_amd.abi import RefineCfg
    n, px = 32, 2.0
    vol, stack, rows = synth.make_dataset(n, 8, pixel=px, snr=0.5)
    imgs = stack.numpy()
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 12.0, global_search=0, res_signed_cc=30.0)
    m = FM.make_mask(n)
    mcfg = MaskCfg.make(px, edge_width=4, outside_weight=0.25, filter=2, filter_radius_A=10.0, filter_edge_px=4.0)
    kw = dict(pixel_size=px, molecular_mass_kda=50.0)
    plain = pipeline.iteration(vol, imgs, rows, cfg, **kw)
    again = pipeline.iteration(vol, imgs, rows, cfg, mask=None, **kw)
    masked = pipeline.iteration(vol, imgs, rows, cfg, mask=m, mask_cfg=mcfg, **kw)
    pre = pipeline.iteration(H.mask_volume(vol, m, mcfg), imgs, rows, cfg, **kw)
    for a, b in ((plain, again), (masked, pre)):
        assert np.array_equal(a["rows"], b["rows"])
        for k in ("half1", "half2", "filtered", "stats"):
            assert np.abs(a[k] - b[k]).max() <= 64 * R.EPS32 * np.abs(b[k]).max(), k
    assert not np.array_equal(masked["rows"], plain["rows"])
    with pytest.raises(ValueError, match="ERROR"):
        pipeline.iteration(vol, imgs, rows, cfg, mask_cfg=mcfg, **kw)
