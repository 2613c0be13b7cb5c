"""Every supported box (even, 32..512, prime factors 2, 3, 5, 7 only: 64 sizes) through the insertion, finalisation and
search paths.  Much of the kernels' work is planned per box at run time (k_prep's row-pair count L and column chunks, the
FFT factor plans, ragged 16^3 insertion bricks, per-shell LDS arrays of the finalisation), so each box is its own case.

Leg A compares insertion and ppm_finalize with the float64 restatement tests/f64_ref.py shell by shell; leg B compares
scores, matching projections and (above 256) refinement with the CPU oracle; leg C checks that unsupported boxes are refused.

Error model of leg A (what limits the agreement with float64): the kernels hold slice positions, trilinear weights and the
image FFT in float32 (relative round-off ~ eps32 x (log2 N + |k|), |k| <= N/2 pixels of position) and evaluate the CTF phase chi
in float32 (absolute error ~ eps32 |chi| plus ~1e-6 of the hardware sine); chi grows as |s|^4 Cs lambda^3, so it is largest
at the biggest box (px = 256 / N gives the finest pixel there).  `floor_model` states this; the bounds are a fixed multiple of
it, set from the floors measured on the MI355X (CHANGELOG.md) and no more than 10x them."""
import concurrent.futures as cf
import json
import math

import numpy as np
import pytest

import f64_ref as R
from pyp_amd import synth
from pyp_amd.abi import FinalCfg, ReconCfg, RefineCfg

pytestmark = pytest.mark.gpu

BOXES = R.supported_boxes()
ANG_TOL_DEG, SHIFT_TOL_PX = 0.1, 0.5                 # BASELINE.json north_star
MAPS_ABOVE_256 = (270, 324, 512)                      # maps of leg A above 256 (time budget: a float64 map costs ~N^3 log N)
SEARCH_ABOVE_256 = R.SEARCH_ABOVE_256                 # leg B above 256: the distinct k_prep plans (see f64_ref.prep_plan)
SHELL_K, VOXEL_K, FSC_K, MAP_K = R.SHELL_K, R.VOXEL_K, R.FSC_K, R.MAP_K
floor_model, leg_a_rows = R.floor_model, R.leg_a_rows
prep_plan, ragged_band = R.prep_plan, R.ragged_band



@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def report(leg, N, **kw):
    print("FLOOR " + json.dumps(dict(leg=leg, box=N, **kw)))


@pytest.mark.parametrize("N", BOXES)
def test_leg_a_insert_and_finalize_vs_float64(H, N):
    px, imgs, rows, rc = leg_a_rows(N)
    model = floor_model(N, rows)
    ga = H.Accumulator(N, px, "C1")
    ga.insert(rc, imgs, rows)
    want, counts = R.insert(N, px, R.symmetry_ops("C1"), imgs, rows, rc)
    assert ga.counts() == counts == [3, 2]
    got = ga.download()
    rep = R.compare_by_shell(got, want, N)
    stray = R.stray_values(got, want)
    fc = FinalCfg(molecular_mass_kda=300.0, inner_radius=0.0, outer_radius=0.45 * N * px, mask_falloff=0.0)
    maps = N <= 256 or N in MAPS_ABOVE_256
    del got
    w = R.finalize(want, N, px, fc, maps=maps)
    del want
    g = ga.finalize(fc)
    ga.close()
    ws, gs = w[3], g[3]
    fsc_err = float(np.abs(ws[:, 3:5] - gs[:, 3:5]).max())
    tol_rec, tol_part = R.ssnr_tolerance(ws, FSC_K * model, SHELL_K * model)
    ssnr_err = float(max((np.abs(ws[:, 6] - gs[:, 6]) / tol_rec).max(), (np.abs(ws[:, 5] - gs[:, 5]) / tol_part).max()))
    map_err = [R.rel_l2(b, a) for a, b in zip(w[:3], g[:3])] if maps else []
    report("A", N, model=model, shell=rep.max_shell_rel, voxel=rep.max_voxel_rel, where=str(rep), fsc=fsc_err, ssnr=ssnr_err,
           maps=map_err, stray=stray)
    assert stray == 0, (N, stray)
    assert rep.max_shell_rel < SHELL_K * model, f"box {N}: {rep}"
    assert rep.max_voxel_rel < VOXEL_K * model, f"box {N}: {rep}"
    assert np.array_equal(ws[:, :3], gs[:, :3]), N                   # shell, resolution, radius: the same double arithmetic
    assert fsc_err < FSC_K * model, (N, fsc_err)                 # FSC, part-FSC
    assert ssnr_err < 1.0, (N, ssnr_err)                          # part-SSNR, rec-SSNR: per shell, R.ssnr_tolerance
    for e in map_err:
        assert e < MAP_K * model, (N, map_err)


def test_background_ring_on_the_mask_radius_box_60(H):
    """Regression: at box 60, 0.4 N px / px is 24 - 1 ulp in double but exactly 24 in float, and 24^2 is the r^2 of the pixels
    (0, +-24), (+-24, 0): the background statistics must follow the double test r^2 > Rm^2 (ppm_oracle.c preprocess_row), which
    counts them.  With the float test the normalisation moved by 7e-4 and the accumulators by 90 x the float32 floor."""
    N = 60
    px, imgs, rows, rc = leg_a_rows(N)
    assert float(np.float32(rc.mask_radius)) / float(np.float32(px)) < 24.0
    assert np.float32(np.float32(rc.mask_radius) / np.float32(px)) == np.float32(24.0)
    ga = H.Accumulator(N, px, "C1")
    ga.insert(rc, imgs, rows)
    want, _ = R.insert(N, px, R.symmetry_ops("C1"), imgs, rows, rc)
    rep = R.compare_by_shell(ga.download(), want, N)
    ga.close()
    model = floor_model(N, rows)
    assert rep.max_shell_rel < SHELL_K * model, str(rep)


@pytest.mark.parametrize("N", [80, 96])
def test_finalize_is_reproducible(H, N):
    """Regression: ppm_finalize zeroed its shell-sum buffer with a hipMemset on the legacy null stream, which the handle's
    non-blocking stream does not wait for; once (box 80) the sums started from a freshly allocated, not yet zeroed buffer and
    the FSC came out 0.11 off.  Finalising the same accumulator repeatedly, with other allocations in between, gives the same
    table and maps to double / float round-off of the shell sums' atomic order."""
    px, imgs, rows, rc = leg_a_rows(N)
    ga = H.Accumulator(N, px, "C1")
    ga.insert(rc, imgs, rows)
    fc = FinalCfg(molecular_mass_kda=300.0, inner_radius=0.0, outer_radius=0.45 * N * px, mask_falloff=0.0)
    first = ga.finalize(fc)
    for k in range(4):
        other = H.Accumulator(N + 16 * (k % 2) if N + 16 in BOXES else N, px, "C1")     # dirty the allocator between calls
        other.finalize(fc)
        other.close()
        again = ga.finalize(fc)
        assert np.array_equal(first[3][:, :3], again[3][:, :3])
        assert np.abs(first[3][:, 3:5] - again[3][:, 3:5]).max() < 1e-12
        for a, b in zip(first[:3], again[:3]):
            assert R.rel_l2(b, a) < 1e-6
    ga.close()


# ----------------------------------------------------------------------------------------------------------- leg B
def blob_volume(N, seed):
    """A few Gaussian blobs on the box grid (numpy, separable: no phantom at large boxes)."""
    rng = np.random.default_rng(seed)
    d = (np.arange(N) - N // 2).astype(np.float32)
    v = np.zeros((N, N, N), np.float32)
    for _ in range(6):
        c = rng.uniform(-0.2 * N, 0.2 * N, 3)
        s = rng.uniform(0.03, 0.08) * N
        gx, gy, gz = (np.exp(-(d - c[i]) ** 2 / (2 * s * s)).astype(np.float32) for i in range(3))
        v += rng.uniform(0.5, 1.5) * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return v


_POOL = {}


def _build(O, n):
    v = blob_volume(n, n)
    return v, O.Reference(v, n / 2)


@pytest.fixture(scope="module", autouse=True)
def _oracle_pool(O):
    """Oracle references of the large search boxes are built in a thread pool from the start of the module (the oracle's own
    FFT of N^3 takes ~50 s at 512 on one core and releases the GIL), while leg A runs; each is dropped after its test.  Three at
    a time: a build holds an N^3 complex64 work array, the N^3 volume and the (2B + 3)^2 (B + 2) cube, <= 2.3 GB at 512, so the
    pool adds <= 7 GB of host memory to leg A's own peak at 512 (float64 accumulators 3.2 GB, the download 1.6 GB, ~5 GB of
    float64 maps and spectra)."""
    O.fft1d(np.zeros(32, np.complex64))          # builds the oracle's FFT tables once, before any thread uses them
    ex = cf.ThreadPoolExecutor(max_workers=3)
    for n in SEARCH_ABOVE_256:
        _POOL[n] = ex.submit(_build, O, n)
    yield
    ex.shutdown(wait=True)
    _POOL.clear()


def oracle_reference(O, N):
    return _POOL.pop(N).result() if N in _POOL else _build(O, N)


SEARCH_BOXES = [n for n in BOXES if n <= 256] + list(SEARCH_ABOVE_256)


@pytest.mark.parametrize("N", SEARCH_BOXES)
def test_leg_b_search_path_vs_oracle(H, O, N):
    """Scores at given poses at two bands (B = N/2 - 1 and the ragged-chunk band of `ragged_band`), matching projections, and
    above 256 a local refinement and a small global search.  Score bound: the float32 round-off of a normalised sum over S
    in-band samples is ~ eps32 sqrt(S) relative; S <= pi (N/2)^2 / 2 = 1e5 at 512 gives ~2e-5, the bound of
    test_gpu_parity.py (2e-5) scaled by N / 64."""
    import torch
    vol, o = oracle_reference(O, N)
    px = 256.0 / N
    _, _, rows = R.seeded_particles(N, 4, 2000 + N)
    stack = synth.render_rows(vol, rows, px, snr=0.5, device="cuda")
    imgs = stack.cpu().numpy()
    del stack
    torch.cuda.empty_cache()
    g = H.Reference(vol, N / 2)
    tol = 2e-5 * max(1.0, N / 64)
    errs = {}
    for B in (N // 2 - 1, ragged_band(N)):
        c = RefineCfg.make(box=N, pixel_size=px, mask_radius=0.4 * N * px, res_high=N * px / (B + 0.5), global_search=0,
                           local_refine=0, res_signed_cc=30.0)
        want = O.score_batch(o, c, imgs, rows)
        got = g.refine(c, imgs, rows)[:, 14] / 100.0
        errs[B] = float(np.abs(want - got).max())
        assert errs[B] < tol, (N, B, prep_plan(N, B), errs[B])
    c = RefineCfg.make(box=N, pixel_size=px, mask_radius=0.4 * N * px, res_high=N * px / (N // 2 - 1.5))
    mw = O.match_projections(o, c, rows)
    mg = g.match_projections(c, rows)
    merr = R.rel_l2(mg, mw)
    report("B", N, score=errs, match=merr, plan=[prep_plan(N, B) for B in errs])
    assert merr < 1e-4, (N, merr)
    if N in SEARCH_ABOVE_256:
        band = 40.0
        cl = RefineCfg.make(box=N, pixel_size=px, mask_radius=0.4 * N * px, res_high=N * px / band, global_search=0,
                            res_signed_cc=30.0)
        start = synth.perturb_rows(rows, 2.0, 1.0, px, seed=N)
        w, _ = O.refine_batch(o, cl, imgs, start)
        gr = g.refine(cl, imgs, start)
        assert synth.angular_error_deg(w, gr).max() < ANG_TOL_DEG and synth.shift_error_px(w, gr, px).max() < SHIFT_TOL_PX
        cg = RefineCfg.make(box=N, pixel_size=px, mask_radius=0.4 * N * px, res_high=N * px / band, res_search=N * px / 16.0,
                            angular_step=30.0, search_range_x=6 * px, search_range_y=6 * px, res_signed_cc=30.0)
        w, _ = O.refine_batch(o, cg, imgs[:2], rows[:2])
        gr = g.refine(cg, imgs[:2], rows[:2])
        assert synth.angular_error_deg(w, gr).max() < ANG_TOL_DEG and synth.shift_error_px(w, gr, px).max() < SHIFT_TOL_PX
    g.close()
    o.close()


# ----------------------------------------------------------------------------------------------------------- leg C
@pytest.mark.parametrize("N", [30, 33, 34, 44, 52, 66, 514])
def test_leg_c_unsupported_boxes_are_refused(H, N):
    from pyp_amd import lib
    with pytest.raises((lib.PpmError, ValueError)):
        H.Accumulator(N, 1.0, "C1")
    with pytest.raises((lib.PpmError, ValueError)):
        H.Reference(np.zeros((N, N, N), np.float32))
    ok = H.Accumulator(32, 8.0, "C1")                                 # the process still works afterwards
    px, imgs, rows = R.seeded_particles(32, 2, 7)
    ok.insert(ReconCfg(box=32, pixel_size=8.0, res_limit=16.0, normalize=1, split_by_pind=1, mask_radius=100.0), imgs, rows)
    assert ok.counts() == [1, 1]
    ok.close()
