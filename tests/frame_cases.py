"""Inputs and references of the movie-frame refinement tests (ppm_frame_refine; tests/test_frames_cpu.py, tests/test_gpu_frames.py).

The yardstick of an OWN MAP is the oracle's own score in double: a score-only pass with res_signed_cc = 0 at a row whose X / Y shift was
moved by d a IS S_r(d) (`oracle_maps`: one O.score_batch call per grid point).  The yardstick of pooling and peak is pyp_amd/frames.py
applied in float64 to those maps (`reference`).  Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

from pyp_amd import frames as F
from pyp_amd import synth
from pyp_amd.abi import FrameCfg, RefineCfg
from pyp_amd.formats import cistem

import defocus_cases as D

C = cistem.COL
PX = 1.5
RHI = 20.0                  # band in Fourier pixels
STEP, RANGE = 0.5, 2.0      # grid: h = 0.5, W = 4, 81 points
SNR = 0.2
TILTS = (-20.0, 0.0, 20.0)


def tol(n):
    """The project's score tolerance (tests/defocus_cases.py): the own map is the same normalised sum."""
    return D.tol(n)


def cfg_for(n, rhi=RHI, px=PX):
    return RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / rhi, res_signed_cc=0.0, global_search=0, local_refine=0)


def fcfg(half_width=2, range_px=RANGE, step_px=STEP, **kw):
    return FrameCfg.make(range_px, step_px, half_width, **kw)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def series(n=64, n_part=4, n_frames=7, defocus_jump=False, tilts=TILTS):
    """(vol, images, start rows, true rows) of the common case: make_tilt_series(n, n_part, tilts) tiled over n_frames frames with planted
    drifts.  defocus_jump: frame 3 of the first group gets a defocus 300 A off its neighbours (rendered with it, too)."""
    vol, stack, rows, true, _, _ = synth.make_frame_series(n, n_part, list(tilts), n_frames, pixel=PX, snr=SNR, vol=D.volume(n))
    imgs = stack.numpy()
    if defocus_jump:
        rows, true = rows.copy(), true.copy()
        for r in (rows, true):
            r[3, C["DEFOCUS_1"]] += 300.0
            r[3, C["DEFOCUS_2"]] += 300.0
        imgs = imgs.copy()
        imgs[3] = synth.render_rows(vol, true[3:4], PX, SNR, 99).numpy()[0]
    return (vol,) + _freeze(imgs, rows, true)


TILE, LDS_STORE_MAX = 2048, 3968     # kFrameTile; the most samples whose slice store fits LDS beside a tile (ppm_frame_kernels.h)


def list_length(rhi):
    """Length of the ring-ordered sample list of the band 0 < |k| < rhi (half plane kx >= 0, every ring padded to 16 samples)."""
    b = int(np.ceil(rhi))
    ky, kx = np.mgrid[-b:b + 1, 0:b + 1]
    k2 = kx * kx + ky * ky
    ring = np.floor(np.sqrt(k2[(k2 > 0) & (k2 < rhi * rhi)])).astype(int)
    return int(sum(-(-c // 16) * 16 for c in np.bincount(ring)))


def oracle_maps(O, oref, cfg, imgs, rows, h, W):
    """S_r(d) of every row over the grid, float64 (M, 2W + 1, 2W + 1), row-major (jy, jx); zeros for rows with OCCUPANCY <= 0."""
    side = 2 * W + 1
    out = np.zeros((len(rows), side, side))
    use = rows[:, C["OCCUPANCY"]] > 0
    for jy in range(side):
        for jx in range(side):
            r = rows.copy()
            r[:, C["X_SHIFT"]] += (jx - W) * h * cfg.pixel_size
            r[:, C["Y_SHIFT"]] += (jy - W) * h * cfg.pixel_size
            out[use, jy, jx] = O.score_batch(oref, cfg, imgs[use], r[use])
    return out


@functools.lru_cache(maxsize=None)
def common_maps(n=64, n_part=4, n_frames=7, defocus_jump=False, rhi=RHI, tilts=TILTS):
    """The oracle's own maps of `series(...)` on the grid h = 0.5, W = 4."""
    from oracle import oracle as O
    vol, imgs, rows, _ = series(n, n_part, n_frames, defocus_jump, tilts)
    h, W, _ = F.plan(RANGE, STEP)
    m = oracle_maps(O, O.Reference(vol, n / 2), cfg_for(n, rhi), imgs, rows, h, W)
    m.setflags(write=False)
    return m


def reference(rows, maps, half_width, h=STEP, px=PX, **kw):
    """frames.pool_and_peak in float64 on the given (oracle) maps, plus per row the margin between the best and the second-best pooled
    value (inf for rows without a map)."""
    ref = F.pool_and_peak(rows, maps, h, half_width, px, **kw)
    margin = np.full(len(rows), np.inf)
    for j in np.flatnonzero(ref["index"] >= 0):
        v = np.sort(ref["pooled"][j].ravel())
        margin[j] = v[-1] - v[-2] if len(v) > 1 else np.inf
    ref["margin"] = margin
    return ref


def shift_error_px(rows, true, px=PX):
    d = rows[:, [C["X_SHIFT"], C["Y_SHIFT"]]] - true[:, [C["X_SHIFT"], C["Y_SHIFT"]]]
    return np.sqrt((d ** 2).sum(axis=1)) / px
