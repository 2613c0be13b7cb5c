"""Float64 restatement of ppm_local_resolution (include/ppm.h) in numpy: what tests/test_locres_cpu.py checks against
itself and tests/test_gpu_locres.py holds the GPU to.

  levels  lambda_min + i step <= lambda_max; lambda_min >= 2.5 pixels, lambda_max 0 = N a / 6, at most N a / 4, 1 .. 64 levels
  level   s = N a / lambda, l = lambda / a;  b(k) = exp(-(|k| - s)^2 / (2 sb^2)), sb = max(s / 8, 1.5), b(0) = 0;
          W(k) = exp(-2 pi^2 sw^2 |k|^2 / N^2), sw = max(l, 2) / 2;  both over the integer |k|^2, 1 / N^3 folded in, rounded to float32
          A = (H1 + H2) / 2, D = (H1 - H2) / 2 in float32;  A_l = IFFT(b FFT A);  E_A = Re IFFT(W FFT(A_l^2)); D likewise
          tau = the r-th smallest of max(E_D, 0) over the inside voxels, r = ceil((1 - p) n) in 1 .. n;  pass: inside and E_A > tau
  map     from the coarsest level down, alive <- alive and pass; a voxel still alive takes lambda (as float32); all others keep 100

The transforms are numpy.fft.fftn of the whole cube in float64 (unnormalised, like the library's, so that the rounded tables mean the
same), the order statistic is np.partition: nothing of the kernels' packing, histograms or counters is repeated here.
"""
import math

import numpy as np

UNASSIGNED = np.float32(100.0)
MAX_LEVELS = 64
PIXEL = 1.0
PLANTED = dict(levels=(3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0), p=0.05, res=(4.0, 8.0), seed=1)


class Refused(ValueError):
    pass


def levels(n, a, min_res=0.0, max_res=0.0, step=1.0):
    """(levels ascending in float64, notes)"""
    if not step >= 0.25:
        raise Refused("step below 0.25 A")
    notes = []
    lo, hi = float(min_res), float(max_res)
    if lo < 2.5 * a:
        lo = 2.5 * a
        notes.append("minimum raised")
    if hi == 0:
        hi = n * a / 6.0
        notes.append("maximum set")
    elif hi > n * a / 4.0:
        raise Refused("maximum above a quarter of the box")
    out = []
    i = 0
    while lo + i * step <= hi:
        out.append(lo + i * step)
        i += 1
    if not out or len(out) > MAX_LEVELS:
        raise Refused("%d levels" % len(out))
    return out, notes


def rank(p, n):
    return int(min(max(math.ceil((1.0 - p) * n), 1), n))


def k2_cube(n):
    k = np.fft.fftfreq(n, 1.0 / n).astype(np.int64)
    return (k * k)[:, None, None] + (k * k)[None, :, None] + (k * k)[None, None, :]


def tables(n, a, lam):
    """(band, window) over |k|^2 = 0 .. 3 (N/2)^2 as float32"""
    k2 = np.arange(3 * (n // 2) ** 2 + 1, dtype=np.float64)
    inv = 1.0 / (float(n) * n * n)
    s, l = n * a / lam, lam / a
    sb, sw = max(s / 8.0, 1.5), max(l, 2.0) / 2.0
    d = np.sqrt(k2) - s
    band = (np.exp(-(d * d) / (2.0 * sb * sb)) * inv).astype(np.float32)
    band[0] = 0.0
    cw = 2.0 * math.pi * math.pi * sw * sw / (float(n) * n)
    window = (np.exp(-(cw * k2)) * inv).astype(np.float32)
    return band, window


def inside_of(n, mask=None):
    if mask is not None:
        return np.asarray(mask, dtype=np.float32) > np.float32(0.5)
    g = np.arange(n) - n // 2
    d2 = (g * g)[:, None, None] + (g * g)[None, :, None] + (g * g)[None, None, :]
    return 4 * d2 < n * n


def energies(h1, h2, a, lam, k2=None):
    """(E_A, E_D) of one level in float64"""
    n = h1.shape[0]
    k2 = k2_cube(n) if k2 is None else k2
    half = np.float32(0.5)
    A = (half * (h1.astype(np.float32) + h2.astype(np.float32))).astype(np.float64)
    D = (half * (h1.astype(np.float32) - h2.astype(np.float32))).astype(np.float64)
    band, window = tables(n, a, lam)
    b, w = band.astype(np.float64)[k2], window.astype(np.float64)[k2]
    n3 = float(n) ** 3
    out = []
    for M in (A, D):
        Ml = np.fft.ifftn(np.fft.fftn(M) * b).real * n3
        out.append(np.fft.ifftn(np.fft.fftn(Ml * Ml) * w).real * n3)
    return out[0], out[1]


def run(h1, h2, a, p, lv, mask=None, keep=True):
    """The whole definition for the levels lv (ascending).  Returns dict(levels float32, E_A, E_D = [L] float64 cubes (keep), tau [L]
    float64, resolution float32 cube, counts [L], n_inside, unassigned, median, inside)."""
    n = h1.shape[0]
    ins = inside_of(n, mask)
    n_in = int(ins.sum())
    if n_in == 0:
        raise Refused("no inside voxel")
    r = rank(p, n_in)
    k2 = k2_cube(n)
    L = len(lv)
    lv32 = np.asarray(lv, dtype=np.float64).astype(np.float32)
    EA, ED, tau = [None] * L, [None] * L, np.zeros(L)
    res = np.full((n, n, n), UNASSIGNED, dtype=np.float32)
    alive = ins.copy()
    for i in range(L - 1, -1, -1):
        ea, ed = energies(h1, h2, a, lv[i], k2)
        tau[i] = np.partition(np.maximum(ed[ins], 0.0), r - 1)[r - 1]
        alive &= ea > tau[i]
        res[alive] = lv32[i]
        if keep:
            EA[i], ED[i] = ea, ed
    counts = np.array([int((res[ins] == v).sum()) for v in lv32], dtype=np.int64)
    vals = np.sort(res[ins])
    return dict(levels=lv32, E_A=EA, E_D=ED, tau=tau, resolution=res, counts=counts, n_inside=n_in, unassigned=int((res[ins] == UNASSIGNED).sum()),
                median=float(vals[(n_in + 1) // 2 - 1]), inside=ins)


def undecided(ref, B):
    """Voxels whose map value round-off of size B x max E_A may change: |E_A - tau| <= 2 B max(E_A over the inside) at some level."""
    u = np.zeros(ref["inside"].shape, dtype=bool)
    for ea, t in zip(ref["E_A"], ref["tau"]):
        u |= np.abs(ea - t) <= 2.0 * B * float(ea[ref["inside"]].max())
    return u & ref["inside"]


def backend(h1, h2, cfg, mask=None):
    """What cli.resmap_main takes as `backend`: the dict of host.local_resolution from this module (cfg: abi.LocresCfg)."""
    from pyp_amd import abi
    n = h1.shape[0]
    lv, notes = levels(n, cfg.pixel_size, cfg.min_res, cfg.max_res, cfg.step)
    ref = run(h1, h2, cfg.pixel_size, cfg.p_value, lv, mask=mask, keep=False)
    info = abi.LocresInfo(n_levels=len(lv), transforms=1 + 3 * len(lv), n_inside=ref["n_inside"], unassigned=ref["unassigned"], median=ref["median"],
                          notes="; ".join(notes).encode())
    for i in range(len(lv)):
        info.levels[i], info.tau[i], info.counts[i] = ref["levels"][i], ref["tau"][i], ref["counts"][i]
    return dict(resolution=ref["resolution"], levels=ref["levels"], tau=ref["tau"].astype(np.float32), counts=ref["counts"], info=info)


# ------------------------------------------------------------------------------------------ generator
def lowpass_sharp(v, a, res):
    """Strictly band-limited: every coefficient with |k| > N a / res is zero."""
    n = v.shape[0]
    keep = k2_cube(n) <= (n * a / res) ** 2
    return np.fft.ifftn(np.fft.fftn(v) * keep).real


def blob_mask(n, cx, radius):
    """Sphere of `radius` voxels about (x, y, z) = (N/2 + cx, N/2, N/2); arrays are [z, y, x]."""
    g = np.arange(n) - n // 2
    d2 = (g * g)[:, None, None] + (g * g)[None, :, None] + ((g - cx) ** 2)[None, None, :]
    return d2 < radius * radius


def make_halves(n, seed=1, a=PIXEL, res=PLANTED["res"]):
    """Two blobs of radius N/8 at x = -N/4 and +N/4: white Gaussian noise inside the blob, low-passed *after* the blob mask to res[0] and
    res[1] A (strictly band-limited).  The signal, both blobs together, is scaled to sigma 1 over the voxels of its blobs, and each half
    gets independent white noise of that sigma.  float32."""
    rng = np.random.default_rng(seed)
    sig = np.zeros((n, n, n))
    both = np.zeros((n, n, n), dtype=bool)
    for cx, r in zip((-(n // 4), n // 4), res):
        m = blob_mask(n, cx, n / 8.0)
        both |= m
        sig += lowpass_sharp(rng.standard_normal((n, n, n)) * m, a, r)
    sig /= sig[both].std()
    h1 = sig + rng.standard_normal((n, n, n))
    h2 = sig + rng.standard_normal((n, n, n))
    return h1.astype(np.float32), h2.astype(np.float32)


def make_mask(n, radius_frac=0.42):
    """An external mask: 1 inside a sphere of radius_frac N, a linear edge of 3 voxels (values between 0 and 1 on it), 0 outside."""
    g = np.arange(n) - n // 2
    d = np.sqrt(((g * g)[:, None, None] + (g * g)[None, :, None] + (g * g)[None, None, :]).astype(np.float64))
    return np.clip((radius_frac * n + 1.5 - d) / 3.0, 0.0, 1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------ the cases of tests/test_gpu_locres.py
GPU_BOXES = (32, 48, 70)        # the smallest box of the transforms; 48; 70 = 2 x 5 x 7, rows of 35 pairs: no multiple of a wavefront or of four floats
GPU_P = 0.05
UNDECIDED_CAP = 0.02            # of the inside voxels
# Largest error of the GPU against this module, relative to max(E_A over the inside voxels), over the levels and boxes of the GPU cases as
# measured on an MI355X (CHANGELOG.md), and the factor the bounds hold over it (other seeds, the boxes in between).
MEASURED = dict(E_A=4.97e-7, E_D=5.46e-7, tau=2.91e-7)
FACTOR = 16.0
B_E_A, B_E_D, B_TAU = (FACTOR * MEASURED[k] for k in ("E_A", "E_D", "tau"))
B_UNDECIDED = max(B_E_A, B_TAU)


def gpu_level_grid(n, a=PIXEL):
    """(min_res, max_res, step) of a GPU case: 4 levels from 2.5 pixels (s = 0.4 N, the upper end of the band table; sb = s / 8 above
    s = 12) to N a / 5 (s = 5, sb on its floor of 1.5).  sw = l / 2: its floor max(l, 2) never binds above 2.5 pixels."""
    lo, hi = 2.5 * a, n * a / 5.0
    return lo, hi + 1e-9, (hi - lo) / 3.0


_cases = {}


def gpu_inputs(n, masked):
    h1, h2 = make_halves(n, 1)
    return h1, h2, (make_mask(n) if masked else None)


def gpu_case(n, masked):
    """The float64 result of a GPU case, computed once."""
    if (n, masked) not in _cases:
        h1, h2, m = gpu_inputs(n, masked)
        lv, _ = levels(n, PIXEL, *gpu_level_grid(n))
        _cases[(n, masked)] = run(h1, h2, PIXEL, GPU_P, lv, mask=m)
    return _cases[(n, masked)]
