"""Float64 restatement of ppm_resample, ppm_resize, ppm_fit_plan and ppm_fit_volume (include/ppm.h) in numpy: what
tests/test_resample_cpu.py checks against mathematics and tests/test_gpu_resample.py holds the GPU to.

  resample, per axis: X = unnormalised DFT of a line of N samples, K = min(N, M), h = K / 2;  Y[k mod M] = X[k mod N] for |k| < h;
      the Nyquist term of the smaller grid Y[h] = X[h] + X[N - h] (M < N), Y[h] = Y[M - h] = X[h] / 2 (M > N), Y = X (M = N);
      all else 0;  y = (1 / N) IDFT_M(Y).
  resize: out[i] = in[i - B // 2 + N // 2] per axis where inside, elsewhere the mean of the face (3-D) / edge (2-D, per image)
      voxels, every voxel once; normalize: (x - mean) / std of the item first.
  fit: s = a_in / a_out, n_c = min(n_in, 2 ceil(B / (2 s)) + 2), (P, M) supported with P >= n_c minimising |M / (P s) - 1|
      (ties: smaller P M, then smaller P), refused above 0.01; resize n_in -> P, resample P -> M, resize M -> B.
"""
import math

import numpy as np

import f64_ref as R

EPS32 = R.EPS32
FIT_TOLERANCE = 0.01


class Refused(ValueError):
    pass


def box_ok(n):
    if n < 32 or n > 512 or n % 2:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


SIZES = [n for n in range(32, 513, 2) if box_ok(n)]


# ------------------------------------------------------------------------------------------ resample
def resample_axis(x, m, axis):
    """The 1-D rule along `axis`; complex in, complex out (the rule is linear over the complex numbers)."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    n = x.shape[-1]
    X = np.fft.fft(x.astype(np.complex128), axis=-1)
    if m == n:
        Y = X
    else:
        Y = np.zeros(x.shape[:-1] + (m,), dtype=np.complex128)
        h = min(n, m) // 2
        Y[..., :h] = X[..., :h]
        if h > 1:
            Y[..., m - h + 1:] = X[..., n - h + 1:]
        if m < n:
            Y[..., h] = X[..., h] + X[..., n - h]
        else:
            Y[..., h] = 0.5 * X[..., h]
            Y[..., m - h] = 0.5 * X[..., h]
    y = np.fft.ifft(Y, axis=-1) * (m / n)
    return np.moveaxis(y, -1, axis)


def resample(x, m, dims=None):
    """Real input; the last `dims` axes (default: all) are resampled to m.  float64."""
    x = np.asarray(x, dtype=np.float64)
    dims = x.ndim if dims is None else dims
    y = x.astype(np.complex128)
    for ax in range(x.ndim - dims, x.ndim):
        y = resample_axis(y, m, ax)
    return np.ascontiguousarray(y.real)


# ------------------------------------------------------------------------------------------ resize
def face_mask(n, dims):
    idx = np.arange(n)
    e = (idx == 0) | (idx == n - 1)
    if dims == 2:
        return e[:, None] | e[None, :]
    return e[:, None, None] | e[None, :, None] | e[None, None, :]


def face_mean(item):
    """Mean of the face / edge voxels of one item (2-D or 3-D), every voxel once, float64."""
    a = np.asarray(item, dtype=np.float64)
    return float(a[face_mask(a.shape[0], a.ndim)].mean())


def resize_item(item, b, normalize=False):
    a = np.asarray(item, dtype=np.float64)
    n, d = a.shape[0], a.ndim
    if normalize:
        sd = float(a.std())
        if not sd > 0:
            raise Refused("ERROR: resize: an item has a standard deviation of 0 and cannot be normalised")
        a = (a - a.mean()) / sd
    pad = face_mean(a)
    out = np.full((b,) * d, pad, dtype=np.float64)
    off = n // 2 - b // 2                                 # out[i] = in[i + off]
    lo_o, hi_o = max(0, -off), min(b, n - off)
    sl_o = (slice(lo_o, hi_o),) * d
    sl_i = (slice(lo_o + off, hi_o + off),) * d
    out[sl_o] = a[sl_i]
    return out, pad


def resize(x, b, normalize=False, volume=False):
    """x: one image (2-D), a stack (3-D) or a volume (3-D with volume=True) -> (out float64, pad values [items])."""
    x = np.asarray(x)
    if x.ndim == 2 or (x.ndim == 3 and volume):
        o, p = resize_item(x, b, normalize)
        return o, np.array([p])
    outs, pads = zip(*(resize_item(im, b, normalize) for im in x))
    return np.stack(outs), np.array(pads)


# ------------------------------------------------------------------------------------------ fit
def fit_plan(n_in, pixel_in, pixel_out, box_out):
    """dict(n_c, P, M, scale, pixel_achieved, rel_error, ok): the search of DESIGN.md §2f, in the arithmetic of ppm_resample_plan.h."""
    s = pixel_in / pixel_out
    n_c = min(n_in, 2 * int(math.ceil(box_out / (2.0 * s))) + 2)
    best, bp, bm = None, 0, 0
    for P in SIZES:
        if P < n_c:
            continue
        for M in SIZES:
            err = abs(M / (P * s) - 1.0)
            if best is None or err < best or (err == best and (P * M < bp * bm or (P * M == bp * bm and P < bp))):
                best, bp, bm = err, P, M
    if best is None:
        return dict(n_c=n_c, P=0, M=0, scale=s, pixel_achieved=0.0, rel_error=0.0, ok=False)
    return dict(n_c=n_c, P=bp, M=bm, scale=s, pixel_achieved=pixel_in * bp / bm, rel_error=best, ok=best <= FIT_TOLERANCE)


def fit(vol, pixel_in, pixel_out, box_out):
    """(map float64 [B, B, B], info): the chain resize n_in -> P, resample P -> M, resize M -> B."""
    vol = np.asarray(vol)
    p = fit_plan(vol.shape[0], pixel_in, pixel_out, box_out)
    if not p["ok"]:
        raise Refused("ERROR: fit: the best pair %d -> %d is %.2f %% off" % (p["P"], p["M"], 100 * p["rel_error"]))
    a, pad1 = resize_item(vol, p["P"])
    b = resample(a, p["M"])
    c, pad2 = resize_item(b, box_out)
    info = dict(p, pad_value_1=pad1, pad_value_2=pad2, stage_max=(float(np.abs(a).max()), float(np.abs(b).max())))
    return c, info


# ------------------------------------------------------------------------------------------ bounds
def floor_model_resample(n, m, d):
    """Relative to max|x|: d axes, along each a forward transform of log2 N butterfly stages and an inverse of log2 M, one float32
    rounding per stage along a path (the model of f64_mask.floor_model_mask)."""
    return EPS32 * d * (math.log2(n) + math.log2(m))


def bound_resample(n, m, d, x):
    return R.MAP_K * floor_model_resample(n, m, d) * float(np.abs(x).max())


# ------------------------------------------------------------------------------------------ inputs of the tests
def make_items(shape, seed=11):
    """Seeded noise plus a blob plus an offset; the last len(shape) - 1 or all axes are the item (a stack's first axis counts items)."""
    rng = np.random.default_rng(seed)
    n = shape[-1]
    grids = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    r2 = sum((g - c * n) ** 2 for g, c in zip(grids[-2:], (0.55, 0.45)))
    if len(shape) == 3:
        r2 = r2 + (grids[0] - 0.5 * shape[0]) ** 2 * (1.0 if shape[0] == n else 0.0)
    blob = np.exp(-r2 / (2 * (0.15 * n) ** 2))
    return (0.5 * rng.standard_normal(shape) + 3.0 * blob + 1.25).astype(np.float32)


def cosines(n, m, d, seed=3, terms=4):
    """A sum of cosines of random amplitude and phase at frequency vectors with every |component| < K / 2 (strictly inside the band
    of both grids): returns (samples on the n^d grid, analytic samples at t = j n / m on the m^d grid), float64."""
    rng = np.random.default_rng(seed)
    h = min(n, m) // 2
    src, dst = np.zeros((n,) * d), np.zeros((m,) * d)
    gs = np.meshgrid(*(np.arange(n, dtype=np.float64),) * d, indexing="ij")
    gd = np.meshgrid(*(np.arange(m, dtype=np.float64) * n / m,) * d, indexing="ij")
    for _ in range(terms):
        k = rng.integers(-(h - 1), h, size=d)
        amp, ph = rng.uniform(0.5, 2.0), rng.uniform(0, 2 * math.pi)
        src += amp * np.cos(2 * math.pi * sum(ki * g for ki, g in zip(k, gs)) / n + ph)
        dst += amp * np.cos(2 * math.pi * sum(ki * g for ki, g in zip(k, gd)) / n + ph)
    return src, dst


def nyquist(n, m, d, phases=None):
    """The pure Nyquist pattern of the smaller grid along every axis: prod_a cos(pi x_a + phi_a) with x in units of the COARSER grid's
    sample.  Returns (samples on the n^d grid, what the rule gives on the m^d grid = prod_a cos(phi_a) cos(pi t_a), t at the
    output's sample positions).  Downsampling (m < n): the pattern lives on the output grid and is cos(pi K x / n) on the input."""
    phases = [0.4 + 0.7 * a for a in range(d)] if phases is None else phases
    K = min(n, m)
    xs = np.arange(n, dtype=np.float64) * K / n            # in coarse samples
    xd = np.arange(m, dtype=np.float64) * K / m
    src, dst = np.ones((n,) * d), np.ones((m,) * d)
    for a, ph in enumerate(phases):
        sh = [1] * d
        sh[a] = -1
        src = src * np.cos(math.pi * xs + ph).reshape(sh)
        dst = dst * (math.cos(ph) * np.cos(math.pi * xd)).reshape(sh)
    return src, dst
