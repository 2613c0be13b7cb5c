"""Float64 restatement of ppm_mask_volume (include/ppm.h) in numpy: what tests/test_mask_cpu.py checks against itself
and tests/test_gpu_mask.py holds the GPU to.

  core = {M >= 0.5} (compared in float32);  d = Euclidean distance in voxels to the nearest core voxel, no wrap-around
  s    = max(clip(M, 0, 1), (1 + cos(pi d / w)) / 2 where d < w)                    (w = 0: the clip alone)
  O    = V, or Re IFFT3(H FFT3(V)) with the cosine-edge low-pass H(|k|) around r_c = N a / R Fourier pixels, e wide
  out  = s V + (1 - s) g O

The distances are integers: `sqdist_windowed` is the scheme of the kernels (three separable min-plus passes over windows of +-w,
saturated at w^2, int64), `sqdist_brute` the definition itself; they agree wherever d < w, and the GPU agrees with both bit for bit.

Error model of the filtered output (`floor_model_mask`), in the manner of f64_sva.floor_model_sva: see there.
"""
import math

import numpy as np

import f64_ref as R

EPS32 = R.EPS32


# ------------------------------------------------------------------------------------------ distances
def core_of(mask):
    return np.asarray(mask, dtype=np.float32) >= np.float32(0.5)


def sqdist_brute(core):
    """Exact squared distance (int64) of every voxel to the nearest core voxel, by definition: O(N^3 x core voxels), small boxes only.
    Without a core voxel: a value above any d^2 of the box."""
    n = core.shape[0]
    pts = np.argwhere(core).astype(np.int64)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.int64),) * 3, indexing="ij")
    best = np.full(core.shape, 3 * n * n + 1, dtype=np.int64)
    for pz, py, px in pts:
        np.minimum(best, (z - pz) ** 2 + (y - py) ** 2 + (x - px) ** 2, out=best)
    return best


def _minplus(d, axis, w):
    """min over |k| <= w of d shifted by k along `axis`, plus k^2, saturated at w^2; nothing comes in over the faces."""
    w2 = w * w
    out = np.minimum(d, w2)
    n = d.shape[axis]
    for k in range(1, min(w, n - 1) + 1):
        lo = [slice(None)] * d.ndim
        hi = [slice(None)] * d.ndim
        lo[axis], hi[axis] = slice(0, n - k), slice(k, n)
        lo, hi = tuple(lo), tuple(hi)
        np.minimum(out[lo], d[hi] + k * k, out=out[lo])      # the neighbour at +k
        np.minimum(out[hi], d[lo] + k * k, out=out[hi])      # the neighbour at -k
    return out


def sqdist_windowed(core, w):
    """The kernels' scheme, int64: x pass on the core flags, then y and z min-plus passes, every window +-w, every value saturated at
    w^2.  Exact wherever d < w (each component of the offset to the nearest core voxel is then below w), w^2 elsewhere.  Only what
    the windows can reach is computed - of every z plane that holds core voxels, the bounding rectangle of its core plus w, and from
    there the planes within w - the rest stays at w^2: the same numbers, and a 512^3 box with a compact core costs what its core
    costs."""
    n = core.shape[0]
    w2 = w * w
    out = np.full(core.shape, w2, dtype=np.int64)
    if w == 0:
        return out
    for z0 in np.flatnonzero(core.reshape(n, -1).any(axis=1)):
        ys, xs = np.flatnonzero(core[z0].any(axis=1)), np.flatnonzero(core[z0].any(axis=0))
        y0, y1, x0, x1 = max(0, ys[0] - w), min(n, ys[-1] + w + 1), max(0, xs[0] - w), min(n, xs[-1] + w + 1)
        d = np.where(core[z0, y0:y1, x0:x1], 0, w2).astype(np.int64)
        d = _minplus(_minplus(d, 1, w), 0, w)                  # x, then y
        for k in range(-w + 1, w):                             # the z pass, scattered; |k| = w only brings w^2
            if 0 <= z0 + k < n:
                o = out[z0 + k, y0:y1, x0:x1]
                np.minimum(o, d + k * k, out=o)
    return out


def edge_table(w):
    """edge[d^2] for the integer d^2 < w^2, float64."""
    d2 = np.arange(w * w, dtype=np.float64)
    return 0.5 * (1.0 + np.cos(math.pi * np.sqrt(d2) / w))


def soft_mask(mask, w, d2=None):
    """s in float64 (full volume).  d2: squared distances if the caller has them already."""
    m = np.clip(np.asarray(mask, dtype=np.float32), 0.0, 1.0).astype(np.float64)
    if w == 0:
        return m
    if d2 is None:
        d2 = sqdist_windowed(core_of(mask), w)
    tab = np.concatenate([edge_table(w), [0.0]])
    return np.maximum(m, tab[np.minimum(d2, w * w)])


# ------------------------------------------------------------------------------------------ outside density
def lowpass_H(r, r_c, e):
    """H(r): 1 up to r_c - e/2, 0 from r_c + e/2, a raised cosine in between (e = 0: 1 up to and including r_c)."""
    r = np.asarray(r, dtype=np.float64)
    r_one, r_end = r_c - 0.5 * e, r_c + 0.5 * e
    h = np.zeros_like(r)
    h[r <= r_one] = 1.0
    band = (r > r_one) & (r < r_end)
    if e > 0:
        h[band] = 0.5 * (1.0 + np.cos(math.pi * (r[band] - r_one) / e))
    return h


def outside_fft(vol, pixel, radius_A, edge_px):
    """O = Re IFFT3(H FFT3(V)) with numpy.fft in float64 (signed indices in [-N/2, N/2))."""
    v = np.asarray(vol, dtype=np.float64)
    n = v.shape[0]
    k = np.fft.fftfreq(n, 1.0 / n)
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
    H = lowpass_H(np.sqrt(kx * kx + ky * ky + kz * kz), n * pixel / radius_A, edge_px)
    return np.fft.ifftn(np.fft.fftn(v) * H).real


def outside_dft(vol, pixel, radius_A, edge_px):
    """The same O by direct float64 Fourier sums over the cube of frequencies |k_i| <= K that holds the support of H (K = the last
    integer radius below r_c + e/2): three separable matrix products forwards, three back.  For a filter that keeps few Fourier pixels
    of a large box (K = 14 at 512^3: 29 of 512 frequencies per axis) this is a few seconds where the full transforms take a quarter of
    a minute; test_mask_cpu.py holds it to outside_fft."""
    n = vol.shape[0]
    v = np.asarray(vol, dtype=np.float64).reshape(n * n, n)
    r_c = n * pixel / radius_A
    K = min(n // 2 - 1, int(math.floor(r_c + 0.5 * edge_px)))
    k = np.arange(-K, K + 1, dtype=np.float64)
    nk = len(k)
    ph = 2.0 * math.pi * np.outer(np.arange(n, dtype=np.float64), k) / n        # [n, nk]
    c, sn = np.cos(ph), np.sin(ph)                                               # contiguous real factors: the big products go through BLAS
    E = c - 1j * sn                                                              # forward kernel; its conjugate goes back
    f = ((v @ c) - 1j * (v @ sn)).reshape(n, n, nk)                              # x -> kx : [z, y, kx]
    f = np.matmul(E.T[None], f)                                                  # y -> ky : [z, ky, kx]
    f = (E.T @ f.reshape(n, nk * nk)).reshape(nk, nk, nk)                        # z -> kz : [kz, ky, kx]
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
    f *= lowpass_H(np.sqrt(kx * kx + ky * ky + kz * kz), r_c, edge_px) / float(n) ** 3
    Ei = np.conj(E)
    f = (Ei @ f.reshape(nk, nk * nk)).reshape(n, nk, nk)                         # kz -> z
    f = np.matmul(Ei[None], f).reshape(n * n, nk)                                # ky -> y
    out = np.ascontiguousarray(f.real) @ np.ascontiguousarray(c.T) - np.ascontiguousarray(f.imag) @ np.ascontiguousarray(sn.T)   # kx -> x, real part
    return out.reshape(n, n, n)


# ------------------------------------------------------------------------------------------ the whole definition
def mask_volume(vol, mask, pixel=1.0, w=3, g=0.0, filt=0, radius_A=10.0, edge_px=10.0, outside=None, s=None):
    """out in float64.  outside / s: precomputed O / s (the tests share them between cases)."""
    v = np.asarray(vol, dtype=np.float32).astype(np.float64)
    if s is None:
        s = soft_mask(mask, w)
    if outside is None:
        outside = v if filt == 0 else outside_fft(v, pixel, radius_A, edge_px)
    return s * v + (1.0 - s) * (g * outside)


# ------------------------------------------------------------------------------------------ bounds
def bound_unfiltered(vol, g):
    """Filter 0: s is the correctly rounded table value, the blend two products and a sum in float32 - 3.5 roundings, 2.1e-7 of
    max|V| (1 + |g|); the bound is 1e-6 of it."""
    return 1e-6 * float(np.abs(vol).max()) * (1.0 + abs(g))


def floor_model_mask(N, hardware_cosine=False):
    """Relative to max|O|: the error of O on the GPU.  Six float32 line-transform passes (three forwards, three back), each a
    log2 N-stage butterfly network with one rounding per stage along a path: EPS32 x 6 log2 N.  H comes from a table built in
    float64 and rounded once, which this absorbs (as it does the 3.5 roundings of the blend); a kernel that evaluated the cosine in
    hardware would add 1e-6.  The filtered output is held to f64_ref.MAP_K x this x max|O|."""
    return EPS32 * 6.0 * math.log2(N) + (1e-6 if hardware_cosine else 0.0)


def bound_filtered(N, outside):
    return R.MAP_K * floor_model_mask(N) * float(np.abs(outside).max())


# ------------------------------------------------------------------------------------------ inputs of the tests
def make_map(n, seed=7):
    """Seeded noise plus a blob."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float32),) * 3, indexing="ij")
    c = 0.45 * n
    blob = np.exp(-((x - c) ** 2 + (y - 0.55 * n) ** 2 + (z - c) ** 2) / (2 * (0.15 * n) ** 2)).astype(np.float32)
    return (rng.standard_normal((n, n, n)).astype(np.float32) * np.float32(0.5) + np.float32(3.0) * blob).astype(np.float32)


def make_mask(n):
    """Binary: a ball off-centre, and single core voxels at two opposite corners and in the middle of the face x = 0 (wrap-around,
    window clipping)."""
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    m = ((x - 0.6 * n) ** 2 + (y - 0.45 * n) ** 2 + (z - 0.55 * n) ** 2 <= (0.2 * n) ** 2).astype(np.float32)
    m[0, 0, 0] = m[n - 1, n - 1, n - 1] = m[n // 2, n // 2, 0] = 1.0
    return m
