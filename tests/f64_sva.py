"""(Test infrastructure: a float64 restatement of the sub-tomogram average and of the alignment score at a given pose; nothing in
pyp_amd imports it.)

The same operations as orc_sva_insert, orc_reference_create and orc_sva_align with tol_angle = tol_shift = 0 (oracle/ppm_oracle.c),
taken from the conventions of include/ppm.h (ppm_sva_cfg, ppm_sva_insert) and written again in plain numpy with every intermediate in
float64 (the forward transforms run through torch.fft in float64, as f64_ref.finalize does, and the sampler's element-wise
work through torch's float64 tensor operations, for their threads).  The oracle computes positions in double
but stores volumes, transforms and accumulators in float32; the kernels hold positions in float32 too.  This module does neither, so
it is the yardstick for both.

Layouts: an accumulator is [2][N][N][N/2+1][3] {re, im, weight} with qz, qy stored at index q + N/2 (f64_ref.py); a transform is the
half space T[kz mod N][ky mod N][kx = 0 .. N/2] of the centred transform F(k) = (-1)^(kx+ky+kz) fftn(v)[k], its other half being
conj F(-k); a pose is 12 doubles {N row-major, shift x y z}: F_v(k) = Ref(N k) e^{+2 pi i k.p / N}.

The band weights of the score are used as the C ABI stores them (a float per sample), like every config value.

Wedge limits: the wedge test compares atan2(kz, kx) with the limits.  For the average k = N^T S^T q is irrational and the test is
undecided only within rounding of a limit plane: `near_wedge` names those voxels (within `margin` pixels of a plane) and the
comparisons leave them out.  For the score k is an integer triple, and a limit whose tangent is rational (0, +-45, +-90 degrees) lies
exactly ON samples, where atan2f and atan2 may round to different sides of it.  Such ties are left out of this yardstick: the seeded
inputs use the limits (-54, 60) and (-40, 47) only.
"""
import functools
import math

import numpy as np

import f64_ref as R

EPS32 = R.EPS32
WEDGES = ((-54.0, 60.0), (-40.0, 47.0))
MARGIN = 1e-3                  # pixels from a wedge-limit plane inside which a voxel is left out of a comparison
EXCLUDED_CAP = 5e-3            # of the in-band voxels (the reference alone leaves out 4e-4 .. 9e-4 for 4 - 6 sub-volumes)
CHUNK = 1 << 21


# ------------------------------------------------------------------------------------------------ transforms
def _rfftn_centred(x):
    """rfftn of a real [z][y][x] array with the origin at the box centre: (-1)^(kx+ky+kz) fftn(v) is the transform of v rolled by N/2
    along every axis (N even), so the roll is made on the real side."""
    import torch
    return torch.fft.rfftn(torch.from_numpy(np.fft.fftshift(np.asarray(x, dtype=np.float64)))).numpy()


def window(N, cfg):
    """The separable real-space window [z][y][x] of an alignment: 1 inside window[k], exp(-d^2 / 2 sigma^2) outside (0 when sigma = 0),
    no window along an axis whose window[k] <= 0."""
    c = np.abs(np.arange(N) - N // 2).astype(np.float64)
    sg = float(cfg.window_sigma)
    ax = []
    for k in range(3):
        wk = float(cfg.window[k])
        if not wk > 0:
            ax.append(np.ones(N))
            continue
        d = c - wk
        out = np.exp(-d * d / (2.0 * sg * sg)) if sg > 0 else np.zeros(N)
        ax.append(np.where(d > 0, out, 1.0))
    return ax[2][:, None, None] * ax[1][None, :, None] * ax[0][None, None, :]


def transform(vol, cfg=None):
    """Half-space centred transform of a sub-volume: (v - mean) / sigma (population statistics over N^3, sigma = 1 when the variance
    is not positive), times the window of `cfg` (alignment; None = the whole box, as the average takes it), fftn, (-1)^(kx+ky+kz)."""
    v = np.asarray(vol, dtype=np.float64)
    N = v.shape[0]
    mu = v.mean()
    var = (v * v).mean() - mu * mu
    sd = math.sqrt(var) if var > 0 else 1.0
    v = (v - mu) / sd
    if cfg is not None:
        v = v * window(N, cfg)
    return _rfftn_centred(v)


def reference_cube(vol):
    """Transform of the reference as orc_reference_create samples it (pad 1): the volume divided by sinc^2 along each axis (the
    envelope of trilinear interpolation), fftn, 1 / N, (-1)^(kx+ky+kz)."""
    v = np.asarray(vol, dtype=np.float64)
    N = v.shape[0]
    u = np.pi * (np.arange(N) - N // 2) / N
    s = np.where(np.abs(u) < 1e-12, 1.0, np.sin(u) / np.where(u == 0, 1.0, u))
    g = 1.0 / (s * s)
    return _rfftn_centred(v * (g[:, None, None] / N) * g[None, :, None] * g[None, None, :])


def sample(T, X, Y, Z, f32=False):
    """Trilinear sample of a half-space transform at real positions; a point with X < 0 is the conjugate of the sample at -(X, Y, Z)
    (the same interpolant as taking the Friedel mate conj T(-x, -y, -z) tap by tap).  f32: the fractions and tap weights are formed
    in float32 (X, Y, Z then are float32 already).  The element-wise work runs through torch in float64 / complex128 (threads)."""
    import torch
    N, NX = T.shape[0], T.shape[2]
    flat = torch.from_numpy(np.ascontiguousarray(T).reshape(-1))
    X, Y, Z = (torch.from_numpy(np.ascontiguousarray(a)) for a in (X, Y, Z))
    neg = X < 0
    sg = torch.where(neg, -1.0, 1.0).to(X.dtype)
    X, Y, Z = X * sg, Y * sg, Z * sg
    x0, y0, z0 = torch.floor(X), torch.floor(Y), torch.floor(Z)
    fr = [(X - x0, x0.long()), (Y - y0, y0.long()), (Z - z0, z0.long())]
    wt = [[(1.0 - f).double(), f.double()] if not f32 else [(1.0 - f), f] for f, _ in fr]
    ix = [fr[0][1], fr[0][1] + 1]
    iy = [torch.remainder(fr[1][1] + d, N) * NX for d in (0, 1)]
    iz = [torch.remainder(fr[2][1] + d, N) * (N * NX) for d in (0, 1)]
    out = torch.zeros(X.shape, dtype=torch.complex128)
    for dz in (0, 1):
        for dy in (0, 1):
            zy = iz[dz] + iy[dy]
            wzy = wt[2][dz] * wt[1][dy]
            for dx in (0, 1):
                w = wt[0][dx] * wzy if not f32 else (wt[0][dx] * wt[1][dy] * wt[2][dz])
                out += w.double() * flat[zy + ix[dx]].to(torch.complex128)
    return torch.where(neg, out.conj(), out).resolve_conj().numpy()


# ------------------------------------------------------------------------------------------------ the average
def inband_mask(N):
    """Voxels [N][N][N/2+1] an average fills: 0 < |q|^2 < (N/2 - 1)^2, on qx = 0 only the canonical half (qy > 0, or qy = 0 and qz > 0)."""
    d = (np.arange(N) - N // 2).astype(np.int64)
    x = np.arange(N // 2 + 1, dtype=np.int64)
    q2 = (d * d)[:, None, None] + (d * d)[None, :, None] + (x * x)[None, None, :]
    m = (q2 > 0) & (q2 < (N // 2 - 1) ** 2)
    m[:, :, 0] &= (d[None, :] > 0) | ((d[None, :] == 0) & (d[:, None] > 0))
    return m


def inband_voxels(N):
    """Flat indices (qz + N/2, qy + N/2, qx) of inband_mask."""
    return np.flatnonzero(inband_mask(N))


def voxel_sample(N, n, seed):
    """A seeded sample of n in-band voxels plus every in-band voxel of the planes qx = 0 and qx = 1 (sorted flat indices)."""
    vox = inband_voxels(N)
    pick = np.random.default_rng(seed).choice(len(vox), size=min(n, len(vox)), replace=False)
    planes = vox[vox % (N // 2 + 1) <= 1]
    return np.union1d(vox[pick], planes)


def _q_of(N, vox):
    NX = N // 2 + 1
    return (vox % NX).astype(np.float64), ((vox // NX) % N - N // 2).astype(np.float64), (vox // (NX * N) - N // 2).astype(np.float64)


def _positions(q, S, Nm, f32):
    """k = N^T S^T q.  f32: operands and every product and sum rounded to float32, S^T q first and N^T of that after (a model of
    float32 arithmetic, left to right); float64: one product with the matrix N^T S^T."""
    S, Nm = np.asarray(S, dtype=np.float64), np.asarray(Nm, dtype=np.float64)
    if not f32:
        M = Nm.T @ S.T
        return [M[i, 0] * q[0] + M[i, 1] * q[1] + M[i, 2] * q[2] for i in range(3)]
    S, Nm = S.astype(np.float32), Nm.astype(np.float32)
    qx, qy, qz = (a.astype(np.float32) for a in q)
    g = [S[0, i] * qx + S[1, i] * qy + S[2, i] * qz for i in range(3)]
    return [Nm[0, i] * g[0] + Nm[1, i] * g[1] + Nm[2, i] * g[2] for i in range(3)]


def _tilt(kx, kz):
    """Tilt angle of (kx, kz) in degrees, folded into (-90, 90] (float64, through torch for its threads)."""
    import torch
    a = torch.rad2deg(torch.atan2(torch.from_numpy(np.ascontiguousarray(kz, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(kx, dtype=np.float64))))
    a = torch.where(a > 90.0, a - 180.0, a)
    return torch.where(a <= -90.0, a + 180.0, a).numpy()


def _phase(rev):
    """exp(2 pi i rev), complex128."""
    import torch
    r = torch.from_numpy(np.ascontiguousarray(rev, dtype=np.float64))
    return torch.polar(torch.ones_like(r), 2.0 * math.pi * r).numpy()


def _voxels(N, voxels):
    """(the voxels a call works on: `voxels`, or every in-band voxel; the number of in-band voxels of the box)."""
    allv = inband_voxels(N)
    return (allv if voxels is None else np.asarray(voxels, dtype=np.int64)), len(allv)


def near_wedge(N, wedges, poses, sym_ops=None, voxels=None, margin=MARGIN):
    """(mask over `voxels` - default: every in-band voxel - that is True where, for any sub-volume and operator, the rotated sample
    k = N^T S^T q lies within `margin` pixels of a wedge-limit plane; the voxels; the number of in-band voxels of the box)."""
    vox, n_inband = _voxels(N, voxels)
    ops = R.symmetry_ops("C1") if sym_ops is None else np.asarray(sym_ops, dtype=np.float64).reshape(-1, 3, 3)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    near = np.zeros(len(vox), dtype=bool)
    geoms = {(tuple(p[:9]), float(w[0]), float(w[1])) for p, w in zip(poses, np.asarray(wedges, dtype=np.float64))}     # shifts do not matter
    for c0 in range(0, len(vox), CHUNK):
        q = _q_of(N, vox[c0:c0 + CHUNK])
        for S in ops:
            for Nm, lw, uw in geoms:
                kx, _, kz = _positions(q, S, np.array(Nm).reshape(3, 3), False)
                for a in (lw, uw):
                    near[c0:c0 + CHUNK] |= np.abs(kz * math.cos(math.radians(a)) - kx * math.sin(math.radians(a))) < margin
    return near, vox, n_inband


def insert(N, vols, wedges, poses, index=None, sym_ops=None, use_wedge=True, voxels=None, margin=MARGIN, f32=False, transforms=None):
    """ppm_sva_insert in float64.  For every in-band voxel q (inband_mask), every operator S in order and every sub-volume in order:
    k = N^T S^T q; wedge test on atan2(kz, kx) folded into (-90, 90], limits inclusive; trilinear sample of the sub-volume's
    transform; times exp(-2 pi i k.p / N) / N; weight + 1; half = parity of index[v] (of v when index is None).

    Returns (acc, counts, near, n_inband).  voxels=None: acc is the whole accumulator [2][N][N][N/2+1][3] and near a mask [N][N][N/2+1];
    voxels = flat in-band indices: acc is [2][len(voxels)][3] and near a mask over them (the large boxes).  near: near_wedge.
    transforms: the sub-volumes' transforms if the caller has them (vols is not read then).  f32: positions, matrix products, tap
    weights and the shift phase (in revolutions) are rounded to float32 and the transforms stored as complex64 - a model of float32
    rounding, not a copy of any kernel; the wedge test is made on those positions."""
    NX = N // 2 + 1
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    nv = len(poses)
    wedges = np.asarray(wedges, dtype=np.float32).reshape(nv, 2).astype(np.float64)
    ops = R.symmetry_ops("C1") if sym_ops is None else np.asarray(sym_ops, dtype=np.float64).reshape(-1, 3, 3)
    vox, n_inband = _voxels(N, voxels)
    near = near_wedge(N, wedges, poses, ops, vox, margin)[0] if use_wedge else np.zeros(len(vox), dtype=bool)
    out = np.zeros((2, len(vox), 3))
    counts = [0, 0]
    t = np.float32 if f32 else np.float64
    for v in range(nv):
        T = transform(vols[v]) if transforms is None else transforms[v]
        if f32:
            T = T.astype(np.complex64)
        h = int((index[v] if index is not None else v) % 2)
        counts[h] += 1
        Nm, p = poses[v, :9].reshape(3, 3), poses[v, 9:].astype(t)
        for S in ops:
            for c0 in range(0, len(vox), CHUNK):
                kx, ky, kz = _positions(_q_of(N, vox[c0:c0 + CHUNK]), S, Nm, f32)
                sel = np.ones(len(kx), dtype=bool)
                if use_wedge:
                    a = _tilt(kx, kz)
                    sel = (a >= wedges[v, 0]) & (a <= wedges[v, 1])
                kx, ky, kz = kx[sel], ky[sel], kz[sel]
                val = sample(T, kx, ky, kz, f32)
                if f32:
                    rev = -(kx * p[0] + ky * p[1] + kz * p[2]) * (np.float32(1.0) / np.float32(N))
                    rev = (rev - np.floor(rev)).astype(np.float64)
                else:
                    rev = -(kx * p[0] + ky * p[1] + kz * p[2]) / N
                val = val * _phase(rev) / N
                idx = c0 + np.flatnonzero(sel)
                out[h, idx, 0] += val.real
                out[h, idx, 1] += val.imag
                out[h, idx, 2] += 1.0
    if voxels is not None:
        return out, counts, near, n_inband
    acc = np.zeros((2, N * N * NX, 3))
    acc[:, vox, :] = out
    nm = np.zeros(N * N * NX, dtype=bool)
    nm[vox] = near
    return acc.reshape(2, N, N, NX, 3), counts, nm.reshape(N, N, NX), n_inband


def without(acc, near):
    """A copy of an accumulator [2][N][N][N/2+1][3] (or [2][n][3]) with the voxels of `near` zeroed: compare_by_shell then skips them."""
    a = np.array(acc, copy=True)
    a[:, near, :] = 0
    return a


def compare_at(got, want, N, voxels):
    """f64_ref.compare_by_shell over a list of voxels: got, want [2][n][3] at the flat indices `voxels`.  The same measures - per
    channel the worst shell's relative L2 error, and the worst voxel's error against the RMS of its shell - with the shell sums and
    the RMS taken over the listed voxels."""
    g = np.asarray(got, dtype=np.float64)
    w = np.asarray(want, dtype=np.float64)
    sh1 = R.shell_index(N).reshape(-1)[voxels].astype(np.int64)
    nb = int(sh1.max()) + 1
    sh = np.broadcast_to(sh1, g.shape[:2]).ravel()
    cnt = 2.0 * np.bincount(sh1, minlength=nb)
    den2 = {0: np.bincount(sh, weights=(w[..., 0] ** 2 + w[..., 1] ** 2).ravel(), minlength=nb),
            2: np.bincount(sh, weights=(w[..., 2] ** 2).ravel(), minlength=nb)}
    rep = R.ShellReport()
    NX = N // 2 + 1
    for c in range(3):
        d = (g[..., c] - w[..., c]).ravel()
        d2 = np.bincount(sh, weights=d * d, minlength=nb)
        den = den2[0 if c < 2 else 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(den > 0, np.sqrt(d2 / den), np.where(d2 > 0, np.inf, 0.0))
            rms = np.sqrt(den / np.maximum(cnt, 1.0))
            vx = np.where(rms[sh] > 0, np.abs(d) / rms[sh], np.where(d != 0, np.inf, 0.0))
        b = int(np.argmax(rel))
        rep.shell_rel[c] = (float(rel[b]), b)
        h, i = np.unravel_index(int(np.argmax(vx)), g.shape[:2])
        z, rest = divmod(int(voxels[i]), N * NX)
        y, x = divmod(rest, NX)
        rep.voxel_rel[c] = (float(vx.max()), (int(h), z - N // 2, y - N // 2, x))
    return rep


# ------------------------------------------------------------------------------------------------ the score
def band_weight(cfg, s):
    """Pass-band weight of a frequency s (cycles per pixel): Gaussian roll-offs outside [highpass, lowpass] (sva_band_weight)."""
    s = np.asarray(s, dtype=np.float64)
    w = np.ones_like(s)
    hc, hd, lc, ld = float(cfg.highpass_cutoff), float(cfg.highpass_decay), float(cfg.lowpass_cutoff), float(cfg.lowpass_decay)
    if hc > 0:
        d = hc - s
        w = np.where(s < hc, w * (np.exp(-d * d / (2.0 * hd * hd)) if hd > 0 else 0.0), w)
    if lc > 0:
        d = s - lc
        w = np.where(s > lc, w * (np.exp(-d * d / (2.0 * ld * ld)) if ld > 0 else 0.0), w)
    return w


def band_radius(cfg):
    """Largest Fourier radius (pixels) that still carries weight >= 1e-3 (sva_band_radius)."""
    N = cfg.box
    lc, ld = float(cfg.lowpass_cutoff), float(cfg.lowpass_decay)
    s = min(lc + (3.7169 * ld if ld > 0 else 0.0) if lc > 0 else 0.5, 0.5)
    return min(s * N, N // 2 - 1)


@functools.lru_cache(maxsize=1)
def _half_space(N, both_halves_of_kx0):
    """(kx, ky, kz, k^2), int32, of every sample with 0 < k^2 < (N/2 - 1)^2 in the half space kx >= 0, in the order kz, ky, kx; on
    kx = 0 the canonical half only unless both are asked for.  Kept for one box: every band of that box is a subset of it."""
    Rr = N // 2 - 1
    d = np.arange(-Rr, Rr + 1, dtype=np.int32)
    x = np.arange(0, Rr + 1, dtype=np.int32)
    k2 = (d * d)[:, None, None] + (d * d)[None, :, None] + (x * x)[None, None, :]
    m = (k2 > 0) & (k2 < Rr * Rr)
    if not both_halves_of_kx0:
        m[:, :, 0] &= (d[None, :] > 0) | ((d[None, :] == 0) & (d[:, None] > 0))
    iz, iy, ix = np.nonzero(m)
    return ix.astype(np.int32), (iy - Rr).astype(np.int32), (iz - Rr).astype(np.int32), k2[m]


def band_samples(cfg, both_halves_of_kx0=False):
    """The band's sample list, before the wedge: (kx, ky, kz, w) over the half space kx >= 0, on kx = 0 the canonical half (ky > 0, or
    ky = 0 and kz > 0), 0 < k^2 < rband^2, band weight >= 1e-3 (the weight as the float the C ABI stores)."""
    N = cfg.box
    rb = band_radius(cfg)
    kx, ky, kz, k2 = _half_space(N, bool(both_halves_of_kx0))
    keep = np.flatnonzero(k2 < rb * rb)
    w = band_weight(cfg, np.sqrt(k2[keep].astype(np.float64)) / N)
    keep = keep[w >= 1e-3]
    w = w[w >= 1e-3]
    return kx[keep].astype(np.int64), ky[keep].astype(np.int64), kz[keep].astype(np.int64), w.astype(np.float32).astype(np.float64)


def in_wedge(kx, kz, lw, uw):
    """sva_in_wedge on integer samples: the tilt angle of (kx, kz) folded into (-90, 90] within the inclusive limits; (0, ., 0) is
    always inside."""
    a = _tilt(kx, kz)
    return ((kx == 0) & (kz == 0)) | ((a >= float(np.float32(lw))) & (a <= float(np.float32(uw))))


def score(ref_T, cfg, T, wedge, pose, samples=None, f32=False):
    """The full-band score of one sub-volume at a given pose (orc_sva_align with tol_angle = tol_shift = 0):
    sum w Re(conj F(k) Ref(N k) e^{+2 pi i k.p / N}) / sqrt(sum w |Ref(N k)|^2 sum w |F(k)|^2) over the band's samples inside the
    wedge.  ref_T = reference_cube(reference), T = transform(sub-volume, cfg).  samples: a list from band_samples (default: cfg's).
    f32: the rotated positions, the tap weights and the shift phase in revolutions are rounded to float32, both transforms stored as
    complex64."""
    N = cfg.box
    kx, ky, kz, w = band_samples(cfg) if samples is None else samples
    if cfg.use_missing_wedge:
        keep = in_wedge(kx, kz, wedge[0], wedge[1])
        kx, ky, kz, w = kx[keep], ky[keep], kz[keep], w[keep]
    pose = np.asarray(pose, dtype=np.float64)
    t = np.float32 if f32 else np.float64
    Nm, p = pose[:9].reshape(3, 3).astype(t), pose[9:].astype(t)
    A = B = C = 0.0
    for c0 in range(0, len(kx), CHUNK):
        s = slice(c0, c0 + CHUNK)
        fx, fy, fz = kx[s].astype(t), ky[s].astype(t), kz[s].astype(t)
        X, Y, Z = (Nm[i, 0] * fx + Nm[i, 1] * fy + Nm[i, 2] * fz for i in range(3))
        F = T[kz[s] % N, ky[s] % N, kx[s]]
        if f32:
            F = F.astype(np.complex64).astype(np.complex128)
            rev = (fx * p[0] + fy * p[1] + fz * p[2]) * (np.float32(1.0) / np.float32(N))
            rev = (rev - np.floor(rev)).astype(np.float64)
            M = sample(ref_T.astype(np.complex64) if ref_T.dtype != np.complex64 else ref_T, X, Y, Z, True)
        else:
            rev = (fx * p[0] + fy * p[1] + fz * p[2]) / N
            M = sample(ref_T, X, Y, Z)
        M = M * _phase(rev)
        A += float((w[s] * (np.conj(F) * M).real).sum())
        B += float((w[s] * np.abs(M) ** 2).sum())
        C += float((w[s] * np.abs(F) ** 2).sum())
    return A / math.sqrt(B * C) if B > 0 and C > 0 else 0.0


# ------------------------------------------------------------------------------------------------ bounds
def floor_model_sva(N, p_max, offset_sigmas=0.0):
    """Expected float32 floor of the sub-tomogram path at box N, for shifts of up to p_max pixels and a density offset of
    offset_sigmas standard deviations: eps32 x (three line transforms, 3 log2 N; positions rounded at |k| <= N/2; the shift phase
    kept in float32 revolutions, 2 pi (N/2) sqrt(3) p_max / N; the raw-volume transform of the two-step path, whose round-off scales
    with mean / sigma, offset_sigmas x 3 log2 N) plus the 1e-6 of the hardware sine.  The bounds are f64_ref.SHELL_K, VOXEL_K and
    MAP_K times this."""
    lg = 3.0 * math.log2(N)
    return EPS32 * (lg + N / 2 + 2.0 * math.pi * (N / 2) * math.sqrt(3.0) * p_max / N + offset_sigmas * lg) + 1e-6


# ------------------------------------------------------------------------------------------------ seeded inputs
def blob_reference(N, seed):
    """A dozen separable Gaussian blobs inside 0.3 N of the box centre, drawn in numpy (no projector), unit variance."""
    rng = np.random.default_rng(seed)
    d = np.arange(N) - N // 2
    gz, gyx = [], []
    for _ in range(12):
        c = rng.uniform(-1, 1, 3)
        c = c / max(1.0, np.linalg.norm(c)) * 0.3 * N * rng.uniform(0.2, 1.0)
        s = rng.uniform(0.03, 0.07) * N
        g = [np.exp(-(d - c[i]) ** 2 / (2 * s * s)) for i in range(3)]
        gz.append(rng.uniform(0.5, 1.5) * g[2])
        gyx.append((g[1][:, None] * g[0][None, :]).ravel())
    v = (np.array(gz).T @ np.array(gyx)).reshape(N, N, N)        # sum over the blobs of gz x gy x gx
    return ((v - v.mean()) / v.std()).astype(np.float32)


GEOMS = 4          # distinct (rotation, wedge) pairs of a case: two kinds of pose x two wedges, whatever the number of sub-volumes


def case_poses(N, nv, seed):
    """Poses, wedges, the integer content shifts d and the half-map indices of a case's nv sub-volumes.  Sub-volume v has geometry
    v mod 4: even = a rotation of a few degrees with p = -d + a fraction of a pixel, odd = a random rotation (the first such that the
    qz axis of the average falls inside its wedge);
    geometries 0, 1 have the wedge (-54, 60), 2 and 3 (-40, 47).  Shifts of up to +-3 px; index = 3 v + 1.  Sub-volumes beyond the
    fourth reuse the four rotations (the wedge-limit planes, and so the excluded voxels, stay those of four) with shifts of their own."""
    rng = np.random.default_rng(seed)
    rots = []
    for g in range(GEOMS):
        if g % 2 == 0:
            rots.append(R.euler(*rng.uniform(-3, 3, 3)))
        else:
            while True:          # geometry 1: drawn again until N^T z lies inside its wedge, so that the qx = 0, qy = 0 line of the average is filled
                M = R.euler(rng.uniform(0, 360), math.degrees(math.acos(rng.uniform(-1, 1))), rng.uniform(0, 360))
                a = math.degrees(math.atan2(M[2, 2], M[2, 0]))
                a = a - 180.0 if a > 90.0 else (a + 180.0 if a <= -90.0 else a)
                if g != 1 or WEDGES[0][0] + 5.0 < a < WEDGES[0][1] - 5.0:
                    break
            rots.append(M)
    poses = np.zeros((nv, 12))
    shifts = rng.integers(-2, 3, size=(nv, 3))
    for v in range(nv):
        poses[v, :9] = rots[v % GEOMS].ravel()
        poses[v, 9:] = -shifts[v] + rng.uniform(-0.5, 0.5, 3)
    wedges = np.array([WEDGES[(v % GEOMS) // 2] for v in range(nv)], dtype=np.float32)
    return poses, wedges, shifts, np.arange(nv) * 3 + 1


def case_volumes(N, shifts, seed, offset):
    """(reference, sub-volumes): sub-volume v = (the reference rolled by the integer shift d_v (x, y, z) + unit white noise) x 7 +
    280 x offset[v], float32."""
    ref = blob_reference(N, seed)
    rng = np.random.default_rng(seed + 1)
    vols = np.empty((len(shifts), N, N, N), dtype=np.float32)
    for v, d in enumerate(shifts):
        x = np.roll(ref, (int(d[2]), int(d[1]), int(d[0])), axis=(0, 1, 2)) + rng.standard_normal((N, N, N), dtype=np.float32)
        vols[v] = x * np.float32(7.0) + np.float32(280.0 * offset[v])
    return ref, vols


P_MAX = 3.0                    # |p| per axis stays below 2 + 0.5
OFFSET_SIGMAS = 40.0

# Boxes of the GPU file by launch plan: two-step transforms with L16 = 16 (32, 48, 112: M = 2, 3, 7; 192: the fft16m<12> / <-12> special
# case; 256: nl M = 256) and L16 = 8 (288: the first such box; 512: M = 32, window and twiddle tables full); staged transforms with
# L = 16, 14, 10, 12 (40, 42, 50, 54), above 256 (270: L = 15) and at k_sva_xpass's largest LDS request (490: L = 14)
TWO_STEP = (32, 48, 112, 192, 256, 288, 512)
STAGED = (40, 42, 50, 54, 270, 490)
GPU_BOXES = tuple(sorted(TWO_STEP + STAGED))
SAMPLED = (490, 512)           # average compared on a voxel sample, 2 sub-volumes
N_SAMPLE = 200000
# (box, symmetry, sub-volumes, PPM_SVA_GENERIC_FFT) of the further average cases
MORE_AVERAGES = ((48, "C3", 4, False), (42, "D2", 4, False), (32, "C1", 35, False), (48, "C1", 4, True), (288, "C1", 4, True))


def xpass_lines(N):
    """Lines per block of k_sva_xpass (host_sva.h): min(16, 7000 / N) lowered until it divides N^2."""
    L = max(1, min(16, 7000 // N))
    while (N * N) % L:
        L -= 1
    return L


def gpu_case(N, nv=None, with_volumes=True):
    """The input set of box N in tests/test_gpu_sva_f64.py: 4 sub-volumes (2 at 490 and 512), the last with the density offset."""
    nv = (2 if N in SAMPLED else 4) if nv is None else nv
    poses, wedges, shifts, index = case_poses(N, nv, 7000 + N)
    offset = np.zeros(nv)
    offset[-1] = 1.0
    out = dict(N=N, nv=nv, poses=poses, wedges=wedges, index=index, offset=offset)
    if with_volumes:
        out["ref"], out["vols"] = case_volumes(N, shifts, 9000 + N, offset)
    return out


def score_settings(N):
    """The three alignment settings of the score tests, tol_angle = tol_shift = 0: the default band; a window (12, 12, 10) with sigma
    2, high-pass (0.03, 0.01), low-pass (0.30, 0.04); no wedge with low-pass (0.45, 0.05)."""
    from pyp_amd.abi import SvaCfg
    z = dict(tol_angle=0.0, tol_shift=0.0)
    return [SvaCfg.make(N, **z),
            SvaCfg.make(N, window=(12, 12, 10), window_sigma=2.0, highpass=(0.03, 0.01), lowpass=(0.30, 0.04), **z),
            SvaCfg.make(N, use_missing_wedge=0, lowpass=(0.45, 0.05), **z)]
