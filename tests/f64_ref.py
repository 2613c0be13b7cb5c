"""(Test infrastructure: a float64 restatement of the insertion and finalisation path; nothing in pyp_amd imports it.)

The same operations as oracle/ppm_oracle.c (preprocess_row, ctf_eval, orc_insert_batch, orc_finalize) and the conventions of
include/ppm.h, written again in plain numpy with every intermediate in float64.  The oracle keeps its FFTs and accumulators in
float32; this module does not, so it is the high-precision yardstick for both the oracle and the HIP kernels.

Layouts are those of the C ABI: an accumulator is [2][N][N][N/2+1][3] {re, im, weight} with kz, ky stored at index k + N/2; maps
are [z][y][x] with the origin at voxel (N/2, N/2, N/2); the statistics table has N/2 - 1 rows of PPM_STATS_COLS columns.
Config arguments are the ctypes structs of pyp_amd.abi (ReconCfg, FinalCfg) or anything with the same attribute names.
"""
import functools
import math

import numpy as np

from pyp_amd.formats import cistem

C = cistem.COL
EPS32 = float(np.finfo(np.float32).eps)


def supported_boxes():
    """Every even box from 32 to 512 whose only prime factors are 2, 3, 5 and 7 (box_ok, pyp_amd/csrc/ppm_geom.h)."""
    def smooth(n):
        for p in (2, 3, 5, 7):
            while n % p == 0:
                n //= p
        return n == 1
    return [n for n in range(32, 513, 2) if smooth(n)]


def _f32(x):
    """A config value as the library reads it: a C float widened to double."""
    return float(np.float32(x))


def band_geometry(N, px, res_limit):
    """r_hi and the band half-width B of an insertion (geom_init with res_high = res_limit, or 2 px when res_limit <= 0)."""
    a = _f32(px)
    rh = _f32(res_limit) if res_limit > 0 else 2.0 * a
    r_hi = min(N * a / rh, N / 2)
    return r_hi, int(math.ceil(r_hi)) - 1


def wavelength(kv):
    v = kv * 1000.0
    return 12.2639 / math.sqrt(v + 0.97845e-6 * v * v)


def ctf(row, N, px, kx, ky):
    """CTF of one row (DEFOCUS_1/2, DEFOCUS_ANGLE, PHASE_SHIFT, VOLTAGE, CS, AMPLITUDE_CONTRAST) at integer Fourier pixels kx, ky."""
    kx = np.asarray(kx, dtype=np.float64)
    ky = np.asarray(ky, dtype=np.float64)
    lam = wavelength(row[16])
    cs = row[17] * 1e7
    df1, df2, ast = row[6], row[7], math.radians(row[8])
    w = row[18]
    extra = row[9] + math.atan(w / math.sqrt(1.0 - w * w))
    k2 = kx * kx + ky * ky
    safe = np.where(k2 == 0, 1.0, k2)
    c2, s2a = (kx * kx - ky * ky) / safe, 2.0 * kx * ky / safe
    df = 0.5 * (df1 + df2 + (df1 - df2) * (c2 * math.cos(2 * ast) + s2a * math.sin(2 * ast)))
    s2 = k2 / (N * _f32(px)) ** 2
    chi = math.pi * lam * s2 * (df - 0.5 * cs * lam * lam * s2) + extra
    return np.where(k2 == 0, -math.sin(extra), -np.sin(chi))


def max_ctf_phase(row, N, px, r_max):
    """Largest |chi| (radians) over the band |k| < r_max: the float32 rounding of chi in a kernel is about |chi| * 6e-8."""
    lam = wavelength(row[16])
    cs = row[17] * 1e7
    s2 = (r_max / (N * _f32(px))) ** 2
    df = max(abs(row[6]), abs(row[7]))
    return math.pi * lam * s2 * (df + 0.5 * cs * lam * lam * s2) + abs(row[9]) + 0.1


def _band_index(B, r2):
    ky, kx = np.meshgrid(np.arange(-B, B + 1), np.arange(0, B + 1), indexing="ij")
    k2 = kx * kx + ky * ky
    keep = (k2 < r2) & (k2 != 0)
    return kx[keep], ky[keep], keep


def prep_band(img, row, N, px, rband, normalize, invert, mask_radius):
    """Pre-processed band [2B+1][B+1] complex128 (ky = -B..B, kx = 0..B; B = ceil(rband) - 1) of one particle as insertion uses
    it: background mean / sigma from the pixels farther than mask_radius (Angstrom) from the box centre (all pixels if fewer
    than 16), normalise / invert, FFT, centre phase (-1)^(kx+ky) / N, zero outside |k| < rband and at DC, and the beam-tilt
    phase exp(-i phi), phi = 2 pi Cs lambda^2 |s|^2 (s . b) removed.  No mask, no whitening; the CTF is applied in `insert`."""
    a = _f32(px)
    x = np.asarray(img, dtype=np.float64).reshape(N, N)
    Rm = _f32(mask_radius) / a
    d = np.arange(N) - N // 2
    r2 = d[None, :] ** 2 + d[:, None] ** 2
    bg = x[r2 > Rm * Rm]
    if bg.size < 16:
        bg = x.ravel()
    mu = bg.mean()
    var = (bg * bg).mean() - mu * mu
    sd = math.sqrt(var) if var > 0 else 1.0
    f = np.fft.fft2((x - mu) * ((1.0 / sd) if normalize else 1.0) * (-1.0 if invert else 1.0))
    B = int(math.ceil(rband)) - 1
    kx, ky, keep = _band_index(B, rband * rband)
    v = f[(ky + N) % N, kx]
    lam = wavelength(row[16])
    cc = 2.0 * math.pi * row[17] * 1e7 * lam * lam * 1e-3 / (N * a) ** 3
    btx, bty = cc * row[19], cc * row[20]
    if btx != 0 or bty != 0:
        v = v * np.exp(-1j * (kx * kx + ky * ky) * (kx * btx + ky * bty))
    v = v * np.where((kx + ky) & 1, -1.0, 1.0) / N
    out = np.zeros((2 * B + 1, B + 1), dtype=np.complex128)
    out[keep] = v
    return out


def euler(psi, theta, phi):
    """M = Rz(phi) Ry(theta) Rz(psi) (degrees)."""
    def rz(t):
        c, s = math.cos(math.radians(t)), math.sin(math.radians(t))
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])

    c, s = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    ry = np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])
    return rz(phi) @ ry @ rz(psi)


def symmetry_ops(sym):
    """Operators of Cn and Dn (n-fold axis z, two-fold axes in the xy plane starting at x), (k, 3, 3) float64."""
    t, n = sym[0].upper(), int(sym[1:] or 1)
    rots = []
    for j in range(n):
        c, s = math.cos(2 * math.pi * j / n), math.sin(2 * math.pi * j / n)
        rots.append(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]))
    if t == "C":
        return np.stack(rots)
    if t == "D":
        flip = np.diag([1.0, -1.0, -1.0])
        return np.stack(rots + [r @ flip for r in rots])
    raise ValueError(f"f64_ref: symmetry {sym} not restated")


def insert(N, px, sym_ops, imgs, rows, rc):
    """Fourier insertion of a stack: float64 accumulators [2][N][N][N/2+1][3] and the particle counts per half.

    Per row: skipped when OCCUPANCY <= 0 or SCORE < score_threshold; half = parity of PIND (split_by_pind) or POSITION;
    weight = OCC / 100 x exp(-B_s (score_average - SCORE) |s|^2 / 4) x the dose attenuation of its exposure; every in-band sample
    of prep_band x CTF x the shift phase exp(+2 pi i k.s / N) goes to X = S M (kx, ky, 0) (conjugated at -X when X < 0) by
    trilinear scatter, {w ctf I, w ctf^2}."""
    a = _f32(px)
    NX = N // 2 + 1
    acc = np.zeros((2, N, N, NX, 3), dtype=np.float64)
    flat = acc.reshape(2, -1, 3)
    counts = [0, 0]
    r_hi, B = band_geometry(N, a, rc.res_limit)
    kx, ky, _ = _band_index(B, r_hi * r_hi)
    k2 = (kx * kx + ky * ky).astype(np.float64)
    na2 = (N * a) ** 2
    dose = None
    if getattr(rc, "n_dose_weights", 0) > 0 and rc.dose_exponent > 0:
        dose = np.asarray(rc._dose, dtype=np.float64)
    ops = np.asarray(sym_ops, dtype=np.float64).reshape(-1, 3, 3)
    imgs = np.asarray(imgs)
    for ip, row in enumerate(np.asarray(rows, dtype=np.float64)):
        if not (row[C["OCCUPANCY"]] > 0) or row[C["SCORE"]] < _f32(rc.score_threshold):
            continue
        key = int(row[26] if rc.split_by_pind else row[0])
        h = key % 2
        counts[h] += 1
        band = prep_band(imgs[ip], row, N, a, r_hi, rc.normalize, rc.invert, rc.mask_radius)
        iv = band[ky + B, kx]
        cv = ctf(row, N, a, kx, ky)
        w = np.full(k2.shape, row[C["OCCUPANCY"]] / 100.0)
        if rc.score_weight_bfactor != 0:
            w = w * np.exp(-0.25 * _f32(rc.score_weight_bfactor) * (_f32(rc.score_average) - row[C["SCORE"]]) * k2 / na2)
        if dose is not None:
            t = int(row[27])
            dq = dose[t] if 0 <= t < len(dose) else 0.0
            tr = _f32(rc.dose_transition)
            tr = tr if 0 < tr <= 1 else 1.0
            cap2 = (tr * N / 2) ** 2
            if 0 < dq < 1:
                w = w * np.exp(_f32(rc.dose_exponent) * math.log(dq) * np.minimum(k2, cap2) / cap2)
        sx, sy = row[C["X_SHIFT"]] / a, row[C["Y_SHIFT"]] / a
        val = w * cv * iv * np.exp(2j * math.pi * (kx * sx + ky * sy) / N)
        vw = w * cv * cv
        M = euler(row[C["PSI"]], row[C["THETA"]], row[C["PHI"]])
        P0 = M[:, 0:1] * kx[None, :] + M[:, 1:2] * ky[None, :]
        for S in ops:
            X, Y, Z = S @ P0
            refl = X < 0
            X, Y, Z = np.where(refl, -X, X), np.where(refl, -Y, Y), np.where(refl, -Z, Z)
            u = np.where(refl, np.conj(val), val)
            x0, y0, z0 = np.floor(X), np.floor(Y), np.floor(Z)
            fx, fy, fz = X - x0, Y - y0, Z - z0
            x0, y0, z0 = x0.astype(np.int64), y0.astype(np.int64), z0.astype(np.int64)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        xi, yi, zi = x0 + dx, y0 + dy + N // 2, z0 + dz + N // 2
                        ok = (xi <= N // 2) & (yi >= 0) & (yi < N) & (zi >= 0) & (zi < N)
                        wt = ((fx if dx else 1 - fx) * (fy if dy else 1 - fy) * (fz if dz else 1 - fz))[ok]
                        idx = (zi[ok] * N + yi[ok]) * NX + xi[ok]
                        np.add.at(flat[h, :, 0], idx, wt * u.real[ok])
                        np.add.at(flat[h, :, 1], idx, wt * u.imag[ok])
                        np.add.at(flat[h, :, 2], idx, wt * vw[ok])
    return acc, counts


def shell_index(N):
    """Shell b = round(|k|) of every accumulator voxel [N][N][N/2+1] (kz, ky = index - N/2, kx = index), int16.  |k|^2 is an
    integer, so no |k| lies within 2.8e-4 of a half-integer below 3 x 256^2: float32 decides the rounding exactly."""
    return _shell_tables(N)[0]


@functools.lru_cache(maxsize=1)
def _shell_tables(N):
    """(shell index, voxels per shell, voxels per shell with kx > 0 counted twice); one box at a time is kept."""
    k = (np.arange(N, dtype=np.float32) - N // 2) ** 2
    x = np.arange(N // 2 + 1, dtype=np.float32) ** 2
    shell = np.floor(np.sqrt(k[:, None, None] + k[None, :, None] + x[None, None, :]) + np.float32(0.5)).astype(np.int16)
    cnt = np.bincount(shell.ravel())
    cnt0 = np.bincount(shell[:, :, 0].ravel(), minlength=len(cnt))
    return shell, cnt.astype(np.float64), 2.0 * cnt - cnt0


def _folded_plane(A):
    """kx = 0 plane holds both Friedel mates: (z, y) += conj (-z, -y) for z, y in -N/2+1 .. N/2-1 (orc_finalize)."""
    p = A[:, :, :, 0, :].copy()
    m = A[:, 1:, 1:, 0, :][:, ::-1, ::-1, :]
    p[:, 1:, 1:, 0] += m[..., 0]
    p[:, 1:, 1:, 1] -= m[..., 1]
    p[:, 1:, 1:, 2] += m[..., 2]
    return p


def finalize(acc, N, px, fc, maps=True):
    """merge3d: (half1, half2, filtered, stats) from float64 accumulators, like orc_finalize / ppm_finalize.

    kx = 0 fold; per shell b = round(|k|) < N/2: weight sums (kx > 0 counted twice), FSC of the Wiener-normalised halves
    n / (w + 1e-3 <w>_b), part-FSC with the particle volume fraction (810 Da / nm^3), part-SSNR, rec-SSNR = 2 FSC / (1 - FSC)
    (FSC clipped to 0 .. 0.999); maps = Re IFFT of (-1)^(x+y+z) n / (w + kappa_b), kappa_b = <w>_b / rec-SSNR_b, divided by the
    sinc^2 of trilinear interpolation and multiplied by the cosine-edged spherical mask.  The shell sums run over the voxels with
    weight (nothing else contributes); maps=False returns only the table."""
    a = _f32(px)
    ns = N // 2
    NX = ns + 1
    A = np.asarray(acc, dtype=np.float64).reshape(2, N, N, NX, 3)
    P = _folded_plane(A)
    shell, _, cnt2 = _shell_tables(N)
    scnt = cnt2[:ns]
    inb = shell < ns
    on = ((A[0, ..., 2] != 0) | (A[1, ..., 2] != 0)) & inb
    on[:, :, 0] = ((P[0, ..., 2] != 0) | (P[1, ..., 2] != 0)) & inb[:, :, 0]
    nz = np.flatnonzero(on)
    del on
    sh = shell.reshape(-1)[nz]
    x0 = nz % NX == 0
    Af = A.reshape(2, -1, 3)[:, nz, :]
    Af[:, x0, :] = P.reshape(2, -1, 3)[:, nz[x0] // NX, :]
    alv = np.where(x0, 1.0, 2.0)
    w1, w2 = Af[0, :, 2], Af[1, :, 2]
    n1 = Af[0, :, 0] + 1j * Af[0, :, 1]
    n2 = Af[1, :, 0] + 1j * Af[1, :, 1]
    sden1 = np.bincount(sh, weights=alv * w1, minlength=ns)
    sden2 = np.bincount(sh, weights=alv * w2, minlength=ns)
    sdt = np.bincount(sh, weights=alv * (w1 + w2), minlength=ns)
    e1 = (1e-3 * sden1 / scnt + 1e-20)[sh]
    e2 = (1e-3 * sden2 / scnt + 1e-20)[sh]
    u, v = n1 / (w1 + e1), n2 / (w2 + e2)
    c12 = np.bincount(sh, weights=alv * (u * np.conj(v)).real, minlength=ns)
    c11 = np.bincount(sh, weights=alv * np.abs(u) ** 2, minlength=ns)
    c22 = np.bincount(sh, weights=alv * np.abs(v) ** 2, minlength=ns)
    mm = _f32(fc.molecular_mass_kda)
    vfrac = (mm * 1000.0 / 0.81) / (N * a) ** 3 if mm > 0 else 1.0
    vfrac = min(1.0, max(1e-6, vfrac))
    stats = np.zeros((ns - 1, 7))
    kap = np.zeros(ns)
    for b in range(ns):
        fsc = c12[b] / math.sqrt(c11[b] * c22[b]) if c11[b] > 0 and c22[b] > 0 else 0.0
        fcl = min(max(fsc, 0.0), 0.999)
        rec = 2.0 * fcl / (1.0 - fcl)
        md = sdt[b] / scnt[b] if scnt[b] > 0 else 0.0
        kap[b] = 1e-20 if b == 0 else md / max(rec, 1e-6)
        if b >= 1:
            stats[b - 1] = (b, N * a / b, b / (N * a), fsc, fcl / (fcl + vfrac * (1 - fcl)), rec / md / vfrac if md > 0 else 0.0, rec)
    if not maps:
        return None, None, None, stats
    import torch
    d = np.arange(N) - ns
    par = (d[:, None, None] + d[None, :, None] + np.arange(NX)[None, None, :]) & 1
    sg = np.where(par, -1.0, 1.0)
    kapv = np.where(inb, kap[np.minimum(shell, ns - 1)], np.inf)
    t = d / N
    sc = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1.0, np.pi * t)) ** 2
    g3 = sc[:, None, None] * sc[None, :, None] * sc[None, None, :]
    rho = np.sqrt(d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2)
    rout, rin = _f32(fc.outer_radius) / a, _f32(fc.inner_radius) / a
    fo = (_f32(fc.mask_falloff) if fc.mask_falloff > 0 else 10.0) / a
    mask = np.ones_like(rho)
    if rout > 0:
        mask = np.where(rho >= rout + 0.5 * fo, 0.0,
                        np.where(rho > rout - 0.5 * fo, 0.5 * (1 + np.cos(np.pi * (rho - rout + 0.5 * fo) / fo)), 1.0))
    if rin > 0:
        mask = np.where(rho < rin, 0.0, mask)
    post = mask / g3
    del rho, mask, g3
    outs = []
    for which in range(3):
        src = (A[which], P[which]) if which < 2 else (A[0] + A[1], P[0] + P[1])
        num = src[0][..., 0] + 1j * src[0][..., 1]
        den = src[0][..., 2].copy()
        num[:, :, 0] = src[1][..., 0] + 1j * src[1][..., 1]
        den[:, :, 0] = src[1][..., 2]
        spec = np.fft.ifftshift(sg * num / (den + kapv), axes=(0, 1))
        vol = torch.fft.irfftn(torch.from_numpy(spec), s=(N, N, N)).numpy() * N
        outs.append(vol * post)
    return outs[0], outs[1], outs[2], stats


class ShellReport:
    """Result of compare_by_shell: per channel, the worst shell's relative L2 error and the worst voxel's error relative to the
    RMS of its shell, with where they are."""

    NAMES = ("re", "im", "weight")

    def __init__(self):
        self.shell_rel = {}     # channel -> (rel, shell)
        self.voxel_rel = {}     # channel -> (rel, (half, kz, ky, kx))

    @property
    def max_shell_rel(self):
        return max(v[0] for v in self.shell_rel.values())

    @property
    def max_voxel_rel(self):
        return max(v[0] for v in self.voxel_rel.values())

    def worst(self):
        c = max(self.shell_rel, key=lambda k: self.shell_rel[k][0])
        return c, self.shell_rel[c][1]

    def ok(self, shell_bound, voxel_bound):
        return self.max_shell_rel <= shell_bound and self.max_voxel_rel <= voxel_bound

    def __str__(self):
        parts = []
        for c in sorted(self.shell_rel):
            r, b = self.shell_rel[c]
            v, where = self.voxel_rel[c]
            parts.append(f"{self.NAMES[c]}: worst shell {b} rel {r:.3g}, worst voxel half/kz/ky/kx {where} at {v:.3g} x shell RMS")
        return "; ".join(parts)


def compare_by_shell(got, want, N):
    """Compare two accumulators [2][N][N][N/2+1][3] shell by shell.  For each channel and shell b = round(|k|): the relative L2
    error ||got - want|| / ||want|| over the shell's voxels of both halves; for each voxel: |got - want| / RMS(want over its
    shell).  Voxels are visited where either side has weight (a sample that lands anywhere leaves weight there; values outside
    that support are checked by `stray_values`).  The real and imaginary channels are measured against the shell's complex magnitude |re + i im| (a float32 error of
    either part scales with it, and a shell whose imaginary part cancels, like the origin under D2, is not a 0 / 0).  The corner
    shells b >= N/2, which no finalisation reads, hold only the tails of trilinear taps (weights fx fy fz of samples at |k| < N/2):
    a position rounded to float32 (eps N/2 pixels) changes a tail of weight f by eps N / (2 f) relative, without bound as f -> 0,
    so they are measured against the RMS of shell N/2 - 1, the last one used, instead of their own.  A shell where `want` is all
    zero and `got` is not counts as an infinite error."""
    NX = N // 2 + 1
    g = np.asarray(got).reshape(2, -1, 3)
    w = np.asarray(want).reshape(2, -1, 3)
    shell, cnt, _ = _shell_tables(N)
    shell = shell.reshape(-1)
    nb = len(cnt)
    cnt = 2.0 * cnt
    nz = np.flatnonzero((g[0, :, 2] != 0) | (g[1, :, 2] != 0) | (w[0, :, 2] != 0) | (w[1, :, 2] != 0))
    gv = g[:, nz, :].astype(np.float64)
    wv = w[:, nz, :].astype(np.float64)
    sh = np.broadcast_to(shell[nz], gv.shape[:2]).ravel()
    scale = {0: (wv[..., 0] ** 2 + wv[..., 1] ** 2).ravel(), 2: (wv[..., 2] ** 2).ravel()}
    w2 = {c: np.bincount(sh, weights=v, minlength=nb) for c, v in scale.items()}
    ns = N // 2
    if nb > ns:
        for c in w2:                     # corner shells b >= N/2: the scale of shell N/2 - 1
            w2[c][ns:] = w2[c][ns - 1] / cnt[ns - 1] * cnt[ns:]
    rep = ShellReport()
    for c in range(3):
        d = (gv[..., c] - wv[..., c]).ravel()
        d2 = np.bincount(sh, weights=d * d, minlength=nb)
        den = w2[0 if c < 2 else 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(den > 0, np.sqrt(d2 / den), np.where(d2 > 0, np.inf, 0.0))
            rms = np.sqrt(den / cnt)
            vox = np.where(rms[sh] > 0, np.abs(d) / rms[sh], np.where(d != 0, np.inf, 0.0))
        b = int(np.argmax(rel))
        rep.shell_rel[c] = (float(rel[b]), b)
        if vox.size:
            h, i = np.unravel_index(int(np.argmax(vox)), gv.shape[:2])
            z, rest = divmod(int(nz[i]), N * NX)
            y, x = divmod(rest, NX)
            rep.voxel_rel[c] = (float(vox[h * len(nz) + i]), (int(h), z - N // 2, y - N // 2, x))
        else:
            rep.voxel_rel[c] = (0.0, None)
    return rep


def stray_values(got, want):
    """Voxels where `got` carries anything but `want` has no weight: writes that landed where no sample reaches (compare_by_shell
    visits them too, this names their number).  The weight channel alone is no guide on `got`: a kernel that sums in fixed
    point may round a tiny weight w ctf^2 to zero next to its non-zero value w ctf I."""
    g = np.asarray(got).reshape(2, -1, 3)
    w = np.asarray(want).reshape(2, -1, 3)
    return int(np.count_nonzero((g != 0).any(axis=2) & (w[..., 2] == 0)))


def rel_l2(got, want):
    """The old whole-volume yardstick: ||got - want|| / ||want||."""
    g = np.asarray(got, dtype=np.float64)
    w = np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


def seeded_particles(N, m, seed, px=None):
    """m seeded particles of box N (px = 256 / N keeps the physical box at 256 A): white noise plus one smooth Gaussian blob
    drawn in numpy (no volume, no projector), random poses, shifts of up to +-6 px, astigmatic defoci 8000 .. 24000 A,
    SCORE 10 .. 30, PIND = 0 .. m-1 and POSITION = 1 .. m.  Returns (px, images (m, N, N) float32, rows (m, 32))."""
    rng = np.random.default_rng(seed)
    px = 256.0 / N if px is None else px
    rows = cistem.default_rows(m, px, 300.0, 2.7, 0.07)
    rows[:, C["PSI"]] = rng.uniform(0, 360, m)
    rows[:, C["PHI"]] = rng.uniform(0, 360, m)
    rows[:, C["THETA"]] = np.degrees(np.arccos(rng.uniform(-1, 1, m)))
    rows[:, C["X_SHIFT"]:C["Y_SHIFT"] + 1] = rng.uniform(-6, 6, (m, 2)) * px
    rows[:, C["DEFOCUS_1"]] = rng.uniform(8000, 24000, m)
    rows[:, C["DEFOCUS_2"]] = rows[:, C["DEFOCUS_1"]] - rng.uniform(200, 900, m)
    rows[:, C["DEFOCUS_ANGLE"]] = rng.uniform(0, 180, m)
    rows[:, C["PIND"]] = np.arange(m)
    rows[:, C["POSITION_IN_STACK"]] = np.arange(1, m + 1)
    rows[:, C["SCORE"]] = rng.uniform(10, 30, m)
    d = np.arange(N) - N // 2
    imgs = rng.normal(0, 1, (m, N, N)).astype(np.float32)
    for i in range(m):
        cx, cy = rng.uniform(-N / 8, N / 8, 2)
        blob = 3.0 * np.exp(-((d[None, :] - cx) ** 2 + (d[:, None] - cy) ** 2) / (2 * (N / 10) ** 2))
        imgs[i] += blob.astype(np.float32)
    return px, imgs, rows


# ------------------------------------------------------------------------------------------- bounds of the box sweep
# bound = K x floor_model(N) (tests/test_gpu_box_sweep.py; measured floors in CHANGELOG.md): worst shell 0.2 .. 0.8 x the model, worst
# voxel 14 .. 112 x, FSC up to 100 x (at 490).  FSC is taken over n / (w + 1e-3 <w>_b): near a CTF zero the Wiener floor caps the
# amplification of a CTF-phase error at 1 / sqrt(1e-3) = 32, so its bound is 4 x that; the SSNR columns get the FSC bound carried
# through 1 / (1 - FSC) shell by shell (ssnr_tolerance)
SHELL_K, VOXEL_K, FSC_K, MAP_K = 3.0, 300.0, 4.0 / math.sqrt(1e-3), 8.0


def floor_model(N, rows):
    """Expected float32 floor of an insertion at box N with px = 256 / N: position and FFT round-off (eps32 (log2 N + N/2)) plus
    the CTF phase error eps32 |chi| of the worst row, plus the 1e-6 of the hardware sine."""
    chi = max(max_ctf_phase(r, N, 256.0 / N, N / 2) for r in rows)
    return EPS32 * (math.log2(N) + N / 2 + chi) + 1e-6


def leg_a_rows(N):
    """6 particles: halves by PIND (0, 2, 4 -> half 0; 1, 3 -> half 1; PIND 5 rejected), a beam-tilted row, an occupancy of 60,
    the score B-factor weight on; ReconCfg at the full band."""
    from pyp_amd.abi import ReconCfg
    px, imgs, rows = seeded_particles(N, 6, 1000 + N)
    rows[1, C["BEAM_TILT_X"]], rows[1, C["BEAM_TILT_Y"]] = 1.2, -0.8
    rows[2, C["OCCUPANCY"]] = 60.0
    rows[5, C["OCCUPANCY"]] = 0.0
    rc = ReconCfg(box=N, pixel_size=px, res_limit=2 * px, score_weight_bfactor=2.0, score_average=20.0, score_threshold=0.0,
                  normalize=1, invert=0, split_by_pind=1, mask_radius=0.4 * N * px)
    return px, imgs, rows, rc


def ssnr_tolerance(stats, fsc_tol, rel_tol):
    """Per-shell tolerances of rec-SSNR and part-SSNR (columns 6 and 5) when FSC may be off by fsc_tol and the shell weight sums
    by rel_tol: rec = 2 f / (1 - f) moves by 2 fsc_tol / (1 - f)^2 (f clipped to 0.999, taken at the upper end of its
    interval); part-SSNR = rec / (<w> vfrac) moves by that over <w> vfrac = rec / part-SSNR (interpolated over the shells where
    rec = 0) plus rel_tol of itself."""
    f = np.clip(stats[:, 3], 0.0, 0.999)
    fhi = np.minimum(f + fsc_tol, 0.999)
    drec = 2.0 * fsc_tol / (1.0 - fhi) ** 2
    rec, part = stats[:, 6], stats[:, 5]
    ok = rec > 0
    ratio = np.interp(np.arange(len(rec)), np.flatnonzero(ok), part[ok] / rec[ok]) if ok.any() else np.ones_like(rec)
    return drec + rel_tol * np.abs(rec), drec * ratio + rel_tol * np.abs(part)


# ------------------------------------------------------------------------------------------- k_prep launch plan
SEARCH_ABOVE_256 = (270, 294, 384, 486, 490, 500, 512)   # search-path boxes above 256 of the box sweep: L = 5, 3, 4, 3, 1, 2, 2 below


def prep_plan(N, B):
    """The column-chunk plan launch_prep (pyp_amd/csrc/host_refine.h) launches with for box N and band half-width B on its default
    path (256 threads, 40 KB of LDS): row pairs L (divides N/2), chunk width nc, chunk count and the last chunk's width.
    lds_fixed = 16 (B + 2) + 16 + 5 x 4 x 8 + (12 + 4) x 4 + 12 N + 16 bytes; L = min(2048 / N, N / 2), lowered until it
    divides N/2 and L N 8 + lds_fixed + 8 (N + 1) <= 20 KB + 8 KB; nc = min(W, (40 KB - lds_fixed - L N 8) / (8 (N + 1)),
    3072 / N); chunks = ceil(W / nc), then nc = ceil(W / chunks) (even chunks), W = B + 1.  Last: the LDS bytes of the launch,
    8 (nc (N + 1) + L N) + lds_fixed.  tests/test_prep_plan_cpu.py holds this restatement to prep_plan of pyp_amd/csrc/ppm_geom.h."""
    lds_fixed = (B + 2) * 16 + 16 + 5 * 4 * 8 + (12 + 4) * 4 + N * 12 + 16
    W = B + 1
    L = max(1, min(2048 // N, N // 2))
    while (N // 2) % L or L * N * 8 + lds_fixed + (N + 1) * 8 > 20 * 1024 + 8192:
        L -= 1
    left = max(0, 40 * 1024 - lds_fixed - L * N * 8)
    nc = max(1, min(W, left // ((N + 1) * 8), 3072 // N))
    nch = -(-W // nc)
    nc = -(-W // nch)
    return L, nc, nch, W - (nch - 1) * nc, 8 * (nc * (N + 1) + L * N) + lds_fixed


def ragged_band(N):
    """Band half-width whose last k_prep column chunk is narrowest (a single column wherever the plan allows one, i.e. at
    boxes of 240 and up; below, chunks are as wide as 3072 / N and evening them leaves no one-column remainder), the widest
    such band."""
    best = min(range(8, N // 2), key=lambda B: (prep_plan(N, B)[3], -B))
    return best
