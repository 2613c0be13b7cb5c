"""Float64 restatement of ppm_postprocess (include/ppm.h) in numpy: what tests/test_post_cpu.py checks against itself and
tests/test_gpu_post.py holds the GPU to.

  shell(k) = floor(|k| + 1/2) by the integer |k|^2, shells 0 .. N/2;  FSC(s) = sum Re F1 F2* / sqrt(sum |F1|^2 sum |F2|^2)
  U = FSC(H1, H2), Mk = FSC(M H1, M H2), Rd = FSC(M H1r, M H2r) with the phases of H1, H2 randomised from shell s_r on
  C = Mk below s_r + 2, (Mk - Rd) / (1 - Rd) from there;  resolution: first C < 0.143, interpolated in frequency
  W = w exp(-B f^2 / 4) L;  unmasked = Re IFFT(W FFT((H1 + H2) / 2)), masked = M unmasked

The transforms are numpy.fft.fftn of the whole cube in float64, the sums np.bincount over every coefficient: nothing of the kernels'
packing, pairing or half-space walk is repeated here.  The hash is the definition's, in uint32 arithmetic.
"""
import math

import numpy as np

import f64_create_mask as CM
import f64_mask as FM
import f64_ref as R

EPS32 = R.EPS32
CUT = 0.143
MASK_EDGE = 6              # cosine edge of the automatic mask (voxels)
REBIN = 0.5

DEFAULTS = dict(mask="none", automask_lp=0.0, threshold_method="intensity", threshold_value=0.0, randomize="fsc", randomize_value=0.8,
                seed=0, bfactor="none", adhoc_bfac=0.0, fit_low=10.0, fit_high=0.0, lowpass="auto", highpass=0.0, gaussian=False,
                skip_fsc_weighting=False, apply_fsc2=False, flip_x=False, flip_y=False, flip_z=False)


class Refused(ValueError):
    pass


def options(**kw):
    """The options of abi.PostCfg.make, by the same names and defaults."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def box_ok(n):
    if n % 2 or not 32 <= n <= 512:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


# ------------------------------------------------------------------------------------------ shells
def shell_cube(n):
    """shell of every coefficient of the cube in numpy's index order, -1 beyond shell N/2: s^2 - s < |k|^2 <= s^2 + s, in integers."""
    k = np.fft.fftfreq(n, 1.0 / n).astype(np.int64)
    k2 = (k * k)[:, None, None] + (k * k)[None, :, None] + (k * k)[None, None, :]
    s = np.floor(np.sqrt(k2.astype(np.float64)) + 0.5).astype(np.int64)
    s = np.where(k2 > s * s + s, s + 1, s)
    s = np.where((k2 <= s * s - s) & (s > 0), s - 1, s)
    assert (((k2 > s * s - s) | (s == 0)) & (k2 <= s * s + s)).all()
    return np.where(s <= n // 2, s, -1)


def shell_sums(F1, F2, sh):
    """[N/2 + 1, 4]: sum Re F1 F2*, sum |F1|^2, sum |F2|^2, coefficients."""
    n = sh.shape[0]
    ok = sh >= 0
    idx = sh[ok]
    a, b = F1[ok], F2[ok]
    cols = [(a * np.conj(b)).real, np.abs(a) ** 2, np.abs(b) ** 2, np.ones(idx.shape)]
    return np.stack([np.bincount(idx, weights=c, minlength=n // 2 + 1) for c in cols], axis=1)


def fsc_of(sums):
    d = sums[:, 1] * sums[:, 2]
    return np.where(d > 0, sums[:, 0] / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)


def rho(F, sh):
    """sqrt(mean |F|^2 over all coefficients / smallest shell mean of |F|^2): how much weaker than the average the weakest shell is."""
    p = np.abs(F) ** 2
    ok = sh >= 0
    means = np.bincount(sh[ok], weights=p[ok]) / np.bincount(sh[ok])
    return float(math.sqrt(p.mean() / means.min()))


# ------------------------------------------------------------------------------------------ phase randomisation
def mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D); x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B); x ^= x >> np.uint32(16)
    return x


def randomise(F1, F2, sh, s_r, seed):
    """Both transforms with new phases from shell s_r on (what lies beyond shell N/2 included); partners get conjugates, self-conjugate
    coefficients stay."""
    n = sh.shape[0]
    i = np.arange(n, dtype=np.int64)
    p = (n - i) % n
    lin = (i[:, None, None] * n + i[None, :, None]) * n + i[None, None, :]
    plin = (p[:, None, None] * n + p[None, :, None]) * n + p[None, None, :]
    beyond = (sh < 0) | (sh >= s_r)
    sel = (lin < plin) & beyond
    c = lin[sel].astype(np.uint32)
    with np.errstate(over="ignore"):
        h1 = mix32(c ^ np.uint32((int(seed) * 0x9E3779B9) & 0xFFFFFFFF))
        h2 = mix32(h1 ^ np.uint32(0x85EBCA6B))
    out = []
    for F, h in ((F1, h1), (F2, h2)):
        phi = 2.0 * math.pi * (h >> np.uint32(8)).astype(np.float64) / 2.0 ** 24
        G = F.copy().reshape(-1)
        v = np.abs(F[sel]) * np.exp(1j * phi)
        G[lin[sel]] = v
        G[plin[sel]] = np.conj(v)
        out.append(G.reshape(F.shape))
    return out


# ------------------------------------------------------------------------------------------ mask
def automask(h1, h2, pixel, opt):
    """(soft mask float64, body uint8, threshold used, low-passed mean map, info of create_mask)."""
    n = h1.shape[0]
    A = (np.float32(0.5) * (np.asarray(h1, np.float32) + np.asarray(h2, np.float32))).astype(np.float32)
    lp = float(opt["automask_lp"])
    radius_A = 0.5 * n * pixel
    edge = min(CM.EDGE_PX, 2.0 * n * pixel / lp) if lp > 0 else 0.0
    L = CM.lowpassed(A, pixel, lp, edge)
    sph = CM.sphere(n, radius_A, pixel)
    v = L[sph]
    if opt["threshold_method"] == "intensity":
        t = float(opt["threshold_value"])
    elif opt["threshold_method"] == "sigma":
        mean = v.sum() / v.size
        t = float(mean + opt["threshold_value"] * math.sqrt(max(0.0, (v * v).sum() / v.size - mean * mean)))
    else:
        k = min(max(int(math.ceil(opt["threshold_value"] * v.size)), 1), v.size)
        t = float(np.partition(v, v.size - k)[v.size - k])
    body, info = CM.create_mask(A, pixel, radius_A, t, lp, edge, REBIN, L=L)
    return FM.soft_mask(body.astype(np.float32), MASK_EDGE), body, t, L, info


# ------------------------------------------------------------------------------------------ curves
def curves(h1, h2, pixel, opt, mask=None, sh=None):
    """dict(U, Mk, Rd, C, sums_m, shell_count, s_r, rho = (unmasked, masked, randomised pair), mask, imag = largest imaginary part of the
    back-transformed randomised halves over their largest modulus)."""
    n = h1.shape[0]
    if not box_ok(n):
        raise Refused(f"ERROR: postprocess: the box must be even, 32..512, with prime factors 2, 3, 5, 7, got {n}")
    if opt["skip_fsc_weighting"] and opt["apply_fsc2"]:
        raise Refused("ERROR: postprocess: skip_fsc_weighting and apply_fsc2 exclude each other")
    sh = shell_cube(n) if sh is None else sh
    a, b = np.asarray(h1, np.float32).astype(np.float64), np.asarray(h2, np.float32).astype(np.float64)
    extra = {}
    if opt["mask"] == "auto":
        M, body, t, L, info = automask(h1, h2, pixel, opt)
        extra = dict(body=body, threshold=t, L=L, mask_info=info)
    elif opt["mask"] == "external":
        M = np.clip(np.asarray(mask, np.float32), 0.0, 1.0).astype(np.float64)
    else:
        M = np.ones_like(a)
    F1, F2 = np.fft.fftn(a), np.fft.fftn(b)
    su = shell_sums(F1, F2, sh)
    U = fsc_of(su)
    ns = n // 2 + 1
    if opt["randomize"] == "resolution":
        s_r = int(min(math.floor(n * pixel / opt["randomize_value"] + 0.5), ns - 1))
    else:
        below = np.flatnonzero(U[1:] < opt["randomize_value"])
        s_r = int(below[0]) + 1 if below.size else ns - 1
    s_r = max(1, min(s_r, ns - 1))
    G1, G2 = randomise(F1, F2, sh, s_r, opt["seed"])
    r1, r2 = np.fft.ifftn(G1), np.fft.ifftn(G2)
    imag = max(np.abs(r1.imag).max(), np.abs(r2.imag).max()) / max(np.abs(r1).max(), np.abs(r2).max())
    M1, M2 = np.fft.fftn(M * a), np.fft.fftn(M * b)
    R1, R2 = np.fft.fftn(M * r1.real), np.fft.fftn(M * r2.real)
    sm, sr = shell_sums(M1, M2, sh), shell_sums(R1, R2, sh)
    Mk, Rd = fsc_of(sm), fsc_of(sr)
    return dict(U=U, Mk=Mk, Rd=Rd, C=corrected(Mk, Rd, s_r), sums_m=sm, shell_count=su[:, 3].astype(np.int64), s_r=s_r,
                rho=(max(rho(F1, sh), rho(F2, sh)), max(rho(M1, sh), rho(M2, sh)), max(rho(R1, sh), rho(R2, sh))), mask=M, imag=float(imag), **extra)


def corrected(Mk, Rd, s_r):
    s = np.arange(len(Mk))
    d = 1.0 - Rd
    return np.where(s < s_r + 2, Mk, np.where(d < 1e-6, 0.0, (Mk - Rd) / np.where(d < 1e-6, 1.0, d)))


def resolution(C, n, pixel):
    """(shell that decides: the first with C < 0.143, 0 if none; frequency in 1/A; resolution in A)."""
    df = 1.0 / (n * pixel)
    below = np.flatnonzero(C[1:] < CUT)
    if not below.size:
        return 0, (n // 2) * df, 1.0 / ((n // 2) * df)
    s = int(below[0]) + 1
    up = C[s - 1] - C[s]
    f = ((s - 1) + (C[s - 1] - CUT) / up) * df if up > 0 and C[s - 1] >= CUT else s * df
    return s, f, 1.0 / f


def fsc_weight(C, opt):
    C = np.asarray(C, np.float64)
    if opt["skip_fsc_weighting"]:
        return np.ones_like(C)
    pos = np.where(C > 0, C, 0.0)
    return pos ** 2 if opt["apply_fsc2"] else np.sqrt(2.0 * pos / (1.0 + pos))


def shell_power(sums_m):
    """P(s): shell mean of |F1 + F2|^2 / 4 of the masked halves."""
    return 0.25 * (sums_m[:, 1] + sums_m[:, 2] + 2.0 * sums_m[:, 0]) / sums_m[:, 3]


def fit_shells(C, n, pixel, opt, f_res):
    f = np.arange(len(C)) / (n * pixel)
    f_hi = 1.0 / opt["fit_high"] if opt["fit_high"] > 0 else f_res
    ok = (f >= 1.0 / opt["fit_low"]) & (f <= f_hi) & (fsc_weight(C, opt) > 0)
    ok[0] = False
    return np.flatnonzero(ok)


def bfactor(C, sums_m, n, pixel, opt, f_res):
    if opt["bfactor"] == "adhoc":
        return float(opt["adhoc_bfac"])
    if opt["bfactor"] == "none":
        return 0.0
    idx = fit_shells(C, n, pixel, opt, f_res)
    if len(idx) < 3:
        raise Refused(f"ERROR: postprocess: the automatic B-factor needs at least three shells, got {len(idx)}")
    x = (idx / (n * pixel)) ** 2
    y = np.log(np.sqrt(shell_power(sums_m)[idx]) * fsc_weight(C, opt)[idx])
    return float(4.0 * ((x - x.mean()) * (y - y.mean())).sum() / ((x - x.mean()) ** 2).sum())


def band_pass(n, pixel, opt, res):
    s = np.arange(n // 2 + 1, dtype=np.float64)
    L = np.ones_like(s)
    lp = res if opt["lowpass"] == "auto" else float(opt["lowpass"])
    for cut_A, low in ((lp, True), (float(opt["highpass"]), False)):
        if not cut_A > 0:
            continue
        sc = n * pixel / cut_A
        if opt["gaussian"]:
            g = np.exp(-math.log(2.0) * (s / sc) ** 2)
        else:
            g = np.where(s <= sc - 1, 1.0, np.where(s >= sc + 1, 0.0, 0.5 * (1.0 + np.cos(math.pi * (s - (sc - 1)) / 2.0))))
        L *= g if low else 1.0 - g
    return L


def filter_table(C, sums_m, n, pixel, opt, res=None, B=None):
    """(W by shell, B, resolution): decided here from C, or with the resolution and B the caller hands in."""
    _, f_res, r = resolution(C, n, pixel)
    res = r if res is None else res
    B = bfactor(C, sums_m, n, pixel, opt, 1.0 / res) if B is None else B
    f = np.arange(n // 2 + 1) / (n * pixel)
    return fsc_weight(C, opt) * np.exp(-B * f * f / 4.0) * band_pass(n, pixel, opt, res), B, res


def maps(h1, h2, M, W, opt, sh=None):
    """(unmasked, masked) in float64, flips applied."""
    n = h1.shape[0]
    sh = shell_cube(n) if sh is None else sh
    A = 0.5 * (np.asarray(h1, np.float32).astype(np.float64) + np.asarray(h2, np.float32).astype(np.float64))
    Wc = np.where(sh >= 0, np.concatenate([W, [0.0]])[sh], 0.0)
    un = np.fft.ifftn(Wc * np.fft.fftn(A)).real
    ma = M * un
    for ax, key in ((2, "flip_x"), (1, "flip_y"), (0, "flip_z")):
        if opt[key]:
            un, ma = np.flip(un, ax), np.flip(ma, ax)
    return un, ma


def postprocess(h1, h2, pixel, opt, mask=None):
    """The whole definition: the dict of `curves` plus unmasked, masked, W, bfactor, resolution, res_shell."""
    n = h1.shape[0]
    sh = shell_cube(n)
    c = curves(h1, h2, pixel, opt, mask=mask, sh=sh)
    W, B, res = filter_table(c["C"], c["sums_m"], n, pixel, opt)
    un, ma = maps(h1, h2, c["mask"], W, opt, sh=sh)
    c.update(unmasked=un, masked=ma, W=W, bfactor=B, resolution=res, res_shell=resolution(c["C"], n, pixel)[0])
    return c


# ------------------------------------------------------------------------------------------ tolerances (tests/test_gpu_post.py)
def eps_k(n, k):
    """k complex 3-D transforms in float32: EPS32 x 3k log2 N."""
    return EPS32 * 3.0 * k * math.log2(n)


def curve_tolerances(n, c):
    """(tol_U, tol_Mk, tol_Rd, tol_C by shell) from the float64 side's rho and Rd."""
    tol_u = R.MAP_K * 4.0 * c["rho"][0] * eps_k(n, 1)
    tol_m = R.MAP_K * 4.0 * c["rho"][1] * eps_k(n, 1)
    tol_r = R.MAP_K * 4.0 * c["rho"][2] * eps_k(n, 3)
    s = np.arange(n // 2 + 1)
    d = np.where(s < c["s_r"] + 2, 1.0, 1.0 - c["Rd"])
    tol_c = np.where(s < c["s_r"] + 2, tol_m, (tol_m + 2.0 * tol_r) / d ** 2)
    return tol_u, tol_m, tol_r, tol_c


def gaps(n, c, fsc_value):
    """(smallest |U - fsc_value| / tol_U over the shells 1 .. s_r that decide s_r under the fsc method, smallest |C - 0.143| / tol_C
    over the shells 1 .. the first below 0.143): how many tolerances the float64 curves keep from the thresholds."""
    tol_u, _, _, tol_c = curve_tolerances(n, c)
    s_r = c["s_r"]
    s = resolution(c["C"], n, 1.0)[0]
    gu = float(np.abs(c["U"][1:s_r + 1] - fsc_value).min() / tol_u)
    gc = float((np.abs(c["C"][1:s + 1] - CUT) / tol_c[1:s + 1]).min()) if s else 0.0
    return gu, gc


def bfactor_bound(n, c, idx, pixel):
    """|dB| <= 4 d sum|x - mean| / sum (x - mean)^2 over the fit's shells idx, x = f^2, d the error of ln(sqrt(P) w) per shell:
    2 rho eps_1 MAP_K from P, tol_C / (2 x 0.143 x 1.143) from w = sqrt(2C / (1 + C)) where C >= 0.143."""
    tol_c = curve_tolerances(n, c)[3]
    d = 2.0 * c["rho"][1] * eps_k(n, 1) * R.MAP_K + float(tol_c[idx].max()) / (2.0 * CUT * (1.0 + CUT))
    x = (idx / (n * pixel)) ** 2
    return 4.0 * d * np.abs(x - x.mean()).sum() / ((x - x.mean()) ** 2).sum()


# ------------------------------------------------------------------------------------------ inputs of the tests
PIXEL = 1.5
# seeds of make_halves at which the float64 curves keep 100 tolerances from 0.8 (shells up to s_r) and from 0.143 (shells up to the
# first below it) with make_mask, found by trying seeds 1 .. 400 in turn; tests/test_post_cpu.py asserts the gaps
SEEDS = {32: 348, 48: 241, 70: 105}
AUTOMASK_LP = 12.0


def automask_case(n, seed=None):
    """An intensity threshold for the automatic mask of make_halves(n): the middle of the widest gap of the low-passed mean map inside a
    window of its range over the sphere, the windows tried in turn until the low-passed body also keeps clear of the re-bin value 1/2.
    dict(h1, h2, t, t_gap, b_gap: in bands of f64_mask.bound_filtered; body, soft, L, info)."""
    h1, h2 = make_halves(n, SEEDS.get(n, 1) if seed is None else seed)
    opt = options(mask="auto", automask_lp=AUTOMASK_LP)
    A = (np.float32(0.5) * (h1 + h2)).astype(np.float32)
    edge = min(CM.EDGE_PX, 2.0 * n * PIXEL / AUTOMASK_LP)
    L = CM.lowpassed(A, PIXEL, AUTOMASK_LP, edge)
    sph = CM.sphere(n, 0.5 * n * PIXEL, PIXEL)
    mn, mx = L[sph].min(), L[sph].max()
    for frac in (0.30, 0.35, 0.40, 0.45, 0.25, 0.50, 0.20):
        mid, half = mn + frac * (mx - mn), 0.025 * (mx - mn)
        t, t_gap = CM.pick_threshold(L[sph], mid - half, mid + half, FM.bound_filtered(n, L))
        t = float(np.float32(t))
        body, info = CM.create_mask(A, PIXEL, 0.5 * n * PIXEL, t, AUTOMASK_LP, edge, REBIN, L=L)
        b_gap = float(np.abs(info["S"][sph] - REBIN).min() / FM.bound_filtered(n, info["S"]))
        if t_gap >= 4 and b_gap >= 4:
            break
    else:
        raise AssertionError("no window with room on both sides")
    opt["threshold_value"] = t
    return dict(h1=h1, h2=h2, opt=opt, t=t, t_gap=t_gap, b_gap=b_gap, body=body, soft=FM.soft_mask(body.astype(np.float32), MASK_EDGE), L=L, info=info)


def make_halves(n, seed=1):
    """40 Gaussians (sigma 1.2 voxels, height 4) at seeded positions within 0.25 N of the centre, plus independent white noise of
    sigma 0.5 in each half: no shell is weak.  (half1, half2) float32, read-only."""
    rng = np.random.default_rng(seed)
    pos = []
    while len(pos) < 40:
        p = rng.uniform(-0.25 * n, 0.25 * n, 3)
        if (p * p).sum() <= (0.25 * n) ** 2:
            pos.append(p + n / 2)
    g = np.arange(n, dtype=np.float64)
    sig = np.zeros((n, n, n))
    for pz, py, px in pos:
        ez, ey, ex = (np.exp(-(g - q) ** 2 / (2 * 1.2 ** 2)) for q in (pz, py, px))
        sig += 4.0 * ez[:, None, None] * ey[None, :, None] * ex[None, None, :]
    out = []
    for _ in range(2):
        h = (sig + 0.5 * rng.standard_normal((n, n, n))).astype(np.float32)
        h.setflags(write=False)
        out.append(h)
    return tuple(out)


def make_mask(n):
    """Ball of radius 0.3 N about the centre with a 4-voxel cosine edge, float32, read-only."""
    g = np.arange(n, dtype=np.float64) - n / 2
    r = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    d = r - 0.3 * n
    m = np.where(d <= 0, 1.0, np.where(d >= 4, 0.0, 0.5 * (1.0 + np.cos(math.pi * d / 4.0)))).astype(np.float32)
    m.setflags(write=False)
    return m
