"""Float64 restatement of ppm_ctf_spectrum and ppm_ctf_fit (include/ppm.h) in numpy: the executable form of the
definition.  tests/test_ctf_cpu.py checks it against the reference-run fixture tests/golden/periodogram_cases.npz and against the truth
of synthetic data; tests/test_gpu_ctf.py holds the GPU to it.

  tiles: T x T, origins 0, h, 2 h, ... with h = T / 2, n // h of them per axis, an origin whose tile would leave the image pulled back
      to n - T (so where h divides n the last tile repeats the one before it and counts twice - the reference's rule, kept).
  movie: frames averaged in groups of g, in order, the last group holding what is left; every group's mean image is tiled.
  power: |rfft2(tile)|^2 averaged over all tiles of all groups; normalise: [0, 0] = 0, then divide by the maximum.
  fit:   crop to B_fit for a pixel below 1.4 A; ring means of sqrt(P), box-averaged background without ring 0, samples between the two
      resolutions minus background minus their mean; score = sum v |c| / sqrt(sum v^2 sum c^2) - (D / tol)^2 / (2 n); a grid over
      (mean defocus, astigmatism, angle), then a pattern search with 10 halvings (the second half of this file).
"""
import math

import numpy as np

import f64_ref as R
import f64_resample as FR

EPS32 = R.EPS32
CHUNK_TILES = 16                       # kCtfChunkTiles of ppm_ctf_plan.h


class Refused(ValueError):
    pass


tile_ok = FR.box_ok


def axis_origins(n, tile):
    h = tile // 2
    return [n - tile if i * h + tile > n else i * h for i in range(n // h)] if n >= tile else []


def group_means(frames, group):
    """frames [nf, ny, nx] -> float64 means of the groups of `group` frames, the last one of what is left."""
    f = np.asarray(frames, dtype=np.float64)
    return [f[i:i + group].mean(axis=0) for i in range(0, f.shape[0], group)]


def plan(shape, tile, group=1):
    """dict(tiles_x, tiles_y, groups, tiles, chunks): the counts of ppm_ctf_spectrum_plan; raises Refused as it refuses."""
    nf, ny, nx = ((1,) + tuple(shape))[-3:]
    if not tile_ok(tile):
        raise Refused("ERROR: ctf spectrum: the tile is not a size the transforms take")
    if group < 1 or group > nf:
        raise Refused("ERROR: ctf spectrum: the number of frames to average must be 1 .. the number of frames")
    if nx < tile or ny < tile:
        raise Refused("ERROR: ctf spectrum: the image is smaller than one tile")
    tx, ty, g = len(axis_origins(nx, tile)), len(axis_origins(ny, tile)), -(-nf // group)
    return dict(tiles_x=tx, tiles_y=ty, groups=g, tiles=g * tx * ty, chunks=-(-(g * tx * ty) // CHUNK_TILES))


def tile_stack(image, tile, group=1):
    """All tiles in walk order (group, tile row, tile column), float64 [tiles, T, T]."""
    a = np.asarray(image)
    plan(a.shape, tile, group)
    imgs = [a.astype(np.float64)] if a.ndim == 2 else group_means(a, group)
    ny, nx = imgs[0].shape
    return np.stack([im[y:y + tile, x:x + tile] for im in imgs for y in axis_origins(ny, tile) for x in axis_origins(nx, tile)])


def periodogram(image, tile, normalise=True, group=1):
    """float64 [T, T / 2 + 1]."""
    tiles = tile_stack(image, tile, group)
    p = np.zeros((tile, tile // 2 + 1))
    for t in tiles:
        p += np.abs(np.fft.rfft2(t)) ** 2
    p /= len(tiles)
    return normalised(p) if normalise else p


def normalised(p):
    p = p.copy()
    p[0, 0] = 0.0
    return p / p.max()


# ------------------------------------------------------------------------------------------ bounds
def bound_fixture(n_tiles):
    """Model against the reference's own float64 run, relative to the largest element (1 after the scaling): both sum the same n_tiles
    float64 terms in the same order, so what may differ is the rounding of |F|^2 (abs, then a power, against abs squared: two
    roundings), of the n_tiles additions, of the division by the count and of the division by the maximum, once for the element and
    once for the maximum itself: (n_tiles + 6) roundings of at most half an ulp each, doubled for a margin against how the two
    libraries' transforms order their own additions."""
    return 2.0 * (n_tiles + 6) * 0.5 * float(np.finfo(np.float64).eps)


def floor_spectrum(tile, group=1):
    """One float32 rounding per butterfly stage along a path: log2 T stages per axis (the radix-4 / 3 / 5 / 7 stages are fewer), one for
    the untangling of the row pair, and the group - 1 additions plus the scaling of a movie's frame mean."""
    return EPS32 * (2.0 * math.log2(tile) + 1.0 + (group if group > 1 else 0))


def bound_spectrum(image, tile, normalise=True, group=1):
    """Element-wise bound on |GPU - model| for ppm_ctf_spectrum, float64 [T, T / 2 + 1], in the style of f64_resample.bound_resample:

      dF = MAP_K floor_spectrum(T) L1 bounds the error of any transform value of a tile: every butterfly output is at most the sum of
           |x| over its inputs, so a rounding of one stage is at most EPS32 L1 with L1 = max over the tiles of sum |x|;
      a tile's power then errs by at most 2 |F| dF + dF^2; averaged over the tiles and with Cauchy-Schwarz (mean |F| <= sqrt(mean
           |F|^2)) that is 2 sqrt(P) dF + dF^2;
      the square, the n_tiles additions and the division add (n_tiles + 2) EPS32 P.

    Normalised, the bound is divided by the maximum M (taken away from [0, 0]) and the maximum's own error bound b(M) / M is added
    relative to the element, plus one rounding for the division."""
    tiles = tile_stack(image, tile, group)
    p = periodogram(image, tile, normalise=False, group=group)
    l1 = float(np.abs(tiles).sum(axis=(1, 2)).max())
    d_f = R.MAP_K * floor_spectrum(tile, group) * l1
    b = 2.0 * np.sqrt(p) * d_f + d_f * d_f + (len(tiles) + 2) * EPS32 * p
    if not normalise:
        return b
    q = p.copy()
    q[0, 0] = 0.0
    i = np.unravel_index(np.argmax(q), q.shape)
    m = q[i]
    out = b / m + (q / m) * (b[i] / m + EPS32)
    out[0, 0] = 0.0
    return out


def floor_multiple(got, want, image, tile, normalise=True, group=1):
    """max |got - want| in units of the bound without its safety factor MAP_K (what the tests print)."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (bound_spectrum(image, tile, normalise, group) / R.MAP_K + 1e-300)).max())


# ------------------------------------------------------------------------------------------ inputs of the tests
def make_image(shape, seed=5):
    """Seeded noise on an offset with a slow ramp (the mean and the gradient of a micrograph), float32."""
    rng = np.random.default_rng(seed)
    ny, nx = shape[-2:]
    ramp = 0.3 * np.arange(ny)[:, None] / ny - 0.2 * np.arange(nx)[None, :] / nx
    return (rng.standard_normal(shape) + 1.5 + ramp).astype(np.float32)


# ========================================================================================== the fit (ppm_ctf_fit)
RESAMPLE_TARGET = 1.4                  # ctffind's "target pixel size after resampling", which PYP leaves at its default
ASTIG_CAP = 1000.0                     # largest astigmatism of the grid when no restraint is given (the pattern search may leave it)
N_THETA, HALVINGS, SWEEPS = 12, 10, 8  # grid angles of 15 degrees; levels of the pattern search; sweeps per level at most
SINE_ABS = 2.0e-6                      # hardware sine (ppm_dev.h: ~1e-6 absolute) plus the float32 rounding of 2 pi rev


def wavelength(kv):
    v = kv * 1000.0
    return 12.2639 / math.sqrt(v + 0.97845e-6 * v * v)


def make_cfg(pixel, kv=300.0, cs=2.7, wgh=0.07, min_res=30.0, max_res=5.0, min_def=5000.0, max_def=50000.0, step=500.0, tol=0.0):
    return dict(pixel=float(pixel), kv=float(kv), cs=float(cs), wgh=float(wgh), min_res=float(min_res), max_res=float(max_res),
                min_def=float(min_def), max_def=float(max_def), step=float(step), tol=float(tol))


def fit_box(tile, pixel):
    """(B_fit, a_fit): the centre crop in Fourier space that brings a pixel below 1.4 A up to it."""
    if pixel >= RESAMPLE_TARGET:
        return tile, pixel
    b = 2 * int(math.floor(tile * pixel / RESAMPLE_TARGET / 2.0))
    return b, pixel * tile / b


def fit_plan(tile, cfg, lo=None, hi=None):
    """Counts of a fit: B_fit, a_fit, the integer |k|^2 range of the fitted samples, the background half width, the astigmatism steps,
    candidates per mean defocus, mean-defocus steps of a window.  Raises Refused as ppm_ctf_fit refuses."""
    if not (tile >= 8 and tile % 2 == 0 and tile <= 512):
        raise Refused("ERROR: ctf fit: the spectrum must be even, 8 .. 512")
    b, a = fit_box(tile, cfg["pixel"])
    if b < 8:
        raise Refused("ERROR: ctf fit: the pixel is too small for this tile")
    if not (cfg["min_res"] > cfg["max_res"] > 0 and cfg["step"] > 0):
        raise Refused("ERROR: ctf fit: resolutions and step")
    lo = cfg["min_def"] if lo is None else lo
    hi = cfg["max_def"] if hi is None else hi
    if not hi >= lo:
        raise Refused("ERROR: ctf fit: defocus window")
    k2lo = int(math.ceil((b * a / cfg["min_res"]) ** 2))
    k2hi = int(math.floor(min((b * a / cfg["max_res"]) ** 2, (b / 2.0) ** 2)))
    nj = int(math.floor((cfg["tol"] if cfg["tol"] > 0 else ASTIG_CAP) / cfg["step"] + 1e-9))
    return dict(tile=tile, B=b, a=a, k2lo=max(k2lo, 1), k2hi=k2hi, bg_w=int(math.ceil(b * a / cfg["min_res"])), nj=nj, nc=1 + N_THETA * nj,
                ni=int(math.floor((hi - lo) / cfg["step"] + 1e-9)) + 1)


def ring_of(k2):
    return np.floor(np.sqrt(k2) + 0.5).astype(np.int64)


def condition(power, cfg):
    """power [T, T / 2 + 1] -> dict(v, s2, c2, s2p: the compacted sample list in scan order (ky = -B/2 .. B/2 - 1, kx = 0 .. B/2), n, V, a_max,
    rings, bg, plan)."""
    p = np.asarray(power, dtype=np.float64)
    t = p.shape[0]
    pl = fit_plan(t, cfg)
    b, a = pl["B"], pl["a"]
    ky = np.arange(-b // 2, b // 2)
    amp = np.sqrt(p[ky % t][:, :b // 2 + 1])                       # the crop: rows by signed frequency
    kx = np.arange(b // 2 + 1)
    k2 = ky[:, None] ** 2 + kx[None, :] ** 2
    ring = ring_of(k2)
    nr = b // 2 + 1
    inside = ring < nr
    cnt = np.bincount(ring[inside], minlength=nr)
    mean = np.bincount(ring[inside], weights=amp[inside], minlength=nr) / cnt
    w = pl["bg_w"]
    bg = np.array([mean[max(1, r - w):max(max(1, r - w), min(nr - 1, r + w)) + 1].mean() for r in range(nr)])     # ring 0 (the image's mean) stays out
    sel = (k2 >= pl["k2lo"]) & (k2 <= pl["k2hi"]) & ~((kx[None, :] == 0) & (ky[:, None] < 0))
    v = amp[sel] - bg[ring[sel]]
    v = v - v.mean()
    k2s = k2[sel].astype(np.float64)
    kxs, kys = np.broadcast_to(kx[None, :], k2.shape)[sel], np.broadcast_to(ky[:, None], k2.shape)[sel]
    return dict(v=v, s2=k2s / (b * a) ** 2, c2=(kxs ** 2 - kys ** 2) / k2s, s2p=2.0 * kxs * kys / k2s, n=int(sel.sum()), V=float((v * v).sum()),
                a_max=float(amp.max()), rings=mean, bg=bg, plan=pl, amp=amp, ring=ring, kx=kx, ky=ky, k2=k2)


def chi(cond, cfg, dbar, delta, theta_deg):
    lam, cs = wavelength(cfg["kv"]), cfg["cs"] * 1e7
    th = np.deg2rad(theta_deg)
    df = 0.5 * (2.0 * dbar + delta * (cond["c2"] * np.cos(2 * th) + cond["s2p"] * np.sin(2 * th)))
    extra = math.atan(cfg["wgh"] / math.sqrt(1.0 - cfg["wgh"] ** 2))
    return math.pi * lam * cond["s2"] * (df - 0.5 * cs * lam * lam * cond["s2"]) + extra


def score(cond, cfg, dbar, delta, theta_deg, parts=False):
    c = np.abs(np.sin(chi(cond, cfg, dbar, delta, theta_deg)))
    cc = float((c * c).sum())
    s = float((cond["v"] * c).sum()) / math.sqrt(cond["V"] * cc)
    if cfg["tol"] > 0:
        s -= (delta / cfg["tol"]) ** 2 / (2.0 * cond["n"])
    return (s, cc) if parts else s


def candidate(cfg, pl, idx, lo=None):
    """(dbar, delta, theta in degrees) of grid candidate idx = i * nc + c: c = 0 is delta = 0; c = 1 + (j - 1) * 12 + k is delta = j step,
    theta = 15 k degrees."""
    lo = cfg["min_def"] if lo is None else lo
    i, c = divmod(idx, pl["nc"])
    if c == 0:
        return lo + i * cfg["step"], 0.0, 0.0
    j, k = divmod(c - 1, N_THETA)
    return lo + i * cfg["step"], (j + 1) * cfg["step"], 180.0 / N_THETA * k


def grid_scores(cond, cfg, lo=None, hi=None):
    """float64 [ni * nc] scores of the whole grid, and the smallest sum of c^2 met (the bound's C_min)."""
    pl = fit_plan(cond["plan"]["tile"], cfg, lo, hi)
    out = np.empty(pl["ni"] * pl["nc"])
    cmin = np.inf
    for idx in range(out.size):
        out[idx], cc = score(cond, cfg, *candidate(cfg, pl, idx, lo), parts=True)
        cmin = min(cmin, cc)
    return out, cmin


def refine(cond, cfg, start):
    """The pattern search from `start` = (dbar, delta, theta): steps (step, step, 15 degrees), per level at most SWEEPS sweeps of the six
    neighbours (delta kept >= 0; theta does not move while delta = 0), a move to the best neighbour only when it beats the current score
    (ties to the lowest neighbour), then all steps halved; HALVINGS levels after the first."""
    cur = list(start)
    best = score(cond, cfg, *cur)
    steps = [cfg["step"], cfg["step"], 180.0 / N_THETA]
    for _ in range(HALVINGS + 1):
        for _ in range(SWEEPS):
            mv, ms = None, best
            for q in range(6):
                ax, sg = q // 2, (1.0 if q % 2 == 0 else -1.0)
                t = list(cur)
                t[ax] += sg * steps[ax]
                if t[1] < 0 or (ax == 2 and cur[1] == 0):
                    continue
                s = score(cond, cfg, *t)
                if s > ms:
                    mv, ms = t, s
            if mv is None:
                break
            cur, best = mv, ms
        steps = [0.5 * s for s in steps]
    return tuple(cur), best


def reduce_angle(theta_deg):
    """ctffind's range (-90, 90]."""
    t = math.fmod(theta_deg, 180.0)
    if t > 90.0:
        t -= 180.0
    if t <= -90.0:
        t += 180.0
    return t


def estimate(power, cfg, lo=None, hi=None):
    """dict(df1, df2, angle, score, grid_index, grid_score, n) of one spectrum."""
    cond = condition(power, cfg)
    sc, _ = grid_scores(cond, cfg, lo, hi)
    gi = int(np.argmax(sc))                                         # ties: the lowest index
    pl = fit_plan(np.asarray(power).shape[0], cfg, lo, hi)
    (d, dl, th), s = refine(cond, cfg, candidate(cfg, pl, gi, lo))
    return dict(df1=d + dl / 2, df2=d - dl / 2, angle=reduce_angle(th), score=s, grid_index=gi, grid_score=float(sc[gi]), n=cond["n"])


def df_direction_error(est, truth, n_phi=360):
    """max over directions of |df_est(phi) - df_true(phi)|, each given as (df1, df2, angle in degrees)."""
    phi = np.linspace(0.0, np.pi, n_phi, endpoint=False)
    f = lambda p: 0.5 * (p[0] + p[1] + (p[0] - p[1]) * np.cos(2 * (phi - np.deg2rad(p[2]))))
    return float(np.abs(f(est) - f(truth)).max())


def truth_bound(cfg):
    """1 / (2 lambda s_max^2): the defocus change that moves the phase at max_res by pi / 2."""
    return cfg["max_res"] ** 2 / (2.0 * wavelength(cfg["kv"]))


def chi_max(cfg, pl, hi=None):
    hi = cfg["max_def"] if hi is None else hi
    s2 = pl["k2hi"] / (pl["B"] * pl["a"]) ** 2
    lam = wavelength(cfg["kv"])
    return math.pi * lam * s2 * (hi + 0.5 * (pl["nj"] + 1) * cfg["step"] + 0.5 * cfg["cs"] * 1e7 * lam * lam * s2) + 1.0


def bound_score(cond, cfg, c_min, hi=None):
    """Bound on |GPU score - model score| of one candidate:

      dc = 5 EPS32 |chi|max + SINE_ABS    ten float32 roundings of half an ulp on the way to chi (s^2, cos 2 phi, sin 2 phi as stored, the
                                          products and sums of ctf_eval_fast), then the hardware sine;
      dv = 2 EPS32 A_max                  the conditioning sums in double and rounds: sqrt, ring background, difference, mean removal;
      through the ratio N / sqrt(V C) with Cauchy-Schwarz (sum |v| <= sqrt(n V), sum |c| <= sqrt(n C)):
          dc sqrt(n / C) from N and as much from C, dv sqrt(n / V) from N and as much from V;
      the sums run in blocks of 256 samples whose totals are then added: (256 + n / 256 + 4) roundings of half an ulp on N and on C,
          with the square root, the division and the restraint."""
    n = cond["n"]
    d_c = 5.0 * EPS32 * chi_max(cfg, cond["plan"], hi) + SINE_ABS
    d_v = 2.0 * EPS32 * cond["a_max"]
    return 2.0 * d_c * math.sqrt(n / c_min) + 2.0 * d_v * math.sqrt(n / cond["V"]) + (256 + n / 256.0 + 4) * EPS32


def bound_score_rms(cond, cfg, c_min, hi=None):
    """Bound on the root mean square of (GPU score - model score) over the candidates of a grid, beside the worst case of bound_score: the
    same roundings taken as independent and of either sign, so that n of them add up to sqrt(n) times one, not n times: the factors
    sqrt(n / C) and sqrt(n / V) of the Cauchy-Schwarz step become 1 / sqrt(C) and 1 / sqrt(V) times the root of the mean square of the
    other factor, which is at most 1 for |c| and sqrt(V / n) for v, and the (256 + n / 256 + 4) summation roundings add in quadrature.
    A slip of a few ulps in the phase (a dropped rounding, another reduction constant) is systematic over the samples and shows here
    long before it reaches the worst-case bound."""
    n = cond["n"]
    d_c = 5.0 * EPS32 * chi_max(cfg, cond["plan"], hi) + SINE_ABS
    d_v = 2.0 * EPS32 * cond["a_max"]
    return 2.0 * d_c / math.sqrt(c_min) + 2.0 * d_v / math.sqrt(cond["V"]) + math.sqrt(256 + n / 256.0 + 4) * EPS32


# ------------------------------------------------------------------------------------------ synthetic spectra and micrographs
def ctf_2d(shape_t, pixel, cfg, df1, df2, angle):
    """CTF on the full transform grid of a t x t image, rows and columns in transform order (numpy's fftfreq)."""
    t = shape_t
    f = np.fft.fftfreq(t, d=pixel)
    ky, kx = np.meshgrid(f, f, indexing="ij")
    s2 = kx * kx + ky * ky
    phi = np.arctan2(ky, kx)
    lam, cs = wavelength(cfg["kv"]), cfg["cs"] * 1e7
    df = 0.5 * (df1 + df2 + (df1 - df2) * np.cos(2 * (phi - np.deg2rad(angle))))
    extra = math.atan(cfg["wgh"] / math.sqrt(1.0 - cfg["wgh"] ** 2))
    return -np.sin(math.pi * lam * s2 * (df - 0.5 * cs * lam * lam * s2) + extra), s2


def synthetic_power(tile, cfg, df1, df2, angle):
    """An exact spectrum (|CTF| envelope + smooth background)^2 on the half plane, no noise."""
    c, s2 = ctf_2d(tile, cfg["pixel"], cfg, df1, df2, angle)
    amp = np.abs(c) * np.exp(-20.0 * s2) + 0.5 + 2.0 * np.exp(-60.0 * s2)
    return (amp ** 2)[:, :tile // 2 + 1]


def synthetic_micrograph(shape, cfg, df1, df2, angle, seed=7, snr=1.0):
    """White noise filtered by the CTF (periodic over the whole image, so every tile sees the same CTF) plus white noise, float32."""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    fy, fx = np.fft.fftfreq(ny, d=cfg["pixel"]), np.fft.fftfreq(nx, d=cfg["pixel"])
    ky, kx = np.meshgrid(fy, fx, indexing="ij")
    s2 = kx * kx + ky * ky
    phi = np.arctan2(ky, kx)
    lam, cs = wavelength(cfg["kv"]), cfg["cs"] * 1e7
    df = 0.5 * (df1 + df2 + (df1 - df2) * np.cos(2 * (phi - np.deg2rad(angle))))
    extra = math.atan(cfg["wgh"] / math.sqrt(1.0 - cfg["wgh"] ** 2))
    c = -np.sin(math.pi * lam * s2 * (df - 0.5 * cs * lam * lam * s2) + extra)
    sig = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * c * np.exp(-10.0 * s2)).real
    return (snr * sig / sig.std() + rng.standard_normal(shape) + 2.0).astype(np.float32)


# ------------------------------------------------------------------------------------------ the fit's test cases (CPU and GPU tests share them)
CFG_BOXES = dict(pixel=3.0, min_res=40.0, max_res=8.0, min_def=4000.0, max_def=9000.0, step=500.0)
CFG_CROP = dict(pixel=1.0, min_res=30.0, max_res=5.0, min_def=3000.0, max_def=8000.0, step=500.0)
CFG_MICROGRAPH = dict(pixel=2.0, min_res=40.0, max_res=6.0, min_def=3000.0, max_def=15000.0, step=250.0)
MICROGRAPH_TRUTH = (8200.0, 7700.0, 35.0)


def batch_case(box, n, windows, seed, crop=False, tol=0.0):
    """n exact spectra of size `box` with seeded truths; windows: per-spectrum +-1000 A around the truth's mean (rounded to 100 A).
    Returns (cfg, float32 spectra [n, box, box / 2 + 1], truths [n, 3], windows [n, 2] or None)."""
    cfg = make_cfg(**dict(CFG_CROP if crop else CFG_BOXES, tol=tol))
    rng = np.random.default_rng(seed)
    truths, spectra = [], []
    for _ in range(n):
        d, dl, th = rng.uniform(cfg["min_def"] + 1200, cfg["max_def"] - 1200), rng.uniform(300.0, 900.0), rng.uniform(-90.0, 90.0)
        truths.append((d + dl / 2, d - dl / 2, th))
        spectra.append(synthetic_power(box, cfg, *truths[-1]) * (1.0 + 0.02 * rng.standard_normal((box, box // 2 + 1))) ** 2)
    truths = np.array(truths)
    win = None
    if windows:
        mid = np.round(truths[:, :2].mean(axis=1) / 100.0) * 100.0
        win = np.stack([mid - 1000.0, mid + 1000.0], axis=1)
    return cfg, np.stack(spectra).astype(np.float32), truths, win


def model_batch(cfg, spectra, win=None):
    """Per spectrum: dict(cond, scores, c_min, bound, est) of the model; spectra as the GPU gets them (float32)."""
    out = []
    for i, p in enumerate(spectra):
        lo, hi = (None, None) if win is None else (float(win[i, 0]), float(win[i, 1]))
        cond = condition(p, cfg)
        sc, cmin = grid_scores(cond, cfg, lo, hi)
        pl = fit_plan(p.shape[0], cfg, lo, hi)
        gi = int(np.argmax(sc))
        (d, dl, th), s = refine(cond, cfg, candidate(cfg, pl, gi, lo))
        out.append(dict(cond=cond, scores=sc, c_min=cmin, bound=bound_score(cond, cfg, cmin, hi), bound_rms=bound_score_rms(cond, cfg, cmin, hi), plan=pl, lo=lo, grid_index=gi,
                        refined=(d, dl, th), refined_score=s))
    return out


def lead(scores):
    """How far the best grid score is ahead of the second best."""
    s = np.sort(scores)
    return float(s[-1] - s[-2])


# ------------------------------------------------------------------------------------------ profile (k_ctf_profile)
FIT_THRESHOLD = 0.5


def profile(power, cfg, dbar, delta, theta_deg):
    """(avrot float64 [6, B / 2 + 1], fit resolution in A, diagnostic image float64 [B, B]) for the given parameters, as include/ppm.h
    states them."""
    cond = condition(power, cfg)
    pl, amp, ring, bg, mean = cond["plan"], cond["amp"], cond["ring"], cond["bg"], cond["rings"]
    b, a, w = pl["B"], pl["a"], pl["bg_w"]
    nr = b // 2 + 1
    kx, ky, k2 = cond["kx"][None, :], cond["ky"][:, None], cond["k2"]
    th = np.deg2rad(theta_deg)
    lam, cs = wavelength(cfg["kv"]), cfg["cs"] * 1e7
    k1, k2c = np.float32(math.pi * lam).astype(np.float64), np.float32(0.5 * cs * lam * lam).astype(np.float64)    # the constants as the kernels hold them
    extra = float(np.float32(math.atan(cfg["wgh"] / math.sqrt(1.0 - cfg["wgh"] ** 2))))
    k2s = np.where(k2 > 0, k2, 1)
    df = dbar + 0.5 * delta * (((kx * kx - ky * ky) * math.cos(2 * th) + 2.0 * kx * ky * math.sin(2 * th)) / k2s)
    warp = dbar > 0 and dbar - 0.5 * delta > 0
    f = np.sqrt(df / dbar) if warp else np.ones_like(df)
    f = np.where(k2 > 0, f, 1.0)
    inside = ring < nr
    tgt = np.floor(np.sqrt(k2) * f + 0.5).astype(np.int64)
    ok = inside & (tgt < nr)
    val = amp - bg[np.minimum(ring, nr - 1)]
    cnt = np.bincount(tgt[ok], minlength=nr).astype(np.float64)
    eq = np.bincount(tgt[ok], weights=val[ok], minlength=nr) / np.maximum(cnt, 1)
    eq[0] = 0.0
    freq = np.arange(nr) / (b * a)
    fit = np.abs(np.sin(k1 * freq ** 2 * (dbar - k2c * freq ** 2) + extra))
    rot = mean - bg
    rot[0] = 0.0
    qual, noise = np.zeros(nr), np.zeros(nr)
    for r in range(nr):
        lo = max(1, r - w)
        hi = max(lo, min(nr - 1, r + w))
        x, y = eq[lo:hi + 1] - eq[lo:hi + 1].mean(), fit[lo:hi + 1] - fit[lo:hi + 1].mean()
        sxx, syy = (x * x).sum(), (y * y).sum()
        qual[r] = (x * y).sum() / math.sqrt(sxx * syy) if sxx > 0 and syy > 0 else 0.0
        n = cnt[lo:hi + 1].sum()
        noise[r] = 1.0 / math.sqrt(n) if n > 0 else 0.0
    res = 1.0 / freq[-1]
    for r in range(1, nr):
        if freq[r] > 1.0 / cfg["min_res"] and qual[r] < FIT_THRESHOLD:
            res = 1.0 / freq[r]
            break
    # diagnostic image: rows ky = -B/2 .. B/2 - 1, columns kx = -B/2 .. B/2 - 1
    diag = np.zeros((b, b))
    right = np.where(inside & (ring > 0), val, 0.0)
    diag[:, b // 2:] = right[:, :b // 2]
    kxl = np.arange(-b // 2, 0)[None, :]
    k2l = kxl * kxl + ky * ky
    dfl = dbar + 0.5 * delta * (((kxl * kxl - ky * ky) * math.cos(2 * th) + 2.0 * kxl * ky * math.sin(2 * th)) / k2l)
    s2l = k2l / (b * a) ** 2
    diag[:, :b // 2] = np.abs(np.sin(k1 * s2l * (dfl - k2c * s2l) + extra))
    return np.stack([freq, rot, eq, fit, qual, noise]), res, diag
