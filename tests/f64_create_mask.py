"""Float64 restatement of ppm_create_mask (include/ppm.h) in numpy: what tests/test_create_mask_cpu.py checks against
itself and tests/test_gpu_create_mask.py holds the GPU to.

  sphere = voxels with integer (x - c)^2 + (y - c)^2 + (z - c)^2 <= (R_o / a)^2, c = N // 2, the right side in float64
  L      = V, or Re IFFT3(H FFT3(V)) with the cosine-edge low-pass of f64_mask around r_c = N a / R_lp, e wide
  B0     = sphere and {L >= t}, t rounded to float32 once; empty: refused, the message holds min / max of L over the sphere
  C      = the body of B0 under 26-connectivity with the most voxels, among equals the one with the smallest linear index
  mask   = C, or sphere and {Re IFFT3(H FFT3(1_C)) >= b}, b rounded to float32 once

The labelling is scipy.ndimage.label with a full 3 x 3 x 3 structure when scipy imports, else `label_runs`: the scheme of the kernels
(runs along x, unions with the runs of the four earlier neighbour rows that overlap the run widened by one voxel, minimum-id roots) in
vectorised numpy.  The CPU test compares the two whenever scipy is there.

Where the GPU has to agree voxel for voxel after a float32 transform, the thresholds are chosen by `pick_threshold`: the midpoint of the
widest gap between consecutive values of L (of the low-passed body) in a window, with the gap measured in units of the bound the filtered
map of apply_mask is already held to (f64_mask.bound_filtered).  A gap of four bands leaves no voxel within two bands of the comparison,
and the GPU is within one band: every comparison then falls the same way.
"""
import numpy as np

import f64_mask as FM

try:
    from scipy import ndimage as _ndimage
except ImportError:          # pragma: no cover
    _ndimage = None

EDGE_PX = 4.0                # what the drop-in sends for e (prompts.CREATE_MASK_EDGE_PX), clipped to 2 r_c


# ------------------------------------------------------------------------------------------ pieces of the definition
def sphere(n, radius_A, pixel):
    c = n // 2
    k = (np.arange(n, dtype=np.int64) - c) ** 2
    return (k[:, None, None] + k[None, :, None] + k[None, None, :]) <= (float(radius_A) / float(pixel)) ** 2


def lowpassed(vol, pixel, lowpass_A, edge_px):
    v = np.asarray(vol, dtype=np.float32).astype(np.float64)
    return v if lowpass_A == 0 else FM.outside_fft(v, pixel, lowpass_A, edge_px)


def label_scipy(b):
    lab, k = _ndimage.label(b, structure=np.ones((3, 3, 3), dtype=bool))
    return lab, int(k)


def runs_of(b):
    """(row, first x, last x) of every maximal run along x, in linear order; row = z N + y."""
    n = b.shape[0]
    rows = b.reshape(n * n, n)
    pad = np.zeros((n * n, n + 2), dtype=np.int8)
    pad[:, 1:-1] = rows
    d = np.diff(pad, axis=1)
    r0, x0 = np.nonzero(d == 1)
    r1, x1 = np.nonzero(d == -1)
    assert np.array_equal(r0, r1)
    return r0.astype(np.int64), x0.astype(np.int64), x1.astype(np.int64) - 1


def label_runs(b):
    """Run-based union-find: returns (labels, number of bodies); labels are 1 + rank of the body by its smallest linear index, 0 outside.
    Pairs of touching runs come from two binary searches per neighbour row; the bodies from minimum hooking and pointer jumping."""
    n = b.shape[0]
    row, first, last = runs_of(b)
    nr = len(row)
    if nr == 0:
        return np.zeros(b.shape, dtype=np.int64), 0
    z, y = row // n, row % n
    key_last, key_first = row * (n + 2) + last, row * (n + 2) + first         # ascending: runs are in linear order
    us, vs = [], []
    for dy, dz in ((-1, 0), (-1, -1), (0, -1), (1, -1)):
        ny, nz = y + dy, z + dz
        ok = (ny >= 0) & (ny < n) & (nz >= 0)
        nrow = nz * n + ny
        lo = np.searchsorted(key_last, nrow * (n + 2) + first - 1, side="left")        # first run of that row ending at or after first - 1
        hi = np.searchsorted(key_first, nrow * (n + 2) + last + 1, side="right")       # one past the last run starting at or before last + 1
        cnt = np.where(ok, np.maximum(hi - lo, 0), 0)
        u = np.repeat(np.arange(nr), cnt)
        off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        us.append(u)
        vs.append(np.repeat(lo, cnt) + off)
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(nr)
    while True:
        pu, pv = parent[u], parent[v]
        m = np.minimum(pu, pv)
        if np.array_equal(pu, pv):
            break
        np.minimum.at(parent, pu, m)
        np.minimum.at(parent, pv, m)
        while True:
            g = parent[parent]
            if np.array_equal(g, parent):
                break
            parent = g
    roots, inv = np.unique(parent, return_inverse=True)
    lab = np.zeros((n * n, n), dtype=np.int64)
    lens = last - first + 1
    idx = np.repeat(row * n + first, lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    lab.reshape(-1)[idx] = np.repeat(inv + 1, lens)
    return lab.reshape(b.shape), len(roots)


def label(b):
    return label_scipy(b) if _ndimage is not None else label_runs(b)


def largest_body(b0, labeller=None):
    """(C, number of bodies, voxels of C)."""
    lab, k = (labeller or label)(b0)
    sizes = np.bincount(lab.reshape(-1), minlength=k + 1)[1:]
    # both labellers number the bodies in the order of their first voxel: among equals, the smallest label holds the smallest linear index
    c = lab == int(np.argmax(sizes)) + 1
    return c, k, int(sizes.max())


class Refused(ValueError):
    pass


def create_mask(vol, pixel, radius_A, threshold, lowpass_A=0.0, edge_px=EDGE_PX, rebin=0.35, L=None, labeller=None):
    """(mask as uint8, info dict) by the definition; L: the low-passed map if the caller has it already."""
    n = vol.shape[0]
    sph = sphere(n, radius_A, pixel)
    if L is None:
        L = lowpassed(vol, pixel, lowpass_A, edge_px)
    b0 = sph & (L >= float(np.float32(threshold)))
    mn, mx = float(L[sph].min()), float(L[sph].max())
    if not b0.any():
        raise Refused(f"ERROR: create_mask: no voxel inside the outer radius reaches the threshold {threshold:g}: the density there ranges from {mn:g} to {mx:g}")
    c, k, size = largest_body(b0, labeller)
    info = dict(density_min=mn, density_max=mx, above=int(b0.sum()), components=k, largest=size)
    if lowpass_A == 0:
        mask = c
    else:
        s = FM.outside_fft(c.astype(np.float64), pixel, lowpass_A, edge_px)
        mask = sph & (s >= float(np.float32(rebin)))
        info["S"] = s
    info["mask_voxels"] = int(mask.sum())
    info["C"] = c
    return mask.astype(np.uint8), info


# ------------------------------------------------------------------------------------------ thresholds with room on either side
def pick_threshold(values, lo, hi, band):
    """The midpoint of the widest gap between consecutive sorted values inside [lo, hi], and that gap in bands."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    v = v[(v >= lo) & (v <= hi)]
    assert len(v) >= 2, "no two values in the window"
    gaps = np.diff(v)
    i = int(np.argmax(gaps))
    return 0.5 * (v[i] + v[i + 1]), float(gaps[i] / band)


def lowpass_map(n):
    """f64_mask.make_map plus two smaller blobs and a few isolated specks: B0 has several bodies."""
    v = FM.make_map(n).copy()
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float32),) * 3, indexing="ij")
    for (cx, cy, cz), amp, sig in (((0.78 * n, 0.30 * n, 0.70 * n), 2.6, 0.07 * n), ((0.25 * n, 0.28 * n, 0.25 * n), 2.4, 0.06 * n)):
        v += (np.float32(amp) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / np.float32(2 * sig * sig))).astype(np.float32)
    for (sx, sy, sz) in ((0.5, 0.2, 0.8), (0.7, 0.75, 0.3), (0.3, 0.7, 0.7)):
        v[int(sz * n), int(sy * n), int(sx * n)] += np.float32(60.0)
    return v.astype(np.float32)


LOWPASS_PIXEL, LOWPASS_A = 2.0, 12.0


def lowpass_case(n):
    """The low-pass case of box n: dict(vol, pixel, radius_A, lowpass_A, edge, L, t, t_gap, C, S, b, b_gap) - thresholds by pick_threshold:
    t within 5 % of the range around the middle of L's range over the sphere, b within [0.30, 0.40]."""
    vol = lowpass_map(n)
    pixel, lp = LOWPASS_PIXEL, LOWPASS_A
    radius_A = 0.45 * n * pixel
    edge = min(EDGE_PX, 2.0 * n * pixel / lp)
    L = lowpassed(vol, pixel, lp, edge)
    sph = sphere(n, radius_A, pixel)
    mn, mx = L[sph].min(), L[sph].max()
    mid, half = 0.5 * (mn + mx), 0.05 * (mx - mn)
    t, t_gap = pick_threshold(L[sph], mid - half, mid + half, FM.bound_filtered(n, L))
    t = float(np.float32(t))
    c, _, _ = largest_body(sph & (L >= t))
    s = FM.outside_fft(c.astype(np.float64), pixel, lp, edge)
    b, b_gap = pick_threshold(s[sph], 0.30, 0.40, FM.bound_filtered(n, s))
    b = float(np.float32(b))
    return dict(vol=vol, pixel=pixel, radius_A=radius_A, lowpass_A=lp, edge=edge, L=L, t=t, t_gap=t_gap, C=c, S=s, b=b, b_gap=b_gap)


def script_case(n, pixel, radius_A, lowpass_A, threshold, rebin):
    """A map for answers that are given (a script of the fixture: its threshold, and the 0.35 PYP always sends): lowpass_map(n) scaled
    so that the threshold falls into a wide gap of L, tried gap by gap until the low-passed body also keeps two bands from the re-bin
    value.  dict(vol, edge, L, S, t_room, b_room): the rooms are the distances of the nearest voxel to its comparison, in bands."""
    base = lowpass_map(n)
    edge = min(EDGE_PX, 2.0 * n * pixel / lowpass_A)
    sph = sphere(n, radius_A, pixel)
    L0 = lowpassed(base, pixel, lowpass_A, edge)
    v = np.sort(L0[sph])
    mid, half = 0.5 * (v[0] + v[-1]), 0.25 * (v[-1] - v[0])
    v = v[(v >= mid - half) & (v <= mid + half)]
    gaps = np.diff(v)
    t32, b32 = float(np.float32(threshold)), float(np.float32(rebin))
    for i in np.argsort(-gaps)[:100]:
        vol = (base * np.float32(threshold / (0.5 * (v[i] + v[i + 1])))).astype(np.float32)
        L = lowpassed(vol, pixel, lowpass_A, edge)
        t_room = float(np.abs(L[sph] - t32).min() / FM.bound_filtered(n, L))
        if t_room < 2:
            continue
        _, info = create_mask(vol, pixel, radius_A, threshold, lowpass_A, edge, rebin, L=L)
        b_room = float(np.abs(info["S"][sph] - b32).min() / FM.bound_filtered(n, info["S"]))
        if b_room >= 2:
            return dict(vol=vol, edge=edge, L=L, S=info["S"], t_room=t_room, b_room=b_room)
    raise AssertionError("no scale of the map leaves room around both comparisons")


# ------------------------------------------------------------------------------------------ crafted bodies: pure integer logic
BOXES = (8, 31, 64, 65, 130)
CASES = ("equal_bodies", "corner_touch", "opposite_faces", "serpentine", "lattice", "run_merge", "straddle", "outside_sphere", "random", "dense")


def serpentine(n, nz=None):
    """One voxel thick: every second plane holds every second row in full, joined at alternating ends by single voxels; the planes are
    joined by single voxels too.  One body, with a diameter of about a quarter of the box's voxels."""
    nz = n if nz is None else nz
    b = np.zeros((nz, n, n), dtype=bool)
    b[0:nz:2, 0:n:2, :] = True
    for y in range(1, n - 1, 2):                              # rows y - 1 and y + 1 joined at x = n - 1 or x = 0
        b[0:nz:2, y, (n - 1) if (y // 2) % 2 == 0 else 0] = True
    ylast = (n - 1) // 2 * 2                                  # the last full row
    for z in range(1, nz - 1, 2):                             # planes z - 1 and z + 1 joined at the last or the first row
        b[z, ylast if (z // 2) % 2 == 0 else 0, 0] = True
    return b


def crafted(name, n):
    """(map of zeros and ones as float32, outer radius in voxels, what is known by construction: a dict of info fields).  Threshold 0.5,
    pixel size 1, no low-pass."""
    b = np.zeros((n, n, n), dtype=bool)
    radius = 2.0 * n                                          # everything
    known = {}
    if name == "equal_bodies":
        b[1:3, 1:3, 1:3] = True
        b[5:7, 5:7, 5:7] = True
        b[5, 1, 1] = True                                     # and a smaller one between them in index order
        known = dict(above=17, components=3, largest=8, mask_voxels=8, first=(1 * n + 1) * n + 1)
    elif name == "corner_touch":
        b[1:3, 1:3, 1:3] = True
        b[3:5, 3:5, 3:5] = True
        b[6, 6, 1:4] = True
        known = dict(above=19, components=2, largest=16, mask_voxels=16)
    elif name == "opposite_faces":
        b[:, :, 0] = True
        b[:, :, n - 1] = True
        b[:, 0, 1:3] = True                                   # the face x = 0 is the larger by 2 n
        known = dict(above=2 * n * n + 2 * n, components=2, largest=n * n + 2 * n, mask_voxels=n * n + 2 * n)
    elif name == "serpentine":
        b = serpentine(n)
        known = dict(above=int(b.sum()), components=1, largest=int(b.sum()), mask_voxels=int(b.sum()))
    elif name == "lattice":
        b[::2, ::2, ::2] = True
        k = (n + 1) // 2
        known = dict(above=k ** 3, components=k ** 3, largest=1, mask_voxels=1, first=0)
    elif name == "run_merge":
        zc = n // 2
        b[zc, 2, 1:3] = True                                  # two runs of one row ...
        b[zc, 2, 5:7] = True
        b[zc, 1, 3:5] = True                                  # ... joined only through the row above (diagonally)
        b[zc, 5, 0:2] = True                                  # the same through the row below, and through the plane below
        b[zc, 5, 4:6] = True
        b[zc, 6, 2:4] = True
        b[zc + 1, 5, 2:4] = True
        b[1, 1, 1:6] = True
        known = dict(above=6 + 8 + 5, components=3, largest=8, mask_voxels=8)
    elif name == "straddle":
        x0, x1 = (60, min(68, n)) if n > 64 else (max(n - 6, 0), n)
        b[3, 3, x0:x1] = True                                 # over x = 63 | 64 where the row has more than one word
        b[3, 4, max(x0 - 3, 0):x0] = True                     # touches it diagonally from the next row
        b[4, 2, x1 - 1] = True                                # and from the next plane
        b[6, 6, 0:3] = True
        size = (x1 - x0) + (x0 - max(x0 - 3, 0)) + 1
        known = dict(above=size + 3, components=2, largest=size, mask_voxels=size)
    elif name == "outside_sphere":
        radius = n / 4.0
        c = n // 2
        b[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1] = True
        b[0, :, :] = True                                     # n^2 voxels, all outside the sphere
        known = dict(above=8, components=1, largest=8, mask_voxels=8)
    elif name == "random":
        b = np.random.default_rng(n).random((n, n, n)) < 0.09  # near the percolation threshold of 26-connectivity (0.098): bodies of every size and shape
    elif name == "dense":
        b = np.random.default_rng(1000 + n).random((n, n, n)) < 0.35  # far above it: one body through the whole box, runs merging in every way
    else:
        raise KeyError(name)
    return b.astype(np.float32), radius, known
