"""Float64 statement of particle extraction (ppm_extract_boxes / k_extract) pixel by pixel, and the table of cases
that tests/test_extract_model_cpu.py checks against the reference-pinned restatement (oracle/extract_oracle.py) and
tests/test_gpu_extract.py holds the GPU to.  numpy only: no torch, no GPU.

  window   box pixel (r, c) looks at image pixel (R0 + r, C0 + c), R0 = floor(by / cbin) - box // 2, C0 likewise from bx.  Per axis
           of n image pixels the pixel is "inside" when
               R0 < 0            : 0 <= R0 + r < n                   (near-edge clip)
               R0 + box >= n     : R0 + r < n - 1                    (far-edge clip; the reference drops the last row / column)
               otherwise         : always
           and a box pixel is inside when it is on both axes.  Inside pixels are copied; the others hold the float64 mean of the
           inside pixels, or 0 when there are none.
  empty    min == max, or fewer than 1 % of the pixels differ from the median.
  noise    an empty window (with fix_empty) becomes the project's own unit noise of (index of the box within the call, pixel).
  normal.  (x - mean) / std over the pixels whose integer distance^2 from (box // 2, box // 2) exceeds radius_px^2 (radius_px at
           most box / 2); two-pass mean and std; divided only when std > 0.

Where the reference itself raises there is nothing to follow and the rule above is build-defined (`build_defined`):
  both_ends   R0 < 0 and R0 + box > n: every image row of the axis is used, no far-edge drop;
  near_gap    -n < R0 + box < 0: the reference's slice end goes negative and counts from the far edge; here nothing is inside;
  one_column  exactly one inside column (any number of rows): the reference squeezes the column to a vector and cannot place it.
A window with exactly one inside ROW and at least two columns is placed by the reference like any other (class `one_row`); the
restatement in oracle/extract_oracle.py returns zeros for it (its `ndim == 2` test), so that class is pinned by windows the
reference's own function produced (tests/golden/extract_windows.npz) and not by the restatement.
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

EPS32 = 2.0 ** -24
FACTOR = 4.0                                  # the tolerance factor of every case; a case that needs more says so in FACTORS
FACTORS = {}                                  # case name -> (factor, reason)
NOISE_SCALE = 8.0                             # |noise| <= sqrt(2 ln 2^24) = 5.77 < 8
BOXES = (8, 31, 64, 100, 192)
ROWS, COLS = 200, 260
DEAD = (slice(20, 130), slice(40, 150))       # the 7.0-valued block of the `dead` images
DEAD_VALUE = 7.0
EMPTY_AT = {64: (30, 50), 100: (25, 45)}      # (R0, C0) of the emptiness windows, inside the dead block
LIVE_AT = (60, 180)                           # (R0, C0) of a box <= 64 window on live pixels of the `dead` images


# ------------------------------------------------------------------------------------------------ the model
def corner(b, cbin, box):
    return math.floor(b / cbin) - box // 2


def axis_inside(r0, box, n):
    src = r0 + np.arange(box)
    if r0 < 0:
        return (src >= 0) & (src < n)
    if r0 + box >= n:
        return src < n - 1
    return np.ones(box, dtype=bool)


def axis_class(r0, box, n):
    if r0 < 0 and r0 + box > n:
        return "both_ends"
    if -n < r0 + box < 0:
        return "near_gap"
    return "regular"


def window_class(r0, c0, box, rows, cols):
    """regular | one_row | both_ends | near_gap | one_column (the last three: the reference raises, build-defined here)."""
    for k in (axis_class(r0, box, rows), axis_class(c0, box, cols)):
        if k != "regular":
            return k
    nr, nc = int(axis_inside(r0, box, rows).sum()), int(axis_inside(c0, box, cols).sum())
    if nc == 1 and nr >= 1:
        return "one_column"
    if nr == 1 and nc >= 2:
        return "one_row"
    return "regular"


BUILD_DEFINED = ("both_ends", "near_gap", "one_column")


def window(img, bx, by, box, cbin):
    """(raw float64 [box, box], inside mask, fill) by the per-pixel rule."""
    rows, cols = img.shape
    r0, c0 = corner(by, cbin, box), corner(bx, cbin, box)
    okr, okc = axis_inside(r0, box, rows), axis_inside(c0, box, cols)
    inside = np.outer(okr, okc)
    raw = np.zeros((box, box))
    if not inside.any():
        return raw, inside, 0.0
    rr, cc = np.nonzero(inside)
    vals = img[r0 + rr, c0 + cc].astype(np.float64)
    fill = math.fsum(vals) / len(vals)
    raw[:] = fill
    raw[rr, cc] = vals
    return raw, inside, fill


def differing(raw):
    return int((raw != np.median(raw)).sum())


def is_empty(raw):
    return bool(raw.min() == raw.max() or differing(raw) < raw.size * 0.01)


def hash32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def noise(p, box):
    """Unit noise of box `p` of a call: hash32 twice, two uniforms, Box-Muller.  The uniforms and the angle are float32 values by
    definition (u1 = (k + 1) 2^-24: the divisor 16777217 is 2^24 as a float; the angle is the float32 product); from there float64."""
    i = np.arange(box * box, dtype=np.uint32)
    h1 = hash32(np.full(box * box, p, dtype=np.uint32) * np.uint32(2654435761) + i * np.uint32(2) + np.uint32(1))
    h2 = hash32(h1 ^ np.uint32(0x9e3779b9))
    u1 = ((h1 >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * (np.float32(1.0) / np.float32(16777217.0))
    u2 = (h2 >> np.uint32(8)).astype(np.float32) * (np.float32(1.0) / np.float32(16777216.0))
    ang = np.float32(6.283185307179586) * u2
    assert u1.dtype == np.float32 and ang.dtype == np.float32
    v = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(ang.astype(np.float64))
    return v.reshape(box, box)


def ring(box, radius_px):
    radius_px = min(float(radius_px), box / 2.0)
    d = np.arange(box) - box // 2
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    return d2 > radius_px * radius_px, d2, radius_px * radius_px


def ring_stats(x, box, radius_px):
    bg = x[ring(box, radius_px)[0]]
    if bg.size == 0:
        return 0.0, 0.0
    mu = math.fsum(bg) / bg.size
    return mu, math.sqrt(math.fsum((bg - mu) ** 2) / bg.size)


Box = namedtuple("Box", "klass raw inside fill empty differing noisy value mu sd out tol")


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


def model_box(img, bx, by, box, cbin, radius_px, normalize, fix_empty, index, factor=FACTOR):
    """One box of a call.  `out` is the float64 result; `tol` the bound on |float32 result - out| where a bound applies
    (normalize off and not noise: `compare` asks for the bits of the inside pixels and one float32 ulp on the fill)."""
    rows, cols = img.shape
    klass = window_class(corner(by, cbin, box), corner(bx, cbin, box), box, rows, cols)
    raw, inside, fill = window(img, bx, by, box, cbin)
    empty = is_empty(raw)
    noisy = bool(empty and fix_empty)
    value = noise(index, box) if noisy else raw
    mu, sd = ring_stats(value, box, radius_px) if normalize else (0.0, 0.0)
    out = value - mu
    if sd > 0:
        out = out / sd
    scale = sd if sd > 0 else 1.0
    if noisy:      # the noise itself to factor * 2^-24 * 8, then (normalize) the rounding of the stored result
        tol = factor * EPS32 * (NOISE_SCALE + (np.abs(value - mu).max() if normalize else 0.0)) / scale
    elif normalize:
        tol = factor * EPS32 * (np.abs(raw - mu).max() + abs(fill)) / scale
    else:
        tol = ulp32(fill)
    return Box(klass, raw, inside, fill, empty, differing(raw), noisy, value, mu, sd, out, float(tol))


def compare(got, b, normalize):
    """(worst error, its bound) of a float32 result against the model's box; an inside pixel with other bits (normalize off) is inf."""
    got = np.asarray(got, dtype=np.float64)
    if b.noisy or normalize:
        return float(np.abs(got - b.out).max()), b.tol
    err = 0.0
    if b.inside.any() and not np.array_equal(got[b.inside], b.raw[b.inside]):
        err = math.inf
    if (~b.inside).any():
        err = max(err, float(np.abs(got[~b.inside] - float(np.float32(b.fill))).max()))
    return err, b.tol


# ------------------------------------------------------------------------------------------------ the images
_BUILDERS = {}


def _base():
    return np.random.default_rng(20261).normal(10.0, 3.0, (ROWS, COLS)).astype(np.float32)


def _dead(hot=()):
    """The base image with the dead block; `hot` = (row, column, value) pixels set afterwards."""
    a = _base()
    a[DEAD] = DEAD_VALUE
    for r, c, v in hot:
        a[r, c] = v
    return a


def _hot(box, k):
    """k pixels of the emptiness window of `box`, all different values, none at the window's (0, 0) or centre."""
    r0, c0 = EMPTY_AT[box]
    idx = (np.arange(k) * 97 + 5) % (box * box)
    assert len(set(idx)) == k and 0 not in idx and (box // 2) * box + box // 2 not in idx
    return [(r0 + int(i) // box, c0 + int(i) % box, 9.0 + 0.25 * j) for j, i in enumerate(idx)]


def _ring_image():
    """The emptiness window of box 64 with live pixels inside distance^2 <= 300 of its centre: radius 20 leaves a constant ring."""
    a, live = _dead(), _base()
    r0, c0 = EMPTY_AT[64]
    d = np.arange(64) - 32
    disc = d[:, None] ** 2 + d[None, :] ** 2 <= 300
    a[r0:r0 + 64, c0:c0 + 64][disc] = live[r0:r0 + 64, c0:c0 + 64][disc]
    return a


_BUILDERS.update(
    base=_base,
    high=lambda: np.random.default_rng(20262).normal(3.0e4, 30.0, (ROWS, COLS)).astype(np.float32),
    small=lambda: np.random.default_rng(20263).normal(10.0, 3.0, (40, 50)).astype(np.float32),
    dead=_dead,
    dead_40=lambda: _dead(_hot(64, 40)), dead_41=lambda: _dead(_hot(64, 41)),
    dead_99=lambda: _dead(_hot(100, 99)), dead_100=lambda: _dead(_hot(100, 100)),
    probe_gap=lambda: _dead([(EMPTY_AT[64][0], EMPTY_AT[64][1], 9.0), (EMPTY_AT[64][0] + 32, EMPTY_AT[64][1] + 32, 9.0)]),
    ring=_ring_image)


@lru_cache(maxsize=None)
def image(name):
    a = _BUILDERS[name]()
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "name image box coords tags cbin radius_px normalize fix_empty layout radius_tie count_tie")
EDGE_NAMES = ("inside", "near_1", "near_box_m1", "out_near", "far_noclip", "far_touch", "far_1", "far_box_m2", "last", "out_far")
EXTRA_NAMES = ("near_gap", "out_near_far")
CORNERS = (("near_1", "near_1"), ("near_1", "far_1"), ("far_touch", "near_1"), ("far_1", "far_touch"))
FRACTIONS = ("int", "half", "999", "neg_half", "neg_001")
RADIUS_NAMES = ("zero", "r20", "r25_6", "clamped")


def edge_corner(name, box, n):
    """R0 of an edge position along an axis of n pixels."""
    return {"inside": (n - box) // 2, "near_1": -1, "near_box_m1": -(box - 1), "out_near": -box, "far_noclip": n - 1 - box,
            "far_touch": n - box, "far_1": n + 1 - box, "far_box_m2": n - 2, "last": n - 1, "out_far": n + 3,
            "near_gap": -box - 5, "out_near_far": -box - n - 3}[name]


def default_radius(box):
    return 0.385 * box


def _at(r0, c0, box, cbin=1.0):
    """The integer coordinate (bx, by) whose window starts at (r0, c0)."""
    return ((c0 + box // 2) * cbin, (r0 + box // 2) * cbin)


def edge_coords(box, rows=ROWS, cols=COLS, names=EDGE_NAMES):
    """The 23: every edge position on the rows with the columns inside, on the columns with the rows inside, four corners."""
    rin, cin = edge_corner("inside", box, rows), edge_corner("inside", box, cols)
    coords, tags = [], []
    for e in names:
        coords.append(_at(edge_corner(e, box, rows), cin, box)); tags.append(("rows:" + e,) + (("cols:inside",) if e == "inside" else ()))
    for e in names:
        if e != "inside":
            coords.append(_at(rin, edge_corner(e, box, cols), box)); tags.append(("cols:" + e,))
    if names is EDGE_NAMES:
        for er, ec in CORNERS:
            coords.append(_at(edge_corner(er, box, rows), edge_corner(ec, box, cols), box)); tags.append(("corner:%s/%s" % (er, ec),))
    return tuple(coords), tuple(tags)


def _case(name, image_, box, coords, tags, cbin=1.0, radius_px=None, normalize=True, fix_empty=True, layout="host", radius_tie=False,
          count_tie=()):
    return Case(name, image_, box, tuple((float(x), float(y)) for x, y in coords), tuple(tags), float(cbin),
                float(default_radius(box) if radius_px is None else radius_px), bool(normalize), bool(fix_empty), layout, radius_tie,
                tuple(count_tie))


def _sliver_ties(box, tags):
    """Box 100 only: a one-row or one-column overlap is 100 pixels of 10000, the strict 1 % count itself."""
    if box != 100:
        return ()
    return tuple(i for i, t in enumerate(tags) if t[0].endswith(("near_box_m1", "far_box_m2")) and not t[0].startswith("corner"))


def _build_cases():
    out = []
    for box in BOXES:
        coords, tags = edge_coords(box)
        assert len(coords) == 23
        for nrm in (True, False):
            for fix in (True, False):
                out.append(_case("edges_b%d_n%de%d" % (box, nrm, fix), "base", box, coords, tags, normalize=nrm, fix_empty=fix,
                                 count_tie=_sliver_ties(box, tags)))
        xc, xt = edge_coords(box, names=EXTRA_NAMES)
        out.append(_case("extras_b%d" % box, "base", box, xc, xt))
        for pos in ("inside", "near_1"):                               # m = 1
            out.append(_case("single_b%d_%s" % (box, pos), "base", box, [_at(edge_corner(pos, box, ROWS), edge_corner(pos, box, COLS), box)],
                             [("single:" + pos,)]))
        three = [_at(edge_corner("inside", box, ROWS), edge_corner("inside", box, COLS), box), _at(-1, -1, box),
                 _at(edge_corner("far_1", box, ROWS), edge_corner("inside", box, COLS), box)]
        for rn in RADIUS_NAMES:
            if rn in ("r20", "r25_6") and box < 64:
                continue
            r = {"zero": 0.0, "r20": 20.0, "r25_6": 25.6, "clamped": box / 2.0 + 5.0}[rn]
            tie = rn in ("zero", "r20") or (rn == "clamped" and box % 2 == 0)
            out.append(_case("radius_b%d_%s" % (box, rn), "base", box, three, [("radius:" + rn,)] * 3, radius_px=r, radius_tie=tie))
    # coordinates: fractions that separate floor from truncation, under three binnings; the last two are not multiples of the binning
    for box in (31, 64):
        for cbin in (1.0, 2.0, 1.5):
            u = [(100.0, 90.0, "int"), (100.5, 90.5, "half"), (100.999, 90.999, "999"), (-0.5, 90.0, "neg_half"), (100.0, -0.001, "neg_001"),
                 (-0.001, -0.5, "neg_001"), (0.5, 0.999, "half")]
            coords = [(x * cbin, y * cbin) for x, y, _ in u] + [(101.0, 91.0), (100.0, 137.0)]
            tags = [("frac:" + t,) for _, _, t in u] + [("frac:raw",), ("frac:raw",)]
            out.append(_case("coords_b%d_bin%s" % (box, str(cbin).replace(".", "_")), "base", box, coords, tags, cbin=cbin))
    # emptiness, each between two live windows so that the noise is that of index 1
    live = _at(LIVE_AT[0], LIVE_AT[1], 64)

    def empt(name, image_, box, at, tie=False, **kw):
        lv = live if box <= 64 else _at(edge_corner("inside", box, ROWS), 155, box)
        out.append(_case(name, image_, box, [lv, at, lv], [("live",), ("empty:" + name,), ("live",)], count_tie=(1,) if tie else (), **kw))

    e64, e100 = _at(*EMPTY_AT[64], 64), _at(*EMPTY_AT[100], 100)
    empt("constant", "dead", 64, e64)
    empt("count_40", "dead_40", 64, e64, tie=True)
    empt("count_41", "dead_41", 64, e64, tie=True)
    empt("count_99", "dead_99", 100, e100, tie=True)
    empt("count_100", "dead_100", 100, e100, tie=True)
    empt("probe_gap", "probe_gap", 64, e64)
    empt("probe_gap_raw", "probe_gap", 64, e64, normalize=False)
    empt("overlap_36", "base", 64, _at(-60, -55, 64))                  # 4 x 9 pixels of the image
    empt("overlap_45", "base", 64, _at(-59, -55, 64))                  # 5 x 9
    empt("outside", "base", 64, _at(ROWS + 10, 40, 64))
    empt("constant_keep", "dead", 64, e64, fix_empty=False)            # flags: an empty window that is kept
    out.append(_case("constant_ring", "ring", 64, [e64], [("ring:constant",)], radius_px=20.0, radius_tie=True))
    # one-pass variance against two-pass: a large offset
    for box in (64, 192):
        coords, tags = edge_coords(box)
        out.append(_case("high_b%d" % box, "high", box, coords, tags))
    # boxes larger than the image: (R0, C0) pairs
    for box, rws, cls in ((64, dict(both=-10, exact=-24, near=-30, far=5), dict(both=-6, exact=-14, near=-20, far=7)),
                          (100, dict(both=-25, exact=-60, near=-70, far=5), dict(both=-20, exact=-50, near=-60, far=7))):
        pairs = (("both", "near"), ("far", "both"), ("both", "both"), ("exact", "exact"), ("far", "near"), ("exact", "both"))
        out.append(_case("small_b%d" % box, "small", box, [_at(rws[a], cls[b], box) for a, b in pairs], [("small:%s/%s" % p,) for p in pairs]))
    # layouts
    coords, tags = edge_coords(64)
    for lay in ("offset", "out", "perm"):
        out.append(_case("layout_" + lay, "base", 64, coords, tags, layout=lay))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
PERMUTATION = tuple(int(i) for i in np.random.default_rng(23).permutation(23))


@lru_cache(maxsize=None)
def model(name):
    """The model's boxes of a case (computed once, shared by the tests; treat as read-only)."""
    c = BY_NAME[name]
    f = FACTORS.get(name, (FACTOR, ""))[0]
    return tuple(model_box(image(c.image), bx, by, c.box, c.cbin, c.radius_px, c.normalize, c.fix_empty, i, f) for i, (bx, by) in enumerate(c.coords))


# ------------------------------------------------------------------------------------------------ mode -2.1
def running_average_formula(stack, pind, imind, find, half_width, radius_px):
    """Mode -2.1 in float64: row j becomes sum_k w_k stack[k] / sum_k w_k over the rows k of the same particle and movie with
    |FIND_k - FIND_j| <= half_width, w_k = exp(-d^2 / (2 (half_width / 2)^2)); then the ring normalisation."""
    stack = np.asarray(stack, dtype=np.float64)
    box = stack.shape[1]
    out = np.empty_like(stack)
    for j in range(len(stack)):
        acc, wsum = np.zeros((box, box)), 0.0
        for k in range(len(stack)):
            d = float(find[k] - find[j])
            if pind[k] == pind[j] and imind[k] == imind[j] and abs(d) <= half_width:
                w = math.exp(-d * d / (2.0 * (half_width / 2.0) ** 2))
                acc += w * stack[k]; wsum += w
        avg = acc / wsum
        mu, sd = ring_stats(avg, box, radius_px)
        out[j] = (avg - mu) / (sd if sd > 0 else 1.0)
    return out
