"""The float64 model of particle extraction (tests/f64_extract.py) against the reference-pinned restatement
(oracle/extract_oracle.py) and against windows the reference's own loop wrote (tests/golden/extract_windows.npz), the conditions
its case table has to meet, and mode -2.1 (csp_cli.running_average) against an explicit formula.  No GPU."""
import math
import os

import numpy as np
import pytest

import f64_extract as X
from oracle import extract_oracle as xo


def _boxes():
    for c in X.CASES:
        for i, b in enumerate(X.model(c.name)):
            yield c, i, b


def test_model_matches_the_restatement_on_every_case_the_reference_accepts():
    """Window bit for bit, the emptiness decision, the normalised box to 1e-13.  Where the reference raises (build-defined classes)
    the restatement raises too, except for a single inside column, which it turns into zeros like a single inside row: its
    `ndim == 2` test after the squeeze is not the reference's (see test_model_matches_windows_written_by_the_reference)."""
    n = {k: 0 for k in ("regular", "one_row") + X.BUILD_DEFINED}
    for c, i, b in _boxes():
        img, (bx, by) = X.image(c.image).astype(np.float64), c.coords[i]
        n[b.klass] += 1
        if b.klass in ("both_ends", "near_gap"):
            with pytest.raises(ValueError):
                xo.window(img, bx, by, c.box, c.cbin)
            continue
        w = xo.window(img, bx, by, c.box, c.cbin)
        if b.klass in ("one_row", "one_column"):
            assert not w.any() and b.inside.any(), (c.name, i)            # pinned so that nobody leans on it
            continue
        assert np.array_equal(w, b.raw), (c.name, i)
        assert xo.is_empty(w) == b.empty, (c.name, i)
        if c.normalize and not b.noisy:
            want = xo.normalize_image(w.copy(), c.radius_px, 1.0, 1)
            assert np.abs(want - b.out).max() <= 1e-13 * max(1.0, np.abs(want).max()), (c.name, i)
    assert all(v > 0 for v in n.values()), n


def test_model_matches_windows_written_by_the_reference(golden_dir):
    """The reference's loop itself, run once per coordinate (tests/golden/gen_extract_golden.py): the model's window is the one it
    wrote, to the float32 it stores, and the model calls build-defined exactly what made it raise.  This is what pins a single
    inside row (placed) and a single inside column (ValueError), where the restatement answers zeros for both."""
    z = np.load(os.path.join(golden_dir, "extract_windows.npz"))
    img = z["image"]
    seen = set()
    for i, (name, box, (bx, by), raised) in enumerate(zip(z["names"], z["boxes"], z["coords"], z["raised"])):
        box = int(box)
        k = X.window_class(X.corner(by, 1.0, box), X.corner(bx, 1.0, box), box, *img.shape)
        seen.add(k)
        assert (k in X.BUILD_DEFINED) == bool(raised), (name, k)
        if not raised:
            raw, inside, fill = X.window(img, bx, by, box, 1.0)
            w = z["win%d" % i]
            assert w.dtype == np.float32 and np.array_equal(w[inside], raw[inside].astype(np.float32)), name
            # the reference reads float32 images and takes their mean in float32 (pairwise sums of at most 50-odd rows of 8-pixel
            # blocks): one value everywhere outside, within 4 float32 ulps of the float64 mean
            if not inside.all():
                assert len(np.unique(w[~inside])) == 1 and abs(float(w[~inside][0]) - fill) <= 4 * X.ulp32(fill), name
            assert str(name).startswith(k) or k == "regular", (name, k)
    assert seen == {"regular", "one_row"} | set(X.BUILD_DEFINED)


def _tags(c):
    return {t for ts in c.tags for t in ts}


def test_the_table_holds_every_class_at_every_box_it_applies_to():
    for box in X.BOXES:
        mine = [c for c in X.CASES if c.box == box and c.image == "base"]
        tags = set().union(*[_tags(c) for c in mine])
        for e in X.EDGE_NAMES:
            assert "rows:" + e in tags and ("cols:" + e in tags or e == "inside"), (box, e)
        assert {"rows:" + e for e in X.EXTRA_NAMES} <= tags and {"cols:" + e for e in X.EXTRA_NAMES} <= tags
        assert {"corner:%s/%s" % p for p in X.CORNERS} <= tags
        assert {len(c.coords) for c in mine} >= {1, 23}
        assert {(c.normalize, c.fix_empty) for c in mine if len(c.coords) == 23} == {(a, b) for a in (True, False) for b in (True, False)}
        want_r = {"radius:zero", "radius:clamped"} | ({"radius:r20", "radius:r25_6"} if box >= 64 else set())
        assert {t for t in tags if t.startswith("radius:")} == want_r, box
    # the edge names mean what they say
    for box in X.BOXES:
        for n in (X.ROWS, X.COLS):
            r = {e: X.edge_corner(e, box, n) for e in X.EDGE_NAMES + X.EXTRA_NAMES}
            assert 0 <= r["inside"] and r["inside"] + box < n - 1
            assert (r["near_1"], r["near_box_m1"], r["out_near"]) == (-1, 1 - box, -box)
            assert [r[e] + box - n for e in ("far_noclip", "far_touch", "far_1", "far_box_m2")] == [-1, 0, 1, box - 2]
            assert r["last"] == n - 1 and r["out_far"] >= n and -n < r["near_gap"] + box < 0 and r["out_near_far"] + box <= -n
    for box in (31, 64):
        got = {(c.cbin, t) for c in X.CASES if c.box == box and c.name.startswith("coords_") for t in _tags(c)}
        assert got >= {(b, "frac:" + f) for b in (1.0, 2.0, 1.5) for f in X.FRACTIONS}
    # floor, not truncation: the negative fractions land one pixel lower than int() would put them
    c = X.BY_NAME["coords_b64_bin1_5"]
    for (bx, by), t in zip(c.coords, c.tags):
        if t[0] in ("frac:neg_half", "frac:neg_001"):
            assert min(X.corner(bx, c.cbin, 64), X.corner(by, c.cbin, 64)) == -1 - 32 and int(min(bx, by) / c.cbin) == 0
    names = {c.name for c in X.CASES}
    assert names >= {"constant", "count_40", "count_41", "count_99", "count_100", "probe_gap", "overlap_36", "overlap_45", "outside",
                     "constant_ring", "high_b64", "high_b192", "small_b64", "small_b100", "layout_offset", "layout_out", "layout_perm"}
    assert sorted(X.PERMUTATION) == list(range(23)) and list(X.PERMUTATION) != list(range(23))
    for c in X.CASES:
        assert len(c.coords) == len(c.tags) and c.box in X.BOXES
    for name in ("small_b64", "small_b100"):
        kl = [b.klass for b in X.model(name)]
        assert kl.count("both_ends") == 4 and kl.count("regular") == 2            # exact fit and far/near are the reference's
        assert X.image("small").shape == (40, 50)


def test_radii_keep_clear_of_integers_and_the_ties_are_the_named_ones():
    for c in X.CASES:
        bg, d2, r2 = X.ring(c.box, c.radius_px)
        if r2 != round(r2):
            assert abs(r2 - round(r2)) >= 1e-3, (c.name, r2)
            assert float(np.float32(r2)) != round(r2)
        assert bool((d2 == r2).any()) == c.radius_tie, (c.name, r2)
    assert 12 * 12 + 16 * 16 == 20 * 20 and not X.ring(64, 20.0)[0][32 + 12, 32 + 16] and not X.ring(64, 20.0)[0][32 + 20, 32]
    assert X.ring(64, 64 / 2.0 + 5.0)[2] == 32.0 ** 2 and X.ring(31, 31 / 2.0 + 5.0)[2] == 15.5 ** 2          # clamped


def _three_probe_rule(raw, inside_fill):
    """k_extract's rule before this table existed: only the values at (0, 0), at the centre and the fill are candidates."""
    n = raw.shape[0]
    most = max(int((raw == v).sum()) for v in (raw[0, 0], raw[n // 2, n // 2], inside_fill))
    return bool(raw.min() == raw.max() or raw.size - most < 0.01 * raw.size)


def test_emptiness_cases_sit_where_they_are_said_to():
    want = dict(constant=True, count_40=True, count_41=False, count_99=True, count_100=False, probe_gap=True, probe_gap_raw=True,
                overlap_36=True, overlap_45=False, outside=True, constant_keep=True)
    for name, empty in want.items():
        live0, b, live1 = X.model(name)
        assert b.empty == empty and not live0.empty and not live1.empty, name
        assert b.noisy == (empty and X.BY_NAME[name].fix_empty)
    assert [X.model(n)[1].differing for n in ("count_40", "count_41", "count_99", "count_100", "overlap_36", "overlap_45")] == [40, 41, 99, 100, 36, 45]
    assert 0.01 * 64 * 64 == 40.96 and 0.01 * 100 * 100 == 100.0
    # the probe gap: empty for the model, not for the three-probe rule; the counting cases are what both rules agree on
    g = X.model("probe_gap")[1]
    assert g.empty and g.differing == 2 and not _three_probe_rule(g.raw, g.fill)
    for name in ("constant", "count_40", "count_41", "count_99", "count_100"):
        b = X.model(name)[1]
        assert _three_probe_rule(b.raw, b.fill) == b.empty, name
    # no case other than the declared ones within 2 pixels of the 1 % count
    for c, i, b in _boxes():
        near = b.raw.min() != b.raw.max() and abs(b.differing - 0.01 * b.raw.size) <= 2.0
        assert near == (i in c.count_tie), (c.name, i, b.differing)
    ring = X.model("constant_ring")[0]
    assert ring.sd == 0.0 and ring.mu == X.DEAD_VALUE and not ring.empty and np.abs(ring.out).max() > 1.0
    assert math.frexp(X.DEAD_VALUE)[0] * 256 == int(math.frexp(X.DEAD_VALUE)[0] * 256)         # at most 8 significant bits


def test_noise_is_unit_white_noise_of_the_box_index():
    a, b = X.noise(0, 64), X.noise(1, 64)
    assert abs(a.mean()) < 0.05 and abs(a.std() - 1.0) < 0.05 and abs((a * b).mean()) < 0.05 and np.abs(a).max() < X.NOISE_SCALE
    assert abs((a[:, 1:] * a[:, :-1]).mean()) < 0.05 and np.array_equal(a, X.noise(0, 64))
    assert np.float32(1.0) / np.float32(16777217.0) == np.float32(2.0 ** -24)
    # two hash values by hand: 32-bit wrap-around arithmetic
    def h(x):
        x ^= x >> 16; x = x * 0x7feb352d % 2 ** 32; x ^= x >> 15; x = x * 0x846ca68b % 2 ** 32; return x ^ (x >> 16)
    for p, i in ((0, 0), (1, 4095), (22, 36863)):
        h1 = h((p * 2654435761 + 2 * i + 1) % 2 ** 32)
        u1, u2 = ((h1 >> 8) + 1) * 2.0 ** -24, (h(h1 ^ 0x9e3779b9) >> 8) * 2.0 ** -24
        box = 64 if i < 4096 else 192
        want = math.sqrt(-2.0 * math.log(u1)) * math.cos(float(np.float32(6.283185307179586) * np.float32(u2)))
        assert X.noise(p, box).ravel()[i] == pytest.approx(want, abs=1e-12)


def test_tolerances_come_from_the_model_and_stay_under_the_suites_bound():
    worst = 0.0
    for c, i, b in _boxes():
        assert b.tol > 0 or (b.tol == 0 and not b.noisy and not b.raw.any()), (c.name, i)      # a kept all-zero window is exact
        if c.normalize and c.image not in ("high", "small") and b.sd > 0:          # the 200 x 260 images of mean 10
            worst = max(worst, b.tol)
            assert b.tol < 2e-5, (c.name, i, b.tol)
    assert 1e-6 < worst < 2e-5
    hi = X.model("high_b64")[1].tol              # over the near edge by one row
    assert 1e-4 < hi < 1e-3                    # 4 * 2^-24 * 3e4 / 30: the rounding of the fill value at this offset
    assert not X.FACTORS or all(f > X.FACTOR and why for f, why in X.FACTORS.values())


def test_running_average_matches_the_formula():
    from pyp_amd.formats import cistem
    from pyp_amd.surface import csp_cli
    C = cistem.COL
    box, radius = 31, 11.3
    img = X.image("base")
    find = [0, 1, 3, 4, 5]                                             # a gap at 2
    rows, stack = [], []
    for pind, (x, y) in enumerate(((60.0, 70.0), (3.0, 150.5))):       # the second particle overhangs the near edge
        for imind in (0, 1):
            for f in find:
                r = np.zeros(cistem.NCOL)
                r[C["PIND"]], r[C["IMIND"]], r[C["FIND"]] = pind, imind, f
                rows.append(r)
                stack.append(X.model_box(img, x + 0.3 * f + 7 * imind, y - 0.2 * f, box, 1.0, radius, True, True, 0).out)
    order = np.random.default_rng(4).permutation(len(rows))            # rows need not come sorted
    rows, stack = np.array(rows)[order], np.array(stack)[order].astype(np.float32)
    for hw in (1, 2, 3):
        want = X.running_average_formula(stack, rows[:, C["PIND"]], rows[:, C["IMIND"]], rows[:, C["FIND"]], hw, radius)
        got = csp_cli.running_average(stack, rows, hw, radius)
        assert got.dtype == np.float32 and np.abs(got - want).max() < 4 * X.EPS32 * np.abs(want).max(), hw
        # the gap shows: frame 1 at half-width 1 averages frames 0 and 1 only, frame 3 frames 3 and 4
        j = int(np.where((rows[:, C["PIND"]] == 0) & (rows[:, C["IMIND"]] == 0) & (rows[:, C["FIND"]] == 3))[0][0])
        assert np.abs(got[j] - stack[j]).max() > 0.05
    assert csp_cli.running_average(stack, rows, 0, radius) is stack
