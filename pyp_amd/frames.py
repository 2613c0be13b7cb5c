"""Movie-frame refinement (ppm_frame_refine): the rules around the kernels, stated in numpy.

The library scores every frame row of a particle over a grid of shifts (the row's OWN MAP), pools the maps of the neighbouring frames
of the same particle and tilt and reads one shift per frame off the peak of the pooled map.  This module holds the grid rule
(`plan`, the text of pyp_amd/csrc/ppm_frame_plan.h), the pooling weights (`pool_weights`: mode -2.1's weights of csp_cli.running_average,
taken by FIND distance), the peak rule (`peak`) and their application to a table of rows (`pool_and_peak`), all in float64 - what the
tests hold the kernels to - and the decision of the `csp` executable whether an argv asks for frame refinement at all
(`is_frame_refinement`)."""
import math

import numpy as np

from .formats import cistem

MAX_STEPS = 8           # PPM_FRAME_MAX_STEPS (include/ppm.h)
DEFAULT_STEP = 0.5      # pixels, for step_px = 0


def plan(range_px, step_px=0.0):
    """(h, W, clipped): grid step in pixels, steps either side, whether MAX_STEPS cut the range.  The configuration holds floats; the
    quotient is formed in double from them, as ppm::frame_steps forms it."""
    r, s = np.float32(range_px), np.float32(step_px)
    if not s >= 0:
        raise ValueError("ERROR: frame refinement: step_px must not be negative (0 = half a pixel)")
    if not r > 0:
        raise ValueError("ERROR: frame refinement: range_px must be positive")
    h = s if s > 0 else np.float32(DEFAULT_STEP)
    w = max(int(math.ceil(float(r) / float(h) - 1e-6)), 0)
    return float(h), min(w, MAX_STEPS), w > MAX_STEPS


def grid(h, W):
    """Shifts of the grid points in pixels, (2W + 1, 2W + 1, 2) row-major (jy, jx) -> (dx, dy)."""
    j = np.arange(-W, W + 1, dtype=np.float64) * float(h)
    out = np.empty((2 * W + 1, 2 * W + 1, 2))
    out[..., 0], out[..., 1] = j[None, :], j[:, None]
    return out


def pool_weights(find, half_width):
    """w[i, j] = weight of frame j in the pool of frame i, before the normalisation: exp(-D^2 / (2 (half_width / 2)^2)) of the FIND
    distance D for D <= half_width, else 0; half_width 0: the identity."""
    f = np.asarray(find, dtype=np.int64)
    d = np.abs(f[:, None] - f[None, :]).astype(np.float64)
    if half_width <= 0:
        return (d == 0).astype(np.float64)
    sig = half_width / 2.0
    return np.where(d <= half_width, np.exp(-(d * d) / (2 * sig * sig)), 0.0)


def pool(maps, find, half_width):
    """Pooled maps of one group: maps (F, ...) of the usable frames in ascending FIND -> (F, ...), terms added in ascending FIND."""
    m = np.asarray(maps, dtype=np.float64)
    w = pool_weights(find, half_width)
    out = np.zeros_like(m)
    for j in range(len(m)):
        out += w[:, j].reshape((-1,) + (1,) * (m.ndim - 1)) * m[j][None]
    return out / w.sum(axis=1).reshape((-1,) + (1,) * (m.ndim - 1))


def peak(p, h):
    """Peak of one pooled map p (2W + 1, 2W + 1): (flat arg-max index in row-major (jy, jx) order with ties to the lower index, dx, dy in
    pixels, (curvature x, curvature y)).  Per axis the parabolic offset (l - r) / (2 (l - 2c + r)) h is added where the arg-max is off the
    window's edge and l - 2c + r < 0; a curvature is nan where no offset was taken."""
    p = np.asarray(p, dtype=np.float64)
    side = p.shape[0]
    W = side // 2
    q = int(np.argmax(p.ravel()))
    jy, jx = divmod(q, side)
    d = [(jx - W) * float(h), (jy - W) * float(h)]
    curv = [float("nan"), float("nan")]
    c = p[jy, jx]
    for ax, (j, lo, hi) in enumerate(((jx, (jy, jx - 1), (jy, jx + 1)), (jy, (jy - 1, jx), (jy + 1, jx)))):
        if 0 < j < side - 1:
            l, r = p[lo], p[hi]
            cur = l - 2 * c + r
            if cur < 0:
                d[ax] += 0.5 * (l - r) / cur * float(h)
                curv[ax] = cur
    return q, d[0], d[1], tuple(curv)


def groups(rows):
    """Indices of the rows of every (PIND, TIND) group, ascending FIND: a list of int arrays."""
    C = cistem.COL
    r = np.asarray(rows)
    order = np.lexsort((r[:, C["FIND"]].astype(np.int64), r[:, C["TIND"]].astype(np.int64), r[:, C["PIND"]].astype(np.int64)))
    key = np.stack([r[order, C["PIND"]], r[order, C["TIND"]]], axis=1).astype(np.int64)
    cut = np.flatnonzero(np.any(key[1:] != key[:-1], axis=1)) + 1
    return [g for g in np.split(order, cut) if len(g)]


def pool_and_peak(rows, own_maps, h, half_width, pixel, tind_min=0, tind_max=-1, first=0, last=-1):
    """The rule of ppm_frame_refine applied in float64 to given own maps (M, 2W + 1, 2W + 1), `pixel` in Angstrom: returns a dict with rows_out, pooled (M, side,
    side), index (M,; -1 for rows without a map), delta (M, 2) pixels, curvature (M, 2), refined / scored (M,) booleans."""
    C = cistem.COL
    rows = np.asarray(rows, dtype=np.float64)
    own = np.asarray(own_maps, dtype=np.float64)
    m, side = len(rows), own.shape[1]
    W = side // 2
    out = dict(rows_out=rows.copy(), pooled=np.zeros_like(own), index=np.full(m, -1), delta=np.zeros((m, 2)), curvature=np.full((m, 2), np.nan),
               refined=np.zeros(m, bool), scored=np.zeros(m, bool))
    for g in groups(rows):
        tind = int(rows[g[0], C["TIND"]])
        find = rows[g, C["FIND"]].astype(np.int64)
        if len(np.unique(find)) != len(find):
            raise ValueError("ERROR: frame refinement: a FIND occurs twice in a group")
        if tind < first or (last >= 0 and tind > last):
            continue
        use = g[rows[g, C["OCCUPANCY"]] > 0]
        if len(use) == 0:
            continue
        pooled = pool(own[use], rows[use, C["FIND"]].astype(np.int64), half_width)
        write = tind >= tind_min and (tind_max < 0 or tind <= tind_max)
        for k, j in enumerate(use):
            out["pooled"][j] = pooled[k]
            q, dx, dy, curv = peak(pooled[k], h)
            out["index"][j], out["delta"][j], out["curvature"][j] = q, (dx, dy), curv
            r = out["rows_out"][j]
            if write:
                for c, d in (("X_SHIFT", dx), ("Y_SHIFT", dy), ("FSHIFT_X", dx), ("FSHIFT_Y", dy)):
                    r[C[c]] += d * float(pixel)
                r[C["SCORE"]] = 100.0 * own[j].ravel()[q]
                out["refined"][j] = True
            else:
                r[C["SCORE"]] = 100.0 * own[j, W, W]
                out["scored"][j] = True
    return out


def is_frame_refinement(mode, flag, images, settings):
    """Whether a `csp` argv asks for movie-frame refinement: mode 3 (the caller's 5 is mapped to 3 for the region files of frame refinement,
    src/pyp/align/core.py:1106-1151) with the refine-frames flag "1", a frame list as <images> and csp_frame_refinement true in the
    project's .pyp_config.toml (`settings`: the flat table csp_cli.read_flat_toml returns).  Every other argv keeps its path."""
    try:
        m = float(mode)
    except (TypeError, ValueError):
        return False
    return m == 3 and str(flag) == "1" and str(images).endswith(".txt") and settings.get("csp_frame_refinement") is True
