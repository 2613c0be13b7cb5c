"""The exhaustive particle search of the constrained refinement (CspCfg.search_points; include/ppm.h, ppm_csp_cfg): its plan
(ppm_csp_search_plan), what the ranking stage kept for a particle (ppm_csp_search_candidates), and the enumeration of the grid
restated in numpy - the rule of pyp_amd/csrc/ppm_csp_search.h and unit_apply_delta of ppm_geom.h."""
import ctypes as C

import numpy as np

from . import lib
from .abi import CspSearchInfo

MAX_CANDIDATES = 32


def plan(cfg, csp_cfg):
    """The plan ppm_csp_refine follows for csp_cfg.search_points (pure host): a dict of step (degrees), r_g (Fourier pixels), h_s and
    tol_shift (pixels), n_angle / full_turn per specimen axis, n_shift_axis, n_rot, n_shift, n_candidates, active, shift_grid."""
    info = CspSearchInfo()
    lib.check(lib.load().ppm_csp_search_plan(C.byref(cfg), C.byref(csp_cfg), C.byref(info)))
    return dict(active=bool(info.active), shift_grid=bool(info.shift_grid), step=info.step, r_g=info.r_g, h_s=info.h_s, tol_shift=info.tol_shift,
                n_angle=tuple(info.n_angle), full_turn=tuple(info.full_turn), n_shift_axis=info.n_shift_axis, n_rot=info.n_rot,
                n_shift=info.n_shift, n_candidates=info.n_candidates)


def candidates(ref, unit, max_k=MAX_CANDIDATES):
    """What stage 1 of the last csp_refine on `ref` (host.Reference) kept for particle `unit` (PIND): (rot_index, shift_index, score)
    in rank order, score in SCORE units on the coarse band; empty arrays for a particle that was not searched."""
    rot, sh, sc = np.zeros(max_k, dtype=np.int64), np.zeros(max_k, dtype=np.int64), np.zeros(max_k, dtype=np.float64)
    n = lib.load().ppm_csp_search_candidates(ref.h, int(unit), int(max_k), lib.ptr(rot), lib.ptr(sh), lib.ptr(sc))
    if n < 0:
        raise lib.PpmError(lib.last_error())
    return rot[:n], sh[:n], sc[:n]


def _angle(n, full, step, i):
    return i * (360.0 / n) if full else (i - (n - 1) // 2) * step


def _shift(n, tol, i):
    m = (n - 1) // 2
    return ((i - m) * tol) / m if m else 0.0


def candidate_delta(plan, rot_index, shift_index):
    """Displacement (rotations about the specimen x, y, z axes in degrees, then the 3-D shift in pixels) of a grid point: rotation index
    (ia n_b + ib) n_c + ic, shift index (ix n + iy) n + iz."""
    na, nb, nc = plan["n_angle"]
    rot_index, shift_index = int(rot_index), int(shift_index)
    ic, ib, ia = rot_index % nc, (rot_index // nc) % nb, rot_index // (nc * nb)
    n = plan["n_shift_axis"]
    iz, iy, ix = shift_index % n, (shift_index // n) % n, shift_index // (n * n)
    full, step, tol = plan["full_turn"], plan["step"], plan["tol_shift"]
    return np.array([_angle(na, full[0], step, ia), _angle(nb, full[1], step, ib), _angle(nc, full[2], step, ic),
                     _shift(n, tol, ix), _shift(n, tol, iy), _shift(n, tol, iz)])


def candidate_particles(particles, plan, rot_index, shift_index):
    """The particle table (P, 12) with particle i at grid point (rot_index[i], shift_index[i]) about its pose in `particles`:
    N <- N Rx(a) Ry(b) Rz(c), a zero angle skipped, shift += d (unit_apply_delta); a negative rotation index leaves the particle."""
    from . import synth
    out = np.array(particles, dtype=np.float64, order="C")
    for i in range(len(out)):
        if rot_index[i] < 0:
            continue
        d = candidate_delta(plan, rot_index[i], shift_index[i])
        N = synth.euler_matrix(-out[i, 4], -out[i, 5], -out[i, 6])
        for k in range(3):
            if d[k] != 0.0:
                N = N @ synth.rot_xyz(k, d[k])
        out[i, 4:7] = -synth.angles_from_matrix(N)
        out[i, 1:4] += d[3:6]
    return out
