"""The pose a caller gets back is the pose that was scored, the poles included.

Every path that writes a pose rebuilds (psi, theta, phi) from a rotation matrix with one expression, angles_from_matrix
(pyp_amd/csrc/ppm_geom.h for host and kernels, oracle/ppm_oracle.c, pyp_amd/synth.py).  The oracle tests of the suite compare two
copies of that expression with each other, so they cannot see it go wrong in all copies at once.  Here nothing is compared with another
copy: the returned angles are composed again in float64 from elementary rotations (f64_ref.euler, `rot` below) and held to the
rotation that went in, and the SCORE a row reports is held to the score of that very row scored again.  The poses sit where the
expression branches: both poles exactly, just inside and just outside its sin(theta) <= 1e-7 branch, theta beyond 180, angles outside
[0, 360), and one generic control.

The module constants and the cached data sets are shared with tests/test_gpu_pose_roundtrip.py, which repeats the properties through
the HIP library."""
import functools
import math

import numpy as np
import pytest

import f64_ref
from pyp_amd import sva, synth
from pyp_amd.abi import CSP_PARTICLES, CspCfg, RefineCfg
from pyp_amd.formats import cistem

C = cistem.COL
N, PX = 32, 3.0                      # the smallest supported box; the expression does not depend on the size
POLES = [(12.5, 180, 77), (40, 180, 0), (0, 180, 77), (300, 0, 25), (200, 1e-6, 100),
         (10, 180 - 1e-6, 50), (10, 180 - 1e-5, 50), (33, 190, 20), (-20, 90, 400), (123.4, 56.7, 289.1)]
ANG = [C["PSI"], C["THETA"], C["PHI"]]
SHIFT = [C["X_SHIFT"], C["Y_SHIFT"]]
UNTOUCHED = [0] + list(range(6, 12)) + list(range(15, 32))      # what a refinement without defocus search leaves alone
MAT_TOL = 1e-12              # entries <= 1, a few tens of float64 roundings apart (rot_step is held to 1e-13)
RESCORE_TOL = 2e-3           # SCORE = 100 x cc; 2e-5 on cc is the float32 round-off of a normalised sum (test_gpu_parity.py)
GRID_STEPS = (30.0, 40.0)    # n_psi = 12: psi and psi + 180 share a slice; n_psi = 9: odd, no pairing
WINDOWS = (2 * PX, 0.0)      # search range in Angstrom: +-2 search-grid steps; 0 = the mask radius, +-13 steps


def rot(k, deg):
    """Right-handed rotation about x (0), y (1), z (2), float64."""
    t = math.radians(deg); c, s = math.cos(t), math.sin(t)
    return np.array([[[1, 0, 0], [0, c, -s], [0, s, c]], [[c, 0, s], [0, 1, 0], [-s, 0, c]], [[c, -s, 0], [s, c, 0], [0, 0, 1]]][k], dtype=np.float64)


def euler(a):
    return f64_ref.euler(float(a[0]), float(a[1]), float(a[2]))


def mat_tol(theta):
    """Bound on |euler(returned) - euler(given)| per entry.  Outside the pole branch the angles are exact to rounding.  Inside it
    (sin(theta) <= 1e-7) theta is snapped to the pole: Rz(phi) Ry(theta) Rz(psi) then moves by sin(theta) in M[2], M[5], M[6], M[7] and by
    1 - cos(theta) elsewhere, so sqrt(2) sin(theta) bounds it - at most the 2e-7 = sqrt(2) x the branch's threshold, and 1e-12 at an
    exact pole."""
    s = abs(math.sin(math.radians(theta)))
    return MAT_TOL if s > 1e-7 else MAT_TOL + math.sqrt(2.0) * s


def mat_err(rows_a, rows_b):
    """Largest entry of euler(row a) - euler(row b), per row."""
    return np.array([np.abs(euler(x[ANG]) - euler(y[ANG])).max() for x, y in zip(rows_a, rows_b)])


def particle_matrix(p):
    """N of a particle block line: the stored angles are the negated Euler angles of N."""
    return euler((-p[4], -p[5], -p[6]))


def base_cfg(**kw):
    d = dict(box=N, pixel_size=PX, mask_radius=0.4 * N * PX, res_high=PX * N / 12)
    d.update(kw)
    return RefineCfg.make(**d)


def score_cfg():
    return base_cfg(global_search=0, local_refine=0)


def grid_cfg(step, window, **kw):
    d = dict(res_search=PX * N / 10, angular_step=step, search_range_x=window, search_range_y=window)
    d.update(kw)
    return base_cfg(**d)


def raw_grid_cfg(step, window):
    """Grid search alone: the hits stay at their grid points (iters_hit = -1), nothing continues."""
    return grid_cfg(step, window, iters_hit=-1, local_refine=0)


REFINING = (dict(local_refine=0, refine_theta=0, refine_phi=0), dict())


@functools.lru_cache(maxsize=None)
def phantom():
    return synth.phantom(N)


def _rows(poses, shifts_px):
    rows = cistem.default_rows(len(poses), PX, 300.0, 2.7, 0.07)
    rows[:, ANG] = np.asarray(poses, dtype=np.float64)
    rows[:, SHIFT] = np.asarray(shifts_px, dtype=np.float64) * PX
    rows[:, C["DEFOCUS_1"]] = 15000.0 + 700.0 * np.arange(len(poses))
    rows[:, C["DEFOCUS_2"]] = rows[:, C["DEFOCUS_1"]] - 250.0
    rows[:, C["DEFOCUS_ANGLE"]] = 30.0
    return rows


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pole_data():
    """(images, rows): one noise-free particle per entry of POLES, with sub-pixel shifts."""
    rng = np.random.default_rng(20241)
    rows = _rows(POLES, rng.uniform(-1.5, 1.5, (len(POLES), 2)))
    imgs = synth.render_rows(phantom(), rows, PX, snr=0).numpy()
    return _frozen(imgs, rows)


def grid_truths(step):
    n_psi = int(math.floor(360.0 / step + 0.5))
    dpsi = 360.0 / n_psi
    return [(k * dpsi, th, 0.0) for th in (180.0, 0.0) for k in (1, n_psi // 2 + 1, n_psi - 2)]


@functools.lru_cache(maxsize=None)
def grid_data(step):
    """(images, truth rows, start rows): noise-free particles that sit on the two polar grid points of the search at `step`, no shift;
    the start rows know nothing (all angles 0)."""
    truth = _rows(grid_truths(step), np.zeros((6, 2)))
    imgs = synth.render_rows(phantom(), truth, PX, snr=0).numpy()
    start = truth.copy()
    start[:, ANG] = 0.0
    return _frozen(imgs, truth, start)


@functools.lru_cache(maxsize=None)
def csp_data():
    """(images, rows, particles, tilts) of a tilt series of 4 particles x 5 tilts: particle 0 stored at the south pole, particle 1 at
    the north pole, 2 and 3 generic; every tilt axis 85, tilt 2 untilted, so the rows of particles 0 and 1 in that tilt are polar rows
    themselves.  The rows are checked against the float64 composition before anything uses them."""
    _, _, rows, parts, tilts = synth.make_tilt_series(N, 4, np.arange(-48, 49, 24.0), pixel=PX, snr=0.3, vol=phantom())
    p2, t2 = parts.copy(), tilts.copy()
    p2[0, 4:7] = (-12.5, -180.0, -77.0)
    p2[1, 4:7] = (-40.0, 0.0, -25.0)
    t2[:, 5] = 85.0
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, t2)
    assert rows_vs_units(rows2, p2, t2).max() < MAT_TOL
    imgs = synth.render_rows(phantom(), rows2, PX, snr=0).numpy()
    return _frozen(imgs, rows2, p2, t2)


def rows_vs_units(rows, particles, tilts):
    """Per row: largest entry of euler(row) - N Ry(-tilt) Rz(axis), the latter from the row's particle and tilt lines."""
    pidx = {int(p[0]): i for i, p in enumerate(particles)}
    tidx = {int(t[0]): i for i, t in enumerate(tilts)}
    out = []
    for r in rows:
        p, t = particles[pidx[int(r[C["PIND"]])]], tilts[tidx[int(r[C["TIND"]])]]
        out.append(np.abs(euler(r[ANG]) - particle_matrix(p) @ rot(1, -t[4]) @ rot(2, t[5])).max())
    return np.array(out)


def csp_cfgs():
    """(refine cfg, constrained cfg with the rotation frozen, the same with the rotation refined)."""
    kw = dict(tol_angle=(8, 8, 8), tol_shift=4.0)
    return base_cfg(global_search=0), CspCfg.make(CSP_PARTICLES, refine_rotation=0, **kw), CspCfg.make(CSP_PARTICLES, **kw)


def check_score_only_pass(out, rows, rescored):
    """What a pass that refines nothing must hand back (shared with the GPU test)."""
    err = mat_err(out, rows)
    for e, a in zip(err, POLES):
        assert e <= mat_tol(a[1]), (a, e)
    assert np.abs(out[:, SHIFT] - rows[:, SHIFT]).max() < 1e-9
    assert np.array_equal(out[:, UNTOUCHED], rows[:, UNTOUCHED])
    assert ((out[:, ANG] >= 0) & (out[:, ANG] < 360)).all()
    gap = np.abs(rescored[:, C["SCORE"]] - out[:, C["SCORE"]])
    assert gap.max() < RESCORE_TOL, gap
    # ... and the comparison is not one of zeros: SCORE is 100 x a normalised correlation, near 0 for an image of another pose and in
    # the upper half of the scale for a noise-free image at its own
    assert out[:, C["SCORE"]].min() > 50.0


# ------------------------------------------------------------------------------------------------ host-side algebra
@pytest.mark.parametrize("a", POLES)
def test_synth_angles_compose_to_the_matrix_they_came_from(a):
    M = euler(a)
    r = synth.angles_from_matrix(M)
    assert ((r >= 0) & (r < 360)).all()
    assert np.abs(euler(r) - M).max() <= mat_tol(a[1]), (a, r)
    if abs(math.sin(math.radians(a[1]))) <= 1e-7:       # at a pole everything goes into psi
        assert r[2] == 0.0 and r[1] in (0.0, 180.0)


@pytest.mark.parametrize("a", [(12.5, 180, 77), (0, 180, 77), (300, 0, 25)])
def test_particle_block_of_a_polar_sub_tomogram_pose_gives_the_pose_back(a):
    Nm, p = euler(a), np.array([1.25, -0.5, 2.0])
    q = sva.particle_from_pose(Nm, p)
    assert np.abs(euler(-q[:3]) - Nm).max() < MAT_TOL and np.array_equal(q[3:], p)
    normal = (20.0, -35.0, 110.0)                       # ... and through a table line and back
    N2, p2 = sva.line_to_pose(normal, sva.pose_to_matrix(Nm, p, normal))
    q2 = sva.particle_from_pose(N2, p2)
    assert np.abs(euler(-q2[:3]) - Nm).max() < MAT_TOL and np.abs(q2[3:] - p).max() < 1e-12


# ------------------------------------------------------------------------------------------------ the CPU oracle
@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def oref(O):
    return O.Reference(phantom(), N / 2)


def test_oracle_score_only_pass_returns_the_rotation_it_was_given(O, oref):
    imgs, rows = pole_data()
    out, _ = O.refine_batch(oref, score_cfg(), imgs, rows)
    again, _ = O.refine_batch(oref, score_cfg(), imgs, out)
    check_score_only_pass(out, rows, again)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("step", GRID_STEPS)
def test_oracle_grid_hit_on_a_pole_comes_back_as_that_rotation(O, oref, step, window):
    imgs, truth, start = grid_data(step)
    out, _ = O.refine_batch(oref, raw_grid_cfg(step, window), imgs, start)
    err = mat_err(out, truth)
    assert err.max() < MAT_TOL, (err, out[:, ANG])
    assert np.array_equal(out[:, SHIFT], np.zeros((len(out), 2)))


@pytest.mark.parametrize("step", GRID_STEPS)
@pytest.mark.parametrize("kw", REFINING, ids=("theta_phi_frozen", "defaults"))
def test_oracle_reported_score_is_the_score_of_the_returned_row(O, oref, step, kw):
    """While it refines: the hits are refined (and with the defaults the best continues at the full band).  The truth is not asserted -
    at a band of 12 pixels the refinement drifts by 2 - 3 degrees - only that row and score belong together."""
    imgs, truth, start = grid_data(step)
    out, _ = O.refine_batch(oref, grid_cfg(step, WINDOWS[0], **kw), imgs, start)
    again, _ = O.refine_batch(oref, score_cfg(), imgs, out)
    gap = np.abs(again[:, C["SCORE"]] - out[:, C["SCORE"]])
    assert gap.max() < RESCORE_TOL, gap
    if kw:
        assert np.isin(out[:, C["THETA"]], (0.0, 180.0)).all(), out[:, ANG]


@pytest.mark.parametrize("rotation", (0, 1), ids=("rotation_frozen", "rotation_refined"))
def test_oracle_constrained_refinement_keeps_a_polar_particle(O, oref, rotation):
    imgs, rows, parts, tilts = csp_data()
    cfg, frozen, free = csp_cfgs()
    r3, p3, t3, _ = O.csp_refine(oref, cfg, free if rotation else frozen, imgs, rows, parts, tilts)
    assert np.array_equal(t3, tilts)
    if not rotation:
        unit = np.array([np.abs(particle_matrix(a) - particle_matrix(b)).max() for a, b in zip(p3, parts)])
        assert unit.max() < MAT_TOL, unit
    ru = rows_vs_units(r3, p3, t3)
    assert ru.max() < MAT_TOL, ru
    again, _ = O.refine_batch(oref, score_cfg(), imgs, r3)
    gap = np.abs(again[:, C["SCORE"]] - r3[:, C["SCORE"]])
    assert gap.max() < RESCORE_TOL, gap
