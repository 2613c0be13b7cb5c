"""tests/test_pose_roundtrip_cpu.py through the HIP library, without the oracle: what ppm_refine_batch (k_states_from_rows ... k_rows_out)
and ppm_csp_refine (csp_write_back) hand back is held to float64 compositions of elementary rotations and to the library's own score
of the returned row.  Same poses, data and bounds as the CPU file; at most 10 particles of box 32 per call.  Run on the GPU box:
pytest -m gpu"""
import numpy as np
import pytest

from test_pose_roundtrip_cpu import (ANG, C, GRID_STEPS, MAT_TOL, N, PX, REFINING, RESCORE_TOL, SHIFT, WINDOWS, check_score_only_pass, csp_cfgs,
                                     csp_data, grid_cfg, grid_data, mat_err, particle_matrix, phantom, pole_data, raw_grid_cfg,
                                     rows_vs_units, score_cfg)

pytestmark = pytest.mark.gpu
TILE_R = 6          # kTileR of pyp_amd/csrc/host_refine.h: the widest window (steps either side) the register kernel takes


@pytest.fixture(scope="module")
def g():
    from pyp_amd import host
    ref = host.Reference(phantom(), 16)
    yield ref
    ref.close()


def test_score_only_pass_returns_the_rotation_it_was_given(g):
    imgs, rows = pole_data()
    out = g.refine(score_cfg(), imgs, rows)
    check_score_only_pass(out, rows, g.refine(score_cfg(), imgs, out))


@pytest.mark.parametrize("window,path", list(zip(WINDOWS, ("tiles", "fft"))))
@pytest.mark.parametrize("step", GRID_STEPS)
def test_grid_hit_on_a_pole_comes_back_as_that_rotation(g, monkeypatch, step, window, path):
    """The +-2 step window goes to the register kernel (k_global), the window of the mask radius to the full-window transform (k_gfft).
    The library picks by the window's half-width in search-grid steps (here of one pixel: band 10 -> a 32-point grid over box 32); the
    run is repeated with the path forced through PPM_GLOBAL_PATH and must come out bit for bit the same, so the kernel named is the one
    that ran."""
    imgs, truth, start = grid_data(step)
    c = raw_grid_cfg(step, window)
    half_width = int(np.ceil((window if window > 0 else c.mask_radius) / PX))
    assert (half_width > TILE_R) == (path == "fft") and half_width <= 32 // 2 - 1
    out = g.refine(c, imgs, start)
    assert g.note() == ""                                    # neither the band nor the window was cut
    monkeypatch.setenv("PPM_GLOBAL_PATH", path)
    forced = g.refine(c, imgs, start)
    monkeypatch.delenv("PPM_GLOBAL_PATH")
    assert np.array_equal(out, forced)
    err = mat_err(out, truth)
    assert err.max() < MAT_TOL, (err, out[:, ANG])
    assert np.array_equal(out[:, SHIFT], np.zeros((len(out), 2)))


@pytest.mark.parametrize("step", GRID_STEPS)
@pytest.mark.parametrize("kw", REFINING, ids=("theta_phi_frozen", "defaults"))
def test_reported_score_is_the_score_of_the_returned_row(g, step, kw):
    """The same kernel (k_local) on both sides; the matrix of the returned row differs from the scored one by < 1e-12 before the cast
    to float."""
    imgs, truth, start = grid_data(step)
    out = g.refine(grid_cfg(step, WINDOWS[0], **kw), imgs, start)
    again = g.refine(score_cfg(), imgs, out)
    gap = np.abs(again[:, C["SCORE"]] - out[:, C["SCORE"]])
    assert gap.max() < RESCORE_TOL, gap
    if kw:
        assert np.isin(out[:, C["THETA"]], (0.0, 180.0)).all(), out[:, ANG]


@pytest.mark.parametrize("rotation", (0, 1), ids=("rotation_frozen", "rotation_refined"))
def test_constrained_refinement_keeps_a_polar_particle(g, rotation):
    """SCORE comes from k_csp_eval, the second look from k_local: two kernels, whose distance the generic particles 2 and 3 of the same
    run measure.  The polar particles 0 and 1 may be that far apart plus the float32 round-off of a score, no more."""
    imgs, rows, parts, tilts = csp_data()
    cfg, frozen, free = csp_cfgs()
    r3, p3, t3 = g.csp_refine(cfg, free if rotation else frozen, imgs, rows, parts, tilts)
    assert np.array_equal(t3, tilts)
    if not rotation:
        unit = np.array([np.abs(particle_matrix(a) - particle_matrix(b)).max() for a, b in zip(p3, parts)])
        assert unit.max() < MAT_TOL, unit
    ru = rows_vs_units(r3, p3, t3)
    assert ru.max() < MAT_TOL, ru
    again = g.refine(score_cfg(), imgs, r3)
    gap = np.abs(again[:, C["SCORE"]] - r3[:, C["SCORE"]])
    polar = r3[:, C["PIND"]] < 2
    control = gap[~polar].max()
    print("csp re-score gap: control %.3g, polar %.3g" % (control, gap[polar].max()))
    # the yardstick itself is sane: test_gpu_csp.py holds k_csp_eval's SCORE to the oracle's within 0.05, test_gpu_parity.py k_local's
    # within 2e-3, and the oracle scores a row it wrote the same again (6e-14)
    assert control < 0.05 + RESCORE_TOL
    assert gap[polar].max() <= control + RESCORE_TOL, (gap[polar], control)
