"""Constrained tilt-series refinement on the GPU (ppm_csp_refine, bin/csp) against the CPU oracle on the same synthetic tilt
series.  Tolerances: BASELINE.json's 0.1 deg / 0.5 px on the unit parameters and on the rows that follow from them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import CSP_MICROGRAPHS, CSP_PARTICLES, CspCfg, RefineCfg
from pyp_amd.formats import cistem, mrc
from test_csp_cpu import _particle_angle_err, _perturb_particles, defocus_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


@pytest.fixture(scope="module")
def series():
    from oracle import oracle
    from pyp_amd import host
    n, px = 64, 2.0
    vol, stack, rows, parts, tilts = synth.make_tilt_series(n, 8, np.arange(-54, 55, 12.0), pixel=px, snr=0.3)
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 24, res_signed_cc=30.0, global_search=0)
    return n, px, vol, stack.numpy(), rows, parts, tilts, cfg, host.Reference(vol, n / 2), oracle.Reference(vol, n / 2), oracle


def test_particle_mode_matches_oracle(series):
    n, px, vol, imgs, rows, parts, tilts, cfg, g, o, O = series
    p2 = _perturb_particles(parts)
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, tilts)
    for kw in (dict(), dict(refine_translation=0), dict(refine_rotation=0), dict(first=2, last=5), dict(tind_min=1, tind_max=7)):
        cc = CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0, **kw)
        wr, wp, wt, _ = O.csp_refine(o, cfg, cc, imgs, rows2, p2, tilts)
        gr, gp, gt = g.csp_refine(cfg, cc, imgs, rows2, p2, tilts)
        assert _particle_angle_err(wp, gp).max() < 0.1 and np.abs(wp[:, 1:4] - gp[:, 1:4]).max() < 0.5, kw
        assert synth.angular_error_deg(wr, gr).max() < 0.1 and synth.shift_error_px(wr, gr, px).max() < 0.5, kw
        assert np.abs(wr[:, 14] - gr[:, 14]).max() < 0.05 and np.abs(wp[:, 10] - gp[:, 10]).max() < 0.05, kw
        assert np.array_equal(gt, tilts)
    # and it did refine: closer to the truth than the start
    cc = CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0)
    gr, gp, _ = g.csp_refine(cfg, cc, imgs, rows2, p2, tilts)
    assert _particle_angle_err(gp, parts).mean() < 0.4 * _particle_angle_err(p2, parts).mean()
    assert np.linalg.norm(gp[:, 1:4] - parts[:, 1:4], axis=1).max() < 0.35
    assert np.array_equal(gr, g.csp_refine(cfg, cc, imgs, rows2, p2, tilts)[0])            # deterministic


def test_tap_address_tables_and_arithmetic_agree_in_the_constrained_search(series, monkeypatch):
    """k_csp_eval takes its tap addresses from LDS tables like k_local (ppm_dev.h); PPM_LOCAL_TABLES=0 selects the instantiation that
    computes them per gather.  Same taps, fractions equal to the last bit but one: units and rows agree far inside the tolerance."""
    n, px, vol, imgs, rows, parts, tilts, cfg, g, o, O = series
    p2 = _perturb_particles(parts)
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, tilts)
    cc = CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0)
    tr, tp, _ = g.csp_refine(cfg, cc, imgs, rows2, p2, tilts)
    monkeypatch.setenv("PPM_LOCAL_TABLES", "0")
    ar, ap, _ = g.csp_refine(cfg, cc, imgs, rows2, p2, tilts)
    monkeypatch.delenv("PPM_LOCAL_TABLES")
    assert _particle_angle_err(tp, ap).max() < 0.01 and np.abs(tp[:, 1:4] - ap[:, 1:4]).max() < 0.01
    assert synth.angular_error_deg(tr, ar).max() < 0.01 and synth.shift_error_px(tr, ar, px).max() < 0.01


def test_micrograph_mode_matches_oracle(series):
    n, px, vol, imgs, rows, parts, tilts, cfg, g, o, O = series
    rng = np.random.default_rng(5)
    t2 = tilts.copy()
    t2[:, 4] += rng.normal(0, 0.8, len(t2)); t2[:, 5] += rng.normal(0, 0.6, len(t2)); t2[:, 2:4] += rng.normal(0, 1.0, (len(t2), 2))
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, parts, t2)
    for kw in (dict(), dict(refine_rotation=0), dict(first=3, last=6)):
        cm = CspCfg.make(CSP_MICROGRAPHS, tol_angle=(3, 3, 0), tol_shift=4.0, **kw)
        wr, wp, wt, _ = O.csp_refine(o, cfg, cm, imgs, rows2, parts, t2)
        gr, gp, gt = g.csp_refine(cfg, cm, imgs, rows2, parts, t2)
        assert np.abs(wt[:, 4:6] - gt[:, 4:6]).max() < 0.1 and np.abs(wt[:, 2:4] - gt[:, 2:4]).max() < 0.5, kw
        assert synth.angular_error_deg(wr, gr).max() < 0.1 and synth.shift_error_px(wr, gr, px).max() < 0.5, kw
        assert np.abs(wr[:, 14] - gr[:, 14]).max() < 0.05
        assert np.array_equal(gp[:, :10], parts[:, :10])
    cm = CspCfg.make(CSP_MICROGRAPHS, refine_rotation=0, tol_shift=4.0)
    _, _, gt = g.csp_refine(cfg, cm, imgs, rows2, parts, t2)
    t_ref = tilts.copy(); t_ref[:, 4:6] = t2[:, 4:6]
    assert np.linalg.norm(gt[:, 2:4] - tilts[:, 2:4], axis=1).mean() < 0.5 * np.linalg.norm(t2[:, 2:4] - tilts[:, 2:4], axis=1).mean()


def test_defocus_mode_matches_oracle(series):
    """csp mode 4 (per-tilt defocus offset): same offsets as the oracle, scores to float round-off."""
    from pyp_amd import host
    O = series[-1]
    n, px, vol, imgs, rows, parts, tilts, cfg = defocus_series()
    g, o = host.Reference(vol, n / 2), O.Reference(vol, n / 2)
    off = np.linspace(-350.0, 350.0, len(tilts)).round(-1)
    rows2 = rows.copy()
    for t in range(len(tilts)):
        rows2[rows2[:, 27] == t, 6:8] -= off[t]
    for kw in (dict(), dict(first=2, last=6), dict(tind_min=1, tind_max=5)):
        cc = CspCfg.make(CSP_MICROGRAPHS, refine_defocus=1, defocus_range=400.0, defocus_step=50.0, **kw)
        wr, wp, wt, _ = O.csp_refine(o, cfg, cc, imgs, rows2, parts, tilts)
        gr, gp, gt = g.csp_refine(cfg, cc, imgs, rows2, parts, tilts)
        assert np.array_equal(gr[:, 6:8], wr[:, 6:8]), kw                       # the same offset for every tilt
        assert np.abs(gr[:, 14] - wr[:, 14]).max() < 0.02 and np.array_equal(gr[:, 1:6], wr[:, 1:6])
        assert np.array_equal(gp, parts) and np.array_equal(gt, tilts)
    found = np.array([(gr[gr[:, 27] == t, 6] - rows2[rows2[:, 27] == t, 6]).mean() for t in range(1, 6)])
    assert np.abs(found - off[1:6]).max() <= 25.0           # the nearest 50 A grid point


@pytest.mark.parametrize("rng_,off", [(1000.0, [-1000, -600, -250, 0, 600, 800, 1000]), (850.0, [-850, -500, -200, 0, 750, 800, 850])],
                         ids=["1000/50", "850/50"])
def test_defocus_mode_over_the_whole_ladder(series, rng_, off):
    """csp mode 4 at nt = 20 (T = 41, the cap) and nt = 17 (T = 35): the tilts start at offsets that span the ladder, so the
    winners include t = 0, T - 1 and indices >= 32, the second trip of k_defocus's final reduction (all_scores path).  Assertions
    of test_defocus_mode_matches_oracle."""
    from pyp_amd import host
    import defocus_cases as D
    O = series[-1]
    n, px, vol, imgs, rows, parts, tilts, cfg = defocus_series()
    g, o = host.Reference(vol, n / 2), O.Reference(vol, n / 2)
    off = np.array(off, dtype=np.float64)
    nt = D.csp_steps(rng_, 50.0)
    assert D.plan(nt, O.band_dims(cfg)["B"] + 2) == (2 * nt + 1, 2 * nt + 1, 1, 2)          # one chunk, two trips of the reduction
    rows2 = rows.copy()
    for t in range(len(tilts)):
        rows2[rows2[:, 27] == t, 6:8] -= off[t]
    cc = CspCfg.make(CSP_MICROGRAPHS, refine_defocus=1, defocus_range=rng_, defocus_step=50.0)
    wr, wp, wt, _ = O.csp_refine(o, cfg, cc, imgs, rows2, parts, tilts)
    won = {int(round((wr[wr[:, 27] == t, 6] - rows2[rows2[:, 27] == t, 6]).mean() / 50.0)) + nt for t in range(len(tilts))}
    assert {0, nt, 2 * nt} <= won and sum(t >= 32 for t in won) >= 3                         # the oracle's winners span the ladder
    gr, gp, gt = g.csp_refine(cfg, cc, imgs, rows2, parts, tilts)
    assert np.array_equal(gr[:, 6:8], wr[:, 6:8])                                            # the same offset for every tilt
    assert np.abs(gr[:, 14] - wr[:, 14]).max() < 0.02 and np.array_equal(gr[:, 1:6], wr[:, 1:6])
    assert np.array_equal(gp, parts) and np.array_equal(gt, tilts)


def test_csp_errors_are_loud(series):
    from pyp_amd import lib
    n, px, vol, imgs, rows, parts, tilts, cfg, g, o, O = series
    bad = rows.copy(); bad[3, 26] = 999
    with pytest.raises(lib.PpmError, match="ERROR"):
        g.csp_refine(cfg, CspCfg.make(CSP_PARTICLES), imgs, bad, parts, tilts)
    with pytest.raises(lib.PpmError, match="ERROR"):
        g.csp_refine(cfg, CspCfg.make(7), imgs, rows, parts, tilts)


def test_a_refused_call_on_resident_images_leaves_the_handle_clean(series):
    """The refusal of test_csp_errors_are_loud (a row of a missing particle) comes after the spectra of all rows were enqueued, with
    the stack in device memory and so without a wait of its own: the call drains its stream before it returns, and the next call on
    the same handle answers bit for bit what a fresh handle answers."""
    import torch
    from pyp_amd import host, lib
    n, px, vol, imgs, rows, parts, tilts, cfg, g, o, O = series
    dev = torch.as_tensor(imgs.copy()).cuda()
    p2 = _perturb_particles(parts)
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, tilts)
    cc = CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0)
    bad = rows.copy(); bad[3, 26] = 999
    with pytest.raises(lib.PpmError, match="row 4 refers to a particle or tilt missing"):
        g.csp_refine(cfg, CspCfg.make(CSP_PARTICLES), dev, bad, parts, tilts)
    gr, gp, gt = g.csp_refine(cfg, cc, dev, rows2, p2, tilts)
    fresh = host.Reference(vol, n / 2)
    fr, fp, ft = fresh.csp_refine(cfg, cc, dev, rows2, p2, tilts)
    fresh.close()
    assert np.array_equal(gr, fr) and np.array_equal(gp, fp) and np.array_equal(gt, ft)
    assert not np.array_equal(gp, p2)                                   # and it searched


def test_csp_executable_extracts_then_refines_like_the_caller_drives_it(tmp_path):
    """The argv of create_csp_split_commands (local_run.py:364-376, :451-463): mode -2 per particle range into per-range
    stacks (merged like mrc.merge_fast), then mode 5 over particle ranges and mode 6 over tilts; the range outputs are
    merged like merge_alignment_parameters does (particle_cspt.py:96-138) and match the library called directly."""
    from pyp_amd import host
    n, px = 64, 2.0
    vol, stack, rows, parts, tilts = synth.make_tilt_series(n, 6, np.arange(-48, 49, 16.0), pixel=px, snr=0.3)
    series_img, rows = synth.paste_tilt_series(stack, rows, len(tilts), (256, 512))
    p2 = _perturb_particles(parts)
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, tilts)
    (tmp_path / "frealign" / "maps").mkdir(parents=True)
    scratch = tmp_path / "scratch"; scratch.mkdir()
    mrc.write(series_img, str(tmp_path / "frealign" / "ts.mrc"), pixel_size=px)
    mrc.write(vol, str(scratch / "tomo_frames_CSP_01.mrc"), pixel_size=px)
    par, ext = "frealign/maps/ts_r01_02.cistem", "frealign/maps/ts_r01_02_extended.cistem"
    cistem.write_parameters(str(tmp_path / par), rows2)
    cistem.write_extended(str(tmp_path / ext), p2, tilts)
    (tmp_path / ".pyp_config.toml").write_text(
        'data_set = "tomo"\nscope_pixel = 2.0\ndata_bin = 1\nextract_bin = 1\nextract_box = 64\nparticle_rad = 51.2\nparticle_mw = 300\n'
        'refine_iter = 2\nrefine_rlref = 0.0\nrefine_rhref = "5.3333333:4"\nrefine_fboost = false\ncsp_UseImagesForRefinementMin = 0\n'
        'csp_UseImagesForRefinementMax = -1\ncsp_ToleranceParticlesPsi = 8.0\ncsp_ToleranceParticlesTheta = 8.0\ncsp_ToleranceParticlesPhi = 8.0\n'
        'csp_ToleranceParticlesShifts = 8.0\ncsp_ToleranceMicrographTiltAngles = 1.5\ncsp_ToleranceMicrographTiltAxisAngles = 1.0\n'
        'csp_ToleranceMicrographShifts = 8.0\ncsp_OptimizerStepTolerance = 0.01\nreconstruct_norm = true\nrefine_invert = false\n')
    env = dict(os.environ, PYP_SCRATCH=str(scratch))

    def csp(*args, log="csp.log"):
        cmd = f"{BIN}/csp {' '.join(str(a) for a in args)} >> {log} 2>&1"
        return subprocess.run(cmd, shell=True, cwd=tmp_path, env=env).returncode

    # ---- mode -2 over two particle ranges, stacks concatenated in range order
    assert csp(par, ext, -2, 0, 2, 1, "frealign/ts.mrc", "frealign/ts_stack_0000_0002.mrc") == 0
    assert csp(par, ext, -2, 3, 5, 1, "frealign/ts.mrc", "frealign/ts_stack_0003_0005.mrc") == 0
    a, b = mrc.read(str(tmp_path / "frealign/ts_stack_0000_0002.mrc")), mrc.read(str(tmp_path / "frealign/ts_stack_0003_0005.mrc"))
    merged = np.concatenate([a, b])
    assert merged.shape == stack.shape
    cc = np.array([np.corrcoef(merged[j].ravel(), stack[j].numpy().ravel())[0, 1] for j in range(len(merged))])
    assert cc.min() > 0.999                                             # the pasted projections come back (re-normalised)
    mrc.write(merged, str(tmp_path / "frealign/ts_stack.mrc"), pixel_size=px)
    # ---- mode 5 (particles) over two ranges, merged like the caller
    assert csp(par, ext, 5, 0, 2, 1, "frealign/ts.mrc", "frealign/ts_stack.mrc") == 0
    assert csp(par, ext, 5, 3, 5, 1, "frealign/ts.mrc", "frealign/ts_stack.mrc") == 0
    log = (tmp_path / "csp.log").read_text()
    assert log.count("CSP: Normal termination") == 4 and "ERROR" not in log
    outs = sorted(str(p) for p in (tmp_path / "frealign/maps").glob("ts_r01_02_??????_??????.cistem"))
    assert [os.path.basename(o) for o in outs] == ["ts_r01_02_000000_000002.cistem", "ts_r01_02_000003_000005.cistem"]
    rows_m = cistem.merge_parameters(outs)
    assert rows_m.shape == rows2.shape and np.array_equal(rows_m[:, 0], rows2[:, 0])
    pm = p2.copy()
    for o in outs:
        e = cistem.read_extended(o.replace(".cistem", "_extended.cistem"))
        assert np.allclose(e["tilts"], tilts, atol=1e-4)
        for r in e["particles"]:
            pm[int(r[0])] = r
    cfg = RefineCfg.make(box=n, pixel_size=px, molecular_mass_kda=300, mask_radius=51.2, res_high=5.3333333, res_signed_cc=30.0, global_search=0)
    gr, gp, _ = host.Reference(vol, n / 2).csp_refine(cfg, CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0), merged, rows2, p2, tilts)
    assert _particle_angle_err(pm, gp).max() < 0.05 and np.abs(pm[:, 1:4] - gp[:, 1:4]).max() < 0.05      # float32 files, re-normalised boxes
    assert synth.angular_error_deg(rows_m, gr).max() < 0.05
    assert _particle_angle_err(pm, parts).mean() < 0.5 * _particle_angle_err(p2, parts).mean()
    # ---- mode 6 (tilts), one job per tilt like the caller (first = last = scanning-order index); merged over the original
    cistem.write_parameters(str(tmp_path / par), rows_m)
    cistem.write_extended(str(tmp_path / ext), pm, tilts)
    for f in outs:
        os.remove(f); os.remove(f.replace(".cistem", "_extended.cistem"))
    for t in range(len(tilts)):
        assert csp(par, ext, 6, t, t, 1, "frealign/ts.mrc", "frealign/ts_stack.mrc", log="csp6.log") == 0
    outs = sorted(str(p) for p in (tmp_path / "frealign/maps").glob("ts_r01_02_??????_??????.cistem"))
    assert len(outs) == len(tilts)
    rows_t = cistem.merge_parameters(outs)
    assert rows_t.shape == rows2.shape and np.array_equal(rows_t[:, 0], rows2[:, 0])
    for o in outs:
        e = cistem.read_extended(o.replace(".cistem", "_extended.cistem"))
        assert len(e["tilts"]) == 1 and len(e["particles"]) == len(parts)
    assert rows_t[:, 14].mean() >= rows_m[:, 14].mean() - 1e-3
    # mode 4 (defocus per tilt) runs; an unknown mode fails loudly
    assert csp(par, ext, 4, 0, 0, 1, "frealign/ts.mrc", "frealign/ts_stack.mrc", log="csp4.log") == 0
    assert csp(par, ext, 9, 0, 0, 1, "frealign/ts.mrc", "frealign/ts_stack.mrc", log="csp9.log") != 0
    assert "ERROR" in (tmp_path / "csp9.log").read_text()


def test_region_split_2x2x1_end_to_end_like_the_caller(tmp_path):
    """Region-based refinement as csp_run_refinement drives it (align/core.py:1106-1151): the series is split into a 2 x 2 x 1
    grid (regions.split_parameter_file = particle_cspt.py:141-208), `csp` runs once per (region, particle) in mode 5 and once per
    (region, tilt) in mode 6 with the command lines of create_csp_split_commands (local_run.py:327-404), the outputs match the
    caller's glob `_region????_??????_??????` and merge through Parameters.merge's rule; every job equals the ORACLE run on the
    region's rows.  A frame list (`frames_csp.txt`) feeds the same extraction as the tilt-series file."""
    import fnmatch
    from oracle import oracle as O
    import caller_regions as regions
    from pyp_amd.surface import csp_cli
    n, px = 64, 2.0
    vol, stack, rows, parts, tilts = synth.make_tilt_series(n, 6, np.arange(-40, 41, 20.0), pixel=px, snr=0.3, seed=11)
    imgs = stack.numpy()
    p2 = _perturb_particles(parts)
    rng = np.random.default_rng(8)
    t2 = tilts.copy()
    t2[:, 2:4] += rng.normal(0, 1.0, (len(t2), 2))
    rows2 = synth.csp_rows_from_params(rows, parts, tilts, p2, t2)
    (tmp_path / "frealign" / "maps").mkdir(parents=True)
    scratch = tmp_path / "scratch"; scratch.mkdir()
    mrc.write(vol, str(scratch / "tomo_frames_CSP_01.mrc"), pixel_size=px)
    mrc.write(imgs, str(tmp_path / "frealign" / "ts_stack.mrc"), pixel_size=px)
    par = "frealign/maps/ts_r01_02.cistem"
    cistem.write_parameters(str(tmp_path / par), rows2)
    cistem.write_extended(str(tmp_path / par.replace(".cistem", "_extended.cistem")), p2, t2)
    (tmp_path / ".pyp_config.toml").write_text(
        'data_set = "tomo"\nscope_pixel = 2.0\ndata_bin = 1\nextract_bin = 1\nextract_box = 64\nparticle_rad = 51.2\nparticle_mw = 300\n'
        'refine_iter = 2\nrefine_rlref = 0.0\nrefine_rhref = "5.3333333:4"\nrefine_fboost = false\ncsp_UseImagesForRefinementMin = 0\n'
        'csp_UseImagesForRefinementMax = -1\ncsp_ToleranceParticlesPsi = 8.0\ncsp_ToleranceParticlesTheta = 8.0\ncsp_ToleranceParticlesPhi = 8.0\n'
        'csp_ToleranceParticlesShifts = 8.0\ncsp_ToleranceMicrographTiltAngles = 1.5\ncsp_ToleranceMicrographTiltAxisAngles = 1.0\n'
        'csp_ToleranceMicrographShifts = 8.0\ncsp_OptimizerStepTolerance = 0.01\nreconstruct_norm = true\nrefine_invert = false\n')
    env = dict(os.environ, PYP_SCRATCH=str(scratch))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bl, tr = regions.find_specimen_bounds(p2, [1000, 1000, 1000])
        corners, size = regions.divide_regions(bl, tr, split_x=2, split_y=2, split_z=1)
        split = regions.split_parameter_file(rows2, p2, t2, par, regions.sort_particles_regions(p2, corners, size))
    finally:
        os.chdir(cwd)
    assert 2 <= len(split) <= 4 and sorted(int(p) for s in split for p in s[1]) == list(range(6))
    cfg = RefineCfg.make(box=n, pixel_size=px, molecular_mass_kda=300, mask_radius=51.2, res_high=5.3333333, res_signed_cc=30.0, global_search=0)
    oref = O.Reference(vol, n / 2)

    def run_all(cmds, log):
        for c in cmds:
            argv, _ = csp_cli.split_command(c)
            r = subprocess.run(f"{' '.join(argv)} >> {log} 2>&1", shell=True, cwd=tmp_path, env=env)
            assert r.returncode == 0, (tmp_path / log).read_text()[-1500:]

    # ---- outer mode 7 -> 2 -> argv mode 5: one job per particle of every region
    cmds, _ = regions.csp_split_commands(f"{BIN}/csp", split, 2, "ts_r01_02", "frealign/ts_stack.mrc", list(range(6)), list(range(5)))
    assert len(cmds) == 6 and all(" 5 " in c for c in cmds)
    run_all(cmds, "csp5.log")
    outs = sorted(str(p) for p in (tmp_path / "frealign/maps").glob("ts_r01_02_region????_??????_??????.cistem"))
    assert len(outs) == 6 and all(fnmatch.fnmatch(os.path.basename(o), "ts_r01_02_region????_??????_??????.cistem") for o in outs)
    outs_ext = [str(tmp_path / par.replace(".cistem", "_extended.cistem"))] + [o.replace(".cistem", "_extended.cistem") for o in outs]
    rows_m, pm, tm = csp_cli.merge_alignment_parameters(outs, outs_ext)
    assert rows_m.shape == rows2.shape and np.array_equal(rows_m[:, 0], rows2[:, 0]) and len(pm) == 6
    # the oracle on each region file, particle by particle
    for fn, pinds, tinds in split:
        rr = cistem.read_parameters(str(tmp_path / fn))
        ee = cistem.read_extended(str(tmp_path / fn.replace(".cistem", "_extended.cistem")))
        ri = imgs[rr[:, 0].astype(int) - 1]
        for p in pinds:
            cc = CspCfg.make(CSP_PARTICLES, tol_angle=(8, 8, 8), tol_shift=4.0, first=int(p), last=int(p))
            sel = rr[:, 26] == p
            wr, wp, wt, _ = O.csp_refine(oref, cfg, cc, ri[sel], rr[sel], ee["particles"], ee["tilts"])
            got_p = pm[pm[:, 0] == p]
            want_p = wp[wp[:, 0] == p]
            assert _particle_angle_err(want_p, got_p).max() < 0.1 and np.abs(want_p[:, 1:4] - got_p[:, 1:4]).max() < 0.5
            gr = rows_m[np.isin(rows_m[:, 0], rr[sel][:, 0])]
            assert synth.angular_error_deg(wr, gr).max() < 0.1 and synth.shift_error_px(wr, gr, px).max() < 0.5
    assert _particle_angle_err(pm, parts).mean() < 0.5 * _particle_angle_err(p2, parts).mean()
    # the merged rows carry RIND = their region, so the (TIND, region) tilt entries must come along with the particle jobs' outputs
    # (region 0's entries take the place of the original (TIND, 0) ones: Parameters.merge keys tilts by (TIND, RIND))
    assert len(tm) == len(t2) * len(split) and set(rows_m[:, 28].astype(int)) == set(range(len(split)))
    # ---- outer mode 5 -> 3 -> argv mode 6: one job per (region, tilt); merged tilts are keyed (TIND, region)
    for f in outs:
        os.remove(f); os.remove(f.replace(".cistem", "_extended.cistem"))
    cmds, _ = regions.csp_split_commands(f"{BIN}/csp", split, 3, "ts_r01_02", "frealign/ts_stack.mrc", list(range(6)), list(range(5)))
    assert len(cmds) == 5 * len(split) and all(" 6 " in c for c in cmds)
    run_all(cmds, "csp6.log")
    outs = sorted(str(p) for p in (tmp_path / "frealign/maps").glob("ts_r01_02_region????_??????_??????.cistem"))
    assert len(outs) == 5 * len(split)
    outs_ext = [str(tmp_path / par.replace(".cistem", "_extended.cistem"))] + [o.replace(".cistem", "_extended.cistem") for o in outs]
    rows_t, pt, tt = csp_cli.merge_alignment_parameters(outs, outs_ext)
    assert rows_t.shape == rows2.shape and np.array_equal(rows_t[:, 0], rows2[:, 0])
    keys = sorted((int(t[0]), int(t[1])) for t in tt)
    assert keys == sorted({(t, 0) for t in range(5)} | {(t, k) for k in range(len(split)) for t in range(5)})
    fn, pinds, tinds = split[-1]
    k = len(split) - 1
    rr = cistem.read_parameters(str(tmp_path / fn))
    ee = cistem.read_extended(str(tmp_path / fn.replace(".cistem", "_extended.cistem")))
    ri = imgs[rr[:, 0].astype(int) - 1]
    for t in (0, 3):
        cm = CspCfg.make(CSP_MICROGRAPHS, tol_angle=(1.5, 1.0, 0), tol_shift=4.0, first=t, last=t)
        sel = rr[:, 27] == t
        wr, wp, wt, _ = O.csp_refine(oref, cfg, cm, ri[sel], rr[sel], ee["particles"], ee["tilts"])
        want_t = wt[(wt[:, 0] == t) & (wt[:, 1] == k)][0]
        got_t = tt[(tt[:, 0] == t) & (tt[:, 1] == k)][0]
        assert np.abs(want_t[4:6] - got_t[4:6]).max() < 0.1 and np.abs(want_t[2:4] - got_t[2:4]).max() < 0.5
    log = (tmp_path / "csp6.log").read_text() + (tmp_path / "csp5.log").read_text()
    assert "ERROR" not in log and log.count("CSP: Normal termination") == 6 + 5 * len(split)
    # ---- frames: the list names one movie per tilt; the same boxes come out as from the tilt-series file
    series_img, rows_p = synth.paste_tilt_series(stack, rows, len(tilts), (256, 512))
    mrc.write(series_img, str(tmp_path / "frealign" / "ts.mrc"), pixel_size=px)
    for t in range(len(tilts)):
        mrc.write(np.stack([series_img[t] * 0, series_img[t]]), str(tmp_path / "frealign" / f"ts_{t:03d}.mrc"), pixel_size=px)
    (tmp_path / "frames_csp.txt").write_text("\n".join(f"frealign/ts_{t:03d}.mrc" for t in range(len(tilts))))
    rows_f = rows_p.copy()
    rows_f[:, 29] = 1                                           # FIND: the second section of every movie holds the image
    cistem.write_parameters(str(tmp_path / "frealign/maps/fr_r01_02.cistem"), rows_f)
    cistem.write_extended(str(tmp_path / "frealign/maps/fr_r01_02_extended.cistem"), parts, tilts)
    cistem.write_parameters(str(tmp_path / "frealign/maps/ser_r01_02.cistem"), rows_p)
    cistem.write_extended(str(tmp_path / "frealign/maps/ser_r01_02_extended.cistem"), parts, tilts)
    run_all([f"{BIN}/csp frealign/maps/fr_r01_02.cistem frealign/maps/fr_r01_02_extended.cistem -2 0 5 1 frames_csp.txt frealign/fr_stack.mrc",
             f"{BIN}/csp frealign/maps/ser_r01_02.cistem frealign/maps/ser_r01_02_extended.cistem -2 0 5 1 frealign/ts.mrc frealign/ser_stack.mrc"], "csp_frames.log")
    assert np.array_equal(mrc.read(str(tmp_path / "frealign/fr_stack.mrc")), mrc.read(str(tmp_path / "frealign/ser_stack.mrc")))
    # ---- mode -2.1: the same extraction with running frame averages (one frame per movie here: the average of a single frame is the
    # frame itself, normalised again - the stack equals mode -2's up to that second normalisation)
    run_all([f"{BIN}/csp frealign/maps/fr_r01_02.cistem frealign/maps/fr_r01_02_extended.cistem -2.1 0 5 1 frames_csp.txt frealign/fr_avg_stack.mrc"], "csp_avg.log")
    a21, a2 = mrc.read(str(tmp_path / "frealign/fr_avg_stack.mrc")), mrc.read(str(tmp_path / "frealign/fr_stack.mrc"))
    assert a21.shape == a2.shape and np.abs(a21 - a2).max() < 1e-3 and "running averages over +-2 frames" in (tmp_path / "csp_avg.log").read_text()
    r = subprocess.run(f"{BIN}/csp frealign/maps/fr_r01_02.cistem frealign/maps/fr_r01_02_extended.cistem -2 0 5 1 missing_frames.txt x.mrc", shell=True,
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR" in r.stdout and "missing_frames.txt" in r.stdout
