"""Movie-frame refinement on the GPU (ppm_frame_refine, bin/csp with the refine-frames flag) against the CPU oracle and the float64
statement of the pooling and peak rules (pyp_amd/frames.py); inputs and references: tests/frame_cases.py.

Tolerances.  An own map value is the normalised sum the other score tests bound by `defocus_cases.tol(n)` = 2e-5 max(1, n / 64); a pooled
value is a convex combination of own values and takes the same bound.  The arg-max must agree wherever the reference's best value
leads the runner-up by more than twice that (both may move by it); the rest, at most 5 % of the rows, is undecided.  A parabolic offset
(l - r) / (2 (l - 2c + r)) h moves by at most 4 tol / |l - 2c + r| h when its three values move by tol each (to first order: numerator
and denominator by 2 tol and 4 tol, |l - r| <= |l - 2c + r| at a maximum)."""
import fnmatch
import os
import subprocess

import numpy as np
import pytest

import frame_cases as FC
from pyp_amd import frames as F
from pyp_amd import synth
from pyp_amd.formats import cistem, mrc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
C = cistem.COL
N = 64
TOL = FC.tol(N)
SHIFT_COLS = [C["X_SHIFT"], C["Y_SHIFT"], C["FSHIFT_X"], C["FSHIFT_Y"]]


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def common(H):
    """The common case, its GPU reference handle and the GPU result per half-width (computed once, read-only)."""
    vol, imgs, rows, true = FC.series()
    g = H.Reference(vol, N / 2)
    cache = {}

    def run(hw):
        if hw not in cache:
            cache[hw] = g.frame_refine(FC.cfg_for(N), FC.fcfg(hw), imgs, rows, maps=True)
            for a in (cache[hw][0], cache[hw][2], cache[hw][3]):
                a.setflags(write=False)
        return cache[hw]
    return g, imgs, rows, true, run


def _deltas_px(rows_in, rows_out):
    """(X / Y_SHIFT delta, FSHIFT delta) in pixels"""
    d = (rows_out[:, SHIFT_COLS] - rows_in[:, SHIFT_COLS]) / FC.PX
    return d[:, :2], d[:, 2:]


def _untouched_but(rows_in, rows_out, cols):
    keep = [c for c in range(rows_in.shape[1]) if c not in cols]
    return np.array_equal(rows_in[:, keep], rows_out[:, keep])


# ------------------------------------------------------------------------------------------------ 1. own maps against the oracle
def test_own_maps_match_the_oracle_at_every_grid_point(common):
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(2)
    want = FC.common_maps()
    err = np.abs(own - want).max()
    print("box 64: own maps, max |gpu - oracle| = %.3g (bound %.3g)" % (err, TOL))
    assert own.shape == (84, 9, 9) and err < TOL
    assert info["groups"] == 12 and info["models"] == 12 and info["rows_refined"] == 84 and info["rows_scored"] == info["rows_skipped"] == 0
    assert (info["n_steps"], info["step_px"], info["range_px"], info["clipped"]) == (4, 0.5, 2.0, 0)
    assert FC.list_length(FC.RHI) <= FC.TILE                        # one tile, the slice store in LDS


@pytest.mark.parametrize("n,rhi,path", [(96, 40.0, "two tiles, store in LDS"), (128, 56.0, "three tiles, store in global memory")])
def test_own_maps_at_other_boxes_and_a_defocus_jump(H, n, rhi, path):
    """Box 96 (radix 3) and box 128, two groups of 7 frames; frame 3 of the first group has its defocus 300 A off: it still matches, and it
    costs exactly one more gather (the frames either side of it still share theirs).  The bands are chosen for the kernel's other two paths."""
    length = FC.list_length(rhi)
    assert (FC.TILE < length <= FC.LDS_STORE_MAX) if n == 96 else length > FC.LDS_STORE_MAX, path
    tilts = (-20.0, 20.0)
    vol, imgs, rows, _ = FC.series(n, 1, 7, True, tilts)
    want = FC.common_maps(n, 1, 7, True, rhi, tilts)
    g = H.Reference(vol, n / 2)
    out, info, own, pooled = g.frame_refine(FC.cfg_for(n, rhi), FC.fcfg(2), imgs, rows, maps=True)
    err = np.abs(own - want).max()
    print("box %d: own maps, max |gpu - oracle| = %.3g (bound %.3g)" % (n, err, FC.tol(n)))
    assert err < FC.tol(n)
    assert info["groups"] == 2 and info["models"] == 2 + 1
    g.close()


# ------------------------------------------------------------------------------------------------ 2. pooling and peak
@pytest.mark.parametrize("hw", [0, 2, 10])
def test_pooling_and_peak_match_the_float64_statement(common, hw):
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(hw)
    want_own = FC.common_maps()
    ref = FC.reference(rows, want_own, hw)
    err = np.abs(pooled - ref["pooled"]).max()
    print("half_width %d: pooled maps, max |gpu - reference| = %.3g (bound %.3g)" % (hw, err, TOL))
    assert err < TOL
    if hw == 0:
        assert np.array_equal(pooled, own)
    decided = ref["margin"] > 2 * TOL
    print("half_width %d: %d of %d rows undecided" % (hw, (~decided).sum(), len(rows)))
    assert (~decided).mean() <= 0.05
    assert np.array_equal(pooled.reshape(len(rows), -1).argmax(axis=1)[decided], ref["index"][decided])
    dxy, dfs = _deltas_px(rows, out)
    assert np.abs(dxy - dfs).max() < 1e-9                         # X / Y_SHIFT and FSHIFT move together
    h = FC.STEP
    for j in np.flatnonzero(decided):
        q = ref["index"][j]
        for ax in range(2):
            cur = ref["curvature"][j, ax]
            bound = (4 * TOL / abs(cur) * h if np.isfinite(cur) else 0.0) + 1e-6
            assert abs(dxy[j, ax] - ref["delta"][j, ax]) <= bound, (j, ax, dxy[j, ax], ref["delta"][j, ax], cur)
        assert abs(out[j, C["SCORE"]] - 100.0 * want_own[j].ravel()[q]) < 100 * TOL
    assert _untouched_but(rows, out, SHIFT_COLS + [C["SCORE"]])


# ------------------------------------------------------------------------------------------------ 4. invariance, bit for bit
def test_row_order_call_split_and_image_residence_change_nothing(common):
    import torch
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(2)
    cfg, fc = FC.cfg_for(N), FC.fcfg(2)
    perm = np.random.default_rng(3).permutation(len(rows))
    o2, i2, w2, p2 = g.frame_refine(cfg, fc, imgs[perm], rows[perm], maps=True)
    assert np.array_equal(o2, out[perm]) and np.array_equal(w2, own[perm]) and np.array_equal(p2, pooled[perm])
    first = rows[:, C["PIND"]] < 2                                  # six groups a call
    for sel in (first, ~first):
        o3, i3, w3, p3 = g.frame_refine(cfg, fc, imgs[sel], rows[sel], maps=True)
        assert i3["groups"] == 6
        assert np.array_equal(o3, out[sel]) and np.array_equal(w3, own[sel]) and np.array_equal(p3, pooled[sel])
    dev = torch.as_tensor(imgs.copy()).cuda()
    o4, i4, w4, p4 = g.frame_refine(cfg, fc, dev, rows, maps=True)
    assert np.array_equal(o4, out) and np.array_equal(w4, own) and np.array_equal(p4, pooled)


# ------------------------------------------------------------------------------------------------ 5. edges
def test_a_shift_beyond_the_window_ends_on_its_edge_without_a_parabola(common, O):
    g, imgs, rows, true, run = common
    sel = np.flatnonzero((rows[:, C["PIND"]] == 0) & (rows[:, C["TIND"]] == 1))
    r = rows[sel].copy()
    r[:, C["X_SHIFT"]] += 3.0 * FC.PX                               # the truth now lies 3 pixels to the left of a window of +-2
    cfg = FC.cfg_for(N)
    want_own = FC.oracle_maps(O, O.Reference(FC.series()[0], N / 2), cfg, imgs[sel], r, FC.STEP, 4)
    ref = FC.reference(r, want_own, 2)
    jx = ref["index"] % 9
    on_edge = (jx == 0) & (ref["margin"] > 2 * TOL)
    assert on_edge.sum() >= 4, jx
    out, info, own, pooled = g.frame_refine(cfg, FC.fcfg(2), imgs[sel], r, maps=True)
    assert np.abs(own - want_own).max() < TOL
    dxy, dfs = _deltas_px(r, out)
    assert np.abs(dxy[on_edge, 0] + 2.0).max() < 1e-9 and np.abs(dfs[on_edge, 0] + 2.0).max() < 1e-9


def test_an_unoccupied_frame_stays_and_leaves_its_neighbours_pools(common, O):
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(2)
    sel = np.flatnonzero((rows[:, C["PIND"]] == 1) & (rows[:, C["TIND"]] == 0))
    r = rows[sel].copy()
    r[3, C["OCCUPANCY"]] = 0.0
    o2, i2, w2, p2 = g.frame_refine(FC.cfg_for(N), FC.fcfg(2), imgs[sel], r, maps=True)
    assert np.array_equal(o2[3], r[3]) and not w2[3].any() and not p2[3].any()
    assert (i2["rows_refined"], i2["rows_skipped"], i2["groups"], i2["models"]) == (6, 1, 1, 1)
    use = np.arange(7) != 3
    assert np.array_equal(w2[use], own[sel][use])                   # the own maps do not know about the neighbours
    ref = FC.reference(r, FC.common_maps()[sel], 2)
    assert np.abs(p2 - ref["pooled"]).max() < TOL
    assert not np.array_equal(p2[2], pooled[sel][2]) and not np.array_equal(p2[4], pooled[sel][4]) and np.array_equal(p2[0], pooled[sel][0])


def test_a_single_frame_and_a_gap_in_find(common):
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(2)
    want_own = FC.common_maps()
    o1, i1, w1, p1 = g.frame_refine(FC.cfg_for(N), FC.fcfg(2), imgs[5:6], rows[5:6], maps=True)
    assert (i1["groups"], i1["models"], i1["rows_refined"]) == (1, 1, 1)
    assert np.array_equal(w1[0], own[5]) and np.array_equal(p1[0], w1[0])
    sel = np.array([14, 15, 17, 18])                                # FIND 0, 1, 3, 4 of the third group
    assert list(rows[sel, C["FIND"]]) == [0, 1, 3, 4] and len(set(rows[sel, C["TIND"]])) == 1
    o2, i2, w2, p2 = g.frame_refine(FC.cfg_for(N), FC.fcfg(2), imgs[sel], rows[sel], maps=True)
    ref = FC.reference(rows[sel], want_own[sel], 2)
    assert np.abs(p2 - ref["pooled"]).max() < TOL
    w = F.pool_weights([0, 1, 3, 4], 2)
    assert w[1, 2] == np.exp(-2.0) and w[0, 2] == 0                 # by FIND distance: 1 -> 3 is two frames away, 0 -> 3 out of reach


def test_a_range_beyond_the_grid_is_clipped_and_said_so(common, O):
    """17 x 17 = 289 points: a thread's second grid point.  Own maps of one group against the oracle over the whole grid."""
    g, imgs, rows, true, run = common
    sel = np.arange(7)
    cfg = FC.cfg_for(N)
    out, info, own, pooled = g.frame_refine(cfg, FC.fcfg(2, range_px=10.0), imgs[sel], rows[sel], maps=True)
    assert (info["n_steps"], info["clipped"], info["range_px"]) == (8, 1, 4.0) and own.shape == (7, 17, 17)
    assert "frame refinement" in g.note() and "+-4" in g.note()
    want = FC.oracle_maps(O, O.Reference(FC.series()[0], N / 2), cfg, imgs[sel], rows[sel], FC.STEP, 8)
    assert np.abs(own - want).max() < TOL
    assert np.array_equal(own[:, 4:13, 4:13], run(2)[2][sel])       # the inner 9 x 9 points are the narrow grid's, bit for bit
    g.frame_refine(cfg, FC.fcfg(2), imgs[sel], rows[sel])
    assert g.note() == ""


def test_tilt_windows_refine_score_or_skip(common):
    g, imgs, rows, true, run = common
    out, info, own, pooled = run(2)
    want_own = FC.common_maps()
    cfg = FC.cfg_for(N)
    o2, i2 = g.frame_refine(cfg, FC.fcfg(2, tind_min=1, tind_max=1), imgs, rows)
    t = rows[:, C["TIND"]]
    assert (i2["rows_refined"], i2["rows_scored"], i2["rows_skipped"]) == (28, 56, 0)
    assert np.array_equal(o2[t == 1], out[t == 1])
    assert _untouched_but(rows[t != 1], o2[t != 1], [C["SCORE"]])
    assert np.abs(o2[t != 1, C["SCORE"]] - 100.0 * want_own[t != 1, 4, 4]).max() < 100 * TOL
    o3, i3 = g.frame_refine(cfg, FC.fcfg(2, first=2, last=-1), imgs, rows)
    assert (i3["groups"], i3["rows_refined"], i3["rows_skipped"]) == (4, 28, 56)
    assert np.array_equal(o3[t == 2], out[t == 2]) and np.array_equal(o3[t != 2], rows[t != 2])


def test_the_four_refusals(common, H):
    from pyp_amd import lib
    g, imgs, rows, true, run = common
    cfg = FC.cfg_for(N)
    r = rows[:7].copy()
    r[4, C["FIND"]] = 2
    with pytest.raises(lib.PpmError, match="FIND 2 occurs twice"):
        g.frame_refine(cfg, FC.fcfg(2), imgs[:7], r)
    for kw, msg in ((dict(step_px=-0.5), "step_px"), (dict(range_px=0.0), "range_px"), (dict(range_px=-1.0), "range_px"), (dict(half_width=-1), "half_width")):
        with pytest.raises(lib.PpmError, match=msg):
            g.frame_refine(cfg, FC.fcfg(**{**dict(half_width=2), **kw}), imgs[:7], rows[:7])


def test_a_refused_call_on_resident_images_leaves_the_handle_clean(common, H):
    """None of the four refusals is reached after the spectra are enqueued (the plan's three come first of all, the doubled FIND while
    the frame list is built, ahead of any device work), so this takes the earliest that touches the rows, the doubled FIND: the guard
    that drains the stream on an error return does no harm, and the next call on the handle, on images in device memory, answers
    bit for bit what a fresh handle answers."""
    import torch
    from pyp_amd import lib
    g, imgs, rows, true, run = common
    cfg, fc = FC.cfg_for(N), FC.fcfg(2)
    dev = torch.as_tensor(imgs[:14].copy()).cuda()
    r = rows[:14].copy()
    r[4, C["FIND"]] = 2
    with pytest.raises(lib.PpmError, match="FIND 2 occurs twice"):
        g.frame_refine(cfg, fc, dev, r, maps=True)
    out, info, own, pooled = g.frame_refine(cfg, fc, dev, rows[:14], maps=True)
    fresh = H.Reference(FC.series()[0], N / 2)
    o2, i2, w2, p2 = fresh.frame_refine(cfg, fc, dev, rows[:14], maps=True)
    fresh.close()
    assert info == i2 and info["groups"] == 2 and info["rows_refined"] == 14
    assert np.array_equal(out, o2) and np.array_equal(own, w2) and np.array_equal(pooled, p2)
    assert np.array_equal(own, run(2)[2][:14])                          # ... which is what the whole series gave for these groups


# ------------------------------------------------------------------------------------------------ 6. drop-in
TOML = ('data_set = "mov"\nscope_pixel = 1.5\ndata_bin = 1\nextract_bin = 1\nextract_box = 64\nparticle_rad = 38.4\nparticle_mw = 300\n'
        'refine_iter = 2\nrefine_rlref = 0.0\nrefine_rhref = 4.8\nrefine_fboost = false\ncsp_UseImagesForRefinementMin = %d\n'
        'csp_UseImagesForRefinementMax = %d\ncsp_ToleranceMicrographTiltAngles = 1.5\ncsp_ToleranceMicrographTiltAxisAngles = 1.0\n'
        'csp_ToleranceMicrographShifts = 3.0\ncsp_OptimizerStepTolerance = 0.01\ncsp_running_average_frames = 2\nreconstruct_norm = true\n'
        'refine_invert = false\ncsp_frame_refinement = %s\n')
REGION = "frealign/maps/mov_r01_02_region0000.cistem"
ARGV = f"{BIN}/csp {REGION} {REGION.replace('.cistem', '_extended.cistem')} 3 0 -1 1 frames_csp.txt frealign/mov_stack.mrc"


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """A scratch project with one particle's region file and its frame stack, cut by mode -2 from a frame list (one movie per tilt)."""
    tmp = tmp_path_factory.mktemp("frames_project")
    vol, stack, rows, true, parts, tilts = synth.make_frame_series(N, 1, list(FC.TILTS), 7, pixel=FC.PX, snr=FC.SNR, vol=FC.D.volume(N), seed=77)
    imgs = stack.numpy()
    (tmp / "frealign" / "maps").mkdir(parents=True)
    scratch = tmp / "scratch"; scratch.mkdir()
    mrc.write(vol, str(scratch / "mov_frames_CSP_01.mrc"), pixel_size=FC.PX)
    rng = np.random.default_rng(5)
    rows = rows.copy()
    for t in range(len(tilts)):
        movie = rng.normal(0, 1, (7, 160, 160)).astype(np.float32)
        for j in np.flatnonzero(rows[:, C["TIND"]] == t):
            movie[int(rows[j, C["FIND"]]), 80 - 32:80 + 32, 80 - 32:80 + 32] = imgs[j]
            rows[j, C["ORIGINAL_X_POSITION"]], rows[j, C["ORIGINAL_Y_POSITION"]] = 80, 80
        mrc.write(movie, str(tmp / "frealign" / f"mov_{t:03d}.mrc"), pixel_size=FC.PX)
    (tmp / "frames_csp.txt").write_text("\n".join(f"frealign/mov_{t:03d}.mrc" for t in range(len(tilts))))
    cistem.write_parameters(str(tmp / REGION), rows)
    cistem.write_extended(str(tmp / REGION.replace(".cistem", "_extended.cistem")), parts, tilts)
    (tmp / ".pyp_config.toml").write_text(TOML % (0, -1, "true"))
    env = dict(os.environ, PYP_SCRATCH=str(scratch))

    def run(cmd, log):
        r = subprocess.run(f"{cmd} > {log} 2>&1", shell=True, cwd=tmp, env=env)
        assert r.returncode == 0, (tmp / log).read_text()[-1500:]
        return (tmp / log).read_text()
    run(f"{BIN}/csp {REGION} {REGION.replace('.cistem', '_extended.cistem')} -2 0 0 1 frames_csp.txt frealign/mov_stack.mrc", "extract.log")
    return tmp, run, vol, cistem.read_parameters(str(tmp / REGION)), mrc.read(str(tmp / "frealign/mov_stack.mrc")), parts, tilts


def _outputs(tmp):
    outs = sorted(str(p) for p in (tmp / "frealign/maps").glob("mov_r01_02_region????_??????_??????.cistem"))
    assert len(outs) == 1 and os.path.basename(outs[0]) == "mov_r01_02_region0000_000000_-00001.cistem"
    assert fnmatch.fnmatch(os.path.basename(outs[0]), "*_region????_??????_??????.cistem")
    return outs[0], outs[0].replace(".cistem", "_extended.cistem")


def test_dropin_refines_frames_like_the_library_call(project, H):
    tmp, run, vol, rin, stack, parts, tilts = project
    (tmp / ".pyp_config.toml").write_text(TOML % (0, -1, "true"))
    log = run(ARGV, "frames.log")
    assert "ERROR" not in log and "CSP: Normal termination" in log and "9 x 9 points" in log and "3 groups, 3 models; 21 rows refined" in log
    out_main, out_ext = _outputs(tmp)
    got = cistem.read_parameters(out_main)
    g = H.Reference(vol, N / 2)
    want, info = g.frame_refine(FC.cfg_for(N), FC.fcfg(2, range_px=3.0 / FC.PX, step_px=0.0), stack, rin)
    g.close()
    assert np.array_equal(got, want.astype(np.float32).astype(np.float64))
    d = got[:, SHIFT_COLS] - rin[:, SHIFT_COLS]
    assert np.abs(d[:, :2]).max() > 0.1 and np.abs(d[:, :2] - d[:, 2:]).max() < 1e-4          # the same Angstroms, as float32 columns
    assert _untouched_but(rin, got, SHIFT_COLS + [C["SCORE"]])
    ext = cistem.read_extended(out_ext)
    assert np.allclose(ext["particles"], parts, atol=1e-3) and np.allclose(ext["tilts"], tilts, atol=1e-3) and len(ext["tilts"]) == 3


def test_dropin_evaluates_only_beyond_the_refined_tilts(project, O):
    tmp, run, vol, rin, stack, parts, tilts = project
    (tmp / ".pyp_config.toml").write_text(TOML % (3, 3, "true"))
    log = run(ARGV, "evaluate.log")
    assert "0 rows refined, 21 scored" in log and "CSP: Normal termination" in log
    got = cistem.read_parameters(_outputs(tmp)[0])
    assert _untouched_but(rin, got, [C["SCORE"]])
    want = 100.0 * O.score_batch(O.Reference(vol, N / 2), FC.cfg_for(N), stack, rin)
    assert np.abs(got[:, C["SCORE"]] - want).max() < 100 * TOL + 1e-4


def test_dropin_without_the_key_is_the_tilt_refinement_it_was(project, H):
    """csp_frame_refinement = false: the same argv runs mode 3 as before - one shift per tilt - byte for byte what that path's own calls
    write (make_csp_cfg, Reference.csp_refine, the two writers)."""
    from pyp_amd.surface import csp_cli
    tmp, run, vol, rin, stack, parts, tilts = project
    (tmp / ".pyp_config.toml").write_text(TOML % (0, -1, "false"))
    log = run(ARGV, "tilts.log")
    assert "Frame refinement" not in log and "Refined 3 tilts" in log
    out_main, out_ext = _outputs(tmp)
    s = csp_cli._settings(csp_cli.read_flat_toml(str(tmp / ".pyp_config.toml")))
    ext = cistem.read_extended(str(tmp / REGION.replace(".cistem", "_extended.cistem")))
    cfg = csp_cli.RefineCfg.make(box=N, pixel_size=float(rin[0, C["PIXEL_SIZE"]]), molecular_mass_kda=s["mw"], mask_radius=s["radius"], res_low=s["res_low"],
                                 res_high=s["res_high"], res_signed_cc=s["res_signed"], global_search=0, local_refine=1, normalize=s["normalize"], invert=s["invert"])
    g = H.Reference(vol, N / 2)
    rout, pout, tout = g.csp_refine(cfg, csp_cli.make_csp_cfg(s, 3, 0, -1, float(rin[0, C["PIXEL_SIZE"]])), stack, rin, ext["particles"], ext["tilts"])
    g.close()
    cistem.write_parameters(str(tmp / "want.cistem"), rout)
    cistem.write_extended(str(tmp / "want_extended.cistem"), pout, tout)
    assert open(out_main, "rb").read() == open(tmp / "want.cistem", "rb").read()
    assert open(out_ext, "rb").read() == open(tmp / "want_extended.cistem", "rb").read()
    assert np.ptp(rout[rout[:, C["TIND"]] == 0][:, C["X_SHIFT"]] - rin[rin[:, C["TIND"]] == 0][:, C["X_SHIFT"]]) < 1e-3    # one shift per tilt
