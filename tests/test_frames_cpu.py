"""Movie-frame refinement, the parts that need no GPU: the executable's decision whether an argv asks for it, the grid rule of
pyp_amd/csrc/ppm_frame_plan.h against its numpy statement, the pooling weights against mode -2.1's, the peak rule on constructed maps, the
synthetic frame series, and the condition the GPU tests rest on - that the float64 reference itself recovers the planted drifts."""
import json
import os
import subprocess

import numpy as np
import pytest

import frame_cases as FC
from pyp_amd import frames as F
from pyp_amd import synth
from pyp_amd.formats import cistem
from pyp_amd.surface import csp_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = cistem.COL
FRAME_ARGV = "csp ts1_r01_02_region0003.cistem ts1_r01_02_region0003_extended.cistem 3 0 -1 1 frames_csp.txt frealign/ts1_stack.mrc"


def test_only_the_frame_refinement_argv_takes_the_new_path(golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "golden_r03.json")))["csp_split_commands"]
    n = 0
    for key, g in gold.items():
        for cmd in g["commands"]:
            a = csp_cli.parse_argv(csp_cli.split_command(cmd)[0][1:])
            for on in (True, False):
                assert not F.is_frame_refinement(a["mode"], a["flag"], a["images"], {"csp_frame_refinement": on}), cmd
            n += 1
    assert n >= 24
    a = csp_cli.parse_argv(FRAME_ARGV.split()[1:])
    assert (a["mode"], a["first"], a["last"], a["flag"]) == (3, 0, -1, "1")
    assert F.is_frame_refinement(a["mode"], a["flag"], a["images"], {"csp_frame_refinement": True})
    assert csp_cli._out_names(a["param_file"], a["first"], a["last"])[0] == "ts1_r01_02_region0003_000000_-00001.cistem"
    # every one of the four conditions is needed; the key must be the boolean the configuration writer stores
    for mode, flag, images, settings in ((6, "1", "frames_csp.txt", {"csp_frame_refinement": True}), (3, "0", "frames_csp.txt", {"csp_frame_refinement": True}),
                                         (3, "1", "frealign/ts1.mrc", {"csp_frame_refinement": True}), (3, "1", "frames_csp.txt", {"csp_frame_refinement": False}),
                                         (3, "1", "frames_csp.txt", {}), (3, "1", "frames_csp.txt", {"csp_frame_refinement": "true"}),
                                         (-2, "1", "frames_csp.txt", {"csp_frame_refinement": True}), (5, "1", "frames_csp.txt", {"csp_frame_refinement": True})):
        assert not F.is_frame_refinement(mode, flag, images, settings), (mode, flag, images, settings)


def test_the_key_is_read_as_a_boolean_from_the_project_file(tmp_path):
    (tmp_path / "p.toml").write_text('csp_frame_refinement = true\ncsp_running_average_frames = 3\n')
    p = csp_cli.read_flat_toml(str(tmp_path / "p.toml"))
    assert p["csp_frame_refinement"] is True and F.is_frame_refinement(3, "1", "frames_csp.txt", p)
    (tmp_path / "p.toml").write_text('csp_frame_refinement = false\n')
    assert not F.is_frame_refinement(3, "1", "frames_csp.txt", csp_cli.read_flat_toml(str(tmp_path / "p.toml")))


SRC = r'''
#include <cstdio>
#include "ppm_frame_plan.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    float range, step;
    while (fscanf(f, "%f %f", &range, &step) == 2) {
        int clipped = -1;
        const float h = ppm::frame_step(step);
        const int w = ppm::frame_steps(range, h, PPM_FRAME_MAX_STEPS, &clipped);
        printf("%.17g %d %d\n", (double)h, w, clipped);
    }
    fclose(f);
    return 0;
}
'''
# (range_px, step_px) -> (W, clipped), the cases a reader would check by hand; the sweep below adds the rest
PLANS = {(2.0, 0.5): (4, 0), (2.0, 0.0): (4, 0), (0.3, 0.1): (3, 0), (4.0, 0.5): (8, 0), (4.01, 0.5): (8, 1), (100.0, 0.5): (8, 1), (0.2, 0.5): (1, 0),
         (1.0, 1.0): (1, 0), (1.0000001, 1.0): (1, 0), (1.001, 1.0): (2, 0), (66.7, 1.5): (8, 1), (2.0, 0.25): (8, 0), (1e-9, 0.5): (0, 0)}


def test_grid_rule_of_the_header_is_the_numpy_rule(tmp_path):
    """ppm_frame_plan.h compiled alone with the host compiler under AddressSanitizer and UBSan."""
    rng = np.random.default_rng(1)
    cases = list(PLANS) + [(float(np.float32(r)), float(np.float32(s))) for r, s in zip(rng.uniform(0.01, 12, 200), rng.choice([0.0, 0.1, 0.25, 0.5, 0.75, 1.0, 1.5], 200))]
    cases += [(k * s, s) for s in (0.1, 0.25, 0.3, 0.5, 0.7) for k in range(1, 10)]          # whole quotients: the 1e-6
    (tmp_path / "cases.txt").write_text("\n".join(f"{r!r} {s!r}" for r, s in cases) + "\n")
    (tmp_path / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp")])
    out = subprocess.check_output([str(tmp_path / "t"), str(tmp_path / "cases.txt")]).decode().splitlines()
    assert len(out) == len(cases)
    for (r, s), line in zip(cases, out):
        h, w, clipped = line.split()
        ph, pw, pc = F.plan(r, s)
        assert (float(h), int(w), int(clipped)) == (ph, pw, int(pc)), (r, s, line)
        if (r, s) in PLANS:
            assert (pw, int(pc)) == PLANS[(r, s)], (r, s)
        assert pw <= F.MAX_STEPS and (pc or pw * ph >= r - 1e-6 * ph)        # the grid reaches the range unless it was cut
    for bad in ((2.0, -0.5), (0.0, 0.5), (-1.0, 0.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError):
            F.plan(*bad)


def test_pooling_weights_are_those_of_the_running_average():
    """Mode -2.1 (csp_cli.running_average) averages the BOXES of a particle's neighbouring frames with exp(-d^2 / (2 (hw / 2)^2)); frame
    refinement pools the score MAPS with the same weights.  Held against each other through the function itself: frames.pool of a stack of
    boxes, normalised on the background ring as running_average normalises its result, is what running_average returns."""
    find = np.array([0, 1, 2, 3, 4, 5, 6])
    for hw in (1, 2, 3, 10):
        w = F.pool_weights(find, hw)
        d = np.abs(find[:, None] - find[None, :])
        assert np.array_equal(w > 0, d <= hw) and np.allclose(np.diag(w), 1.0)
        assert np.array_equal(w, np.where(d <= hw, np.exp(-(d.astype(np.float64) ** 2) / (2 * (hw / 2.0) ** 2)), 0.0))
        rows = cistem.default_rows(7, 1.0, 300.0, 2.7, 0.07)
        rows[:, C["FIND"]], rows[:, C["PIND"]], rows[:, C["IMIND"]] = find, 0, 0
        rng = np.random.default_rng(hw)
        stack = rng.normal(0, 1, (7, 16, 16)).astype(np.float32)
        got = csp_cli.running_average(stack, rows, hw, 6.0)
        want = F.pool(stack, find, hw)                                # the same average, before running_average normalises it again
        yy, xx = np.mgrid[:16, :16]
        bg = ((yy - 8) ** 2 + (xx - 8) ** 2) > 36.0
        for j in range(7):
            b = want[j][bg]
            assert np.allclose(got[j], (want[j] - b.mean()) / b.std(), atol=2e-6)
    assert np.array_equal(F.pool_weights(find, 0), np.eye(7))
    gap = F.pool_weights([0, 1, 3, 4], 2)
    assert gap[0, 2] == 0 and gap[1, 2] == np.exp(-2.0) and gap[2, 3] == np.exp(-0.5)


def test_peak_rule_on_constructed_maps():
    h = 0.5
    jy, jx = np.mgrid[-4:5, -4:5].astype(np.float64)
    p = -((jx * h - 0.6) ** 2) - 2 * ((jy * h + 0.85) ** 2)          # a paraboloid: the three-point fit is exact
    q, dx, dy, curv = F.peak(p, h)
    assert q == (2 * 9 + 5) and abs(dx - 0.6) < 1e-12 and abs(dy + 0.85) < 1e-12 and curv[0] < 0 and curv[1] < 0
    p = -((jx * h - 3.1) ** 2) - ((jy * h) ** 2)                     # the maximum lies beyond the right edge: the edge point, no offset in x
    q, dx, dy, curv = F.peak(p, h)
    assert q % 9 == 8 and dx == 2.0 and np.isnan(curv[0]) and abs(dy) < 1e-12
    p = np.zeros((9, 9)); p[3, 2] = p[6, 6] = 1.0                    # a tie goes to the lower index; flat neighbours give a concave fit of offset 0
    assert F.peak(p, h)[:3] == (3 * 9 + 2, -1.0, -0.5)
    p = np.zeros((9, 9))                                             # all equal: index 0, a corner, no offsets
    assert F.peak(p, h)[:3] == (0, -2.0, -2.0)
    p = np.zeros((1, 1))                                             # W = 0
    assert F.peak(p, h)[:3] == (0, 0.0, 0.0)


def test_frame_series_tiles_the_tilt_series_and_plants_bounded_drifts():
    vol, imgs, rows, true = FC.series()
    assert imgs.shape == (84, 64, 64) and rows.shape == true.shape == (84, 32)
    assert np.array_equal(rows[:, C["POSITION_IN_STACK"]], np.arange(1, 85)) and np.array_equal(rows[:, C["FIND"]], np.tile(np.arange(7), 12))
    assert len(F.groups(rows)) == 12 and all(len(g) == 7 for g in F.groups(rows))
    _, _, rows0, _, _ = synth.make_tilt_series(64, 4, list(FC.TILTS), pixel=FC.PX, snr=FC.SNR, vol=vol)
    keep = [c for c in range(32) if c not in (C["POSITION_IN_STACK"], C["FIND"])]
    assert np.array_equal(rows[::7][:, keep], rows0[:, keep])
    d = (true[:, [C["X_SHIFT"], C["Y_SHIFT"]]] - rows[:, [C["X_SHIFT"], C["Y_SHIFT"]]]) / FC.PX
    assert np.abs(d).max() <= 0.9 + 0.5 * 0.5 + 1e-9 and np.abs(d).max() > 0.5
    assert np.allclose(true[:, [C["FSHIFT_X"], C["FSHIFT_Y"]]] / FC.PX, d)
    t = np.linspace(-1, 1, 7)
    for g in F.groups(rows)[:3]:
        for ax in range(2):                                         # a t + b (t^2 - 1/2): a quadratic fits it exactly
            assert np.abs(np.polyval(np.polyfit(t, d[g, ax], 2), t) - d[g, ax]).max() < 1e-9


def test_the_float64_reference_recovers_the_planted_drifts():
    """The condition on the inputs the GPU tests rest on (they tie the GPU rows to this reference): pooled over +-2 frames the reference's
    median shift error is below half the start's; no arg-max lies on the window's edge; at most 5 % of the rows are undecided."""
    vol, imgs, rows, true = FC.series()
    maps = FC.common_maps()
    start = np.median(FC.shift_error_px(rows, true))
    ref = FC.reference(rows, maps, 2)
    end = np.median(FC.shift_error_px(ref["rows_out"], true))
    print("median shift error: start %.3f px, reference at half_width 2 %.3f px" % (start, end))
    assert end < 0.5 * start
    for hw in (0, 2, 10):
        ref = FC.reference(rows, maps, hw)
        jy, jx = np.divmod(ref["index"], 9)
        assert not np.any((jy == 0) | (jy == 8) | (jx == 0) | (jx == 8))
        assert (ref["margin"] <= 2 * FC.tol(64)).mean() <= 0.05
        assert ref["refined"].all()
