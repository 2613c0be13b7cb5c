"""The exhaustive particle search of the constrained refinement is planned by one header, pyp_amd/csrc/ppm_csp_search.h (no HIP in it):
the grid step, the coarse band and the candidate counts for a budget of points.  A few lines of C++ with their own
main are compiled against it with the host compiler under AddressSanitizer and UBSan and run over a table of cases; every plan is held to
the restatement of the rule written here and to what the rule promises whatever its text: the product fits the budget, the next finer
step would not (or the band has reached its cap), the angles hold 0 and the shift grid spans exactly +-tolerance.
A second case follows the key csp_NumberOfRandomIterations from a .pyp_config.toml into CspCfg."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_csp_search.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    double ta[3], ts, rm, bf, rhi; int rot, trans, N, K; long P;
    while (fscanf(f, "%lf %lf %lf %d %lf %d %lf %d %lf %lf %ld %d", &ta[0], &ta[1], &ta[2], &rot, &ts, &trans, &rm, &N, &bf, &rhi, &P, &K) == 12) {
        const ppm_csp_search_info G = ppm::csp_search_make(ta, rot != 0, ts, trans != 0, rm, N, bf, rhi, P, K);
        printf("%d %d %.17g %.17g %.17g %d %d %d %d %d %d %d %ld %ld %d", G.active, G.shift_grid, G.step, G.r_g, G.h_s, G.n_angle[0], G.n_angle[1], G.n_angle[2],
               G.full_turn[0], G.full_turn[1], G.full_turn[2], G.n_shift_axis, G.n_rot, G.n_shift, G.n_candidates);
        for (int k = 0; k < 3; k++) { printf(" |"); for (int i = 0; i < G.n_angle[k]; i++) printf(" %.17g", ppm::csp_search_angle(G.n_angle[k], G.full_turn[k], G.step, i)); }
        printf(" |"); for (int i = 0; i < G.n_shift_axis; i++) printf(" %.17g", ppm::csp_search_shift(G.n_shift_axis, G.tol_shift, i));
        double d[6]; ppm::csp_search_delta(G, G.n_rot - 1, G.n_shift - 1, d);           // the last point of both enumerations, and one inside
        printf(" |"); for (int k = 0; k < 6; k++) printf(" %.17g", d[k]);
        ppm::csp_search_delta(G, G.n_rot / 3, G.n_shift / 3, d);
        printf(" |"); for (int k = 0; k < 6; k++) printf(" %.17g", d[k]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
'''

STEPS = (30, 24, 20, 18, 15, 12, 10, 9, 8, 7.5, 6, 5, 4, 3, 2.5, 2, 1.5, 1)
BAND_CAP = 32.0


def march_band(bf, n, rm_px, ha, rcap):
    """ppm_geom.h march_band for an angular probe alone."""
    if bf < 0:
        return rcap
    d = rm_px * ha * math.pi / 180.0
    if not d > 0:
        return rcap
    return min(max(bf * n / (2.0 * math.pi * d), 4.0), rcap)


def counts(tol, rot, tol_shift, trans, rm_px, step):
    n_angle, full = [], []
    for k in range(3):
        n, f = 1, 0
        if rot and tol[k] > 0:
            t = min(tol[k], 90.0 if k == 1 else 180.0)
            if k != 1 and t >= 180.0:
                n, f = int(math.floor(360.0 / step + 0.5)), 1
            else:
                n = 2 * int(math.floor(t / step + 1e-9)) + 1
        n_angle.append(n); full.append(f)
    h_s = rm_px * step * math.pi / 180.0
    ns = 1
    if trans and tol_shift > 0:
        ns = 2 * max(1, int(math.ceil(tol_shift / h_s - 1e-9))) + 1
    return n_angle, full, h_s, ns


def plan(tol, rot, tol_shift, trans, rm_px, n, bf, r_hi, points, cand):
    """The rule of DESIGN.md section 8, restated: (active, shift_grid, step, r_g, h_s, n_angle, full, n_shift_axis, K)."""
    rcap = min(r_hi, BAND_CAP)
    best = None
    if points > 0:
        for step in STEPS:
            na, fu, h_s, ns = counts(tol, rot, tol_shift, trans, rm_px, step)
            r_g = march_band(bf, n, rm_px, step / 2, rcap)
            if na[0] * na[1] * na[2] * ns ** 3 <= points:
                best = (1, int(ns > 1), step, r_g, h_s, na, fu, ns)
            if r_g >= rcap:
                break
        if best is None:
            na, fu, h_s, ns = counts(tol, rot, tol_shift, False, rm_px, 30)
            best = (int(na[0] * na[1] * na[2] <= points), 0, 30, march_band(bf, n, rm_px, 15.0, rcap), h_s, na, fu, 1)
    if best is None or not best[0]:
        return (0,) + (best[1:] if best else (0, 0, 0, 0, [1, 1, 1], [0, 0, 0], 1)) + (0,)
    k = min(cand if cand > 0 else 8, 32, best[5][0] * best[5][1] * best[5][2])
    return best + (k,)


def cases():
    c = []
    # the two tutorial settings: docs/cli/tomography.rst (box 192, 2.7 A/px, radius 150 A, tolerances 30 / 10 / 10 degrees and 50 A,
    # 50 000 points) and docs/cli/classification.rst (all rotations 180 degrees, 5 000 000 points; box 64 here)
    c.append(("tomography tutorial", (30, 10, 10), 1, float(np.float32(50.0 / 2.7)), 1,      # (ppm_csp_cfg carries the tolerances as floats)
              150.0 / 2.7, 192, 3.0, 192 * 2.7 / 8.0, 50000, 0))
    c.append(("classification tutorial", (180, 180, 180), 1, 4.0, 1, 25.6, 64, 3.0, 24.0, 5000000, 0))
    c.append(("the GPU test's plan", (180, 180, 180), 1, 4.0, 1, 25.6, 64, 3.0, 24.0, 250000, 0))
    c.append(("too small for 30 degrees with shifts: the shift grid goes", (180, 180, 180), 1, 4.0, 1, 25.6, 64, 3.0, 24.0, 2000, 0))
    c.append(("too small for 30 degrees at all: no exhaustive stage", (180, 180, 180), 1, 4.0, 1, 25.6, 64, 3.0, 24.0, 500, 0))
    c.append(("translations off", (20, 0, 20), 1, 4.0, 0, 25.6, 64, 3.0, 24.0, 250000, 0))
    c.append(("one axis off", (40, 0, 40), 1, 6.0, 1, 25.6, 64, 3.0, 24.0, 100000, 4))
    c.append(("rotations off", (30, 30, 30), 0, 10.0, 1, 25.6, 64, 3.0, 24.0, 30000, 0))
    c.append(("a tolerance below every step that fits", (0.5, 60, 3), 1, 2.0, 1, 40.0, 128, 3.0, 40.0, 20000, 100))
    c.append(("the band cap ends the list", (5, 5, 5), 1, 1.0, 1, 25.6, 64, 3.0, 24.0, 10 ** 9, 0))
    c.append(("no marching: 30 degrees at the cap", (180, 90, 180), 1, 3.0, 1, 25.6, 64, -1.0, 24.0, 10 ** 9, 0))
    c.append(("no budget", (30, 30, 30), 1, 5.0, 1, 25.6, 64, 3.0, 24.0, 0, 0))
    return c


def test_plan_fits_the_budget_and_the_next_finer_step_would_not(tmp_path):
    table = cases()
    (tmp_path / "cases.txt").write_text("".join("%r %r %r %d %r %d %r %d %r %r %d %d\n" % (tuple(float(x) for x in c[1]) + (c[2], float(c[3]), c[4], float(c[5]), c[6], float(c[7]), float(c[8]), c[9], c[10]))
                                                for c in table))
    (tmp_path / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp")])
    out = subprocess.check_output([str(tmp_path / "t"), str(tmp_path / "cases.txt")]).decode().splitlines()
    assert len(out) == len(table)
    seen_steps = set()
    for (name, tol, rot, ts, trans, rm, n, bf, rhi, points, cand), line in zip(table, out):
        parts = [p.split() for p in line.split("|")]
        h = parts[0]
        active, shift_grid, step, r_g, h_s = int(h[0]), int(h[1]), float(h[2]), float(h[3]), float(h[4])
        n_angle, full, ns, n_rot, n_shift, k = [int(x) for x in h[5:8]], [int(x) for x in h[8:11]], int(h[11]), int(h[12]), int(h[13]), int(h[14])
        want = plan(tol, rot, ts, trans, rm, n, bf, rhi, points, cand)
        assert active == want[0], name
        if not active:
            assert k == 0 and (points == 0 or n_rot > points), (name, line)
            continue
        assert (shift_grid, step, n_angle, full, ns, k) == (want[1], want[2], want[5], want[6], want[7], want[8]), (name, line, want)
        assert abs(r_g - want[3]) <= 1e-12 * r_g and abs(h_s - want[4]) <= 1e-12 * h_s, (name, line, want)
        assert n_rot == n_angle[0] * n_angle[1] * n_angle[2] and n_shift == ns ** 3
        seen_steps.add(step)
        # inside the budget, and the next finer entry is not (or the band is at its cap)
        assert n_rot * n_shift <= points, name
        rcap = min(rhi, BAND_CAP)
        assert r_g <= rcap
        i = STEPS.index(step)
        if shift_grid or not (trans and ts > 0):
            if i + 1 < len(STEPS) and r_g < rcap:
                na2, _, _, ns2 = counts(tol, rot, ts, trans, rm, STEPS[i + 1])
                assert na2[0] * na2[1] * na2[2] * ns2 ** 3 > points, (name, STEPS[i + 1])
        else:                       # the shift grid was dropped: 30 degrees with it did not fit
            assert step == 30
            na2, _, _, ns2 = counts(tol, rot, ts, trans, rm, 30)
            assert na2[0] * na2[1] * na2[2] * ns2 ** 3 > points, name
        # the angles: 0 among them, inside the tolerance, equally spaced; a full turn closes on itself
        for kx in range(3):
            ang = [float(x) for x in parts[1 + kx]]
            assert len(ang) == n_angle[kx] and 0.0 in ang, (name, kx)
            if full[kx]:
                assert ang[0] == 0.0 and abs(ang[-1] + 360.0 / len(ang) - 360.0) < 1e-9
            else:
                lim = min(tol[kx], 90.0 if kx == 1 else 180.0) if rot else 0.0
                assert max(abs(a) for a in ang) <= lim + 1e-9 and (len(ang) == 1 or max(abs(a) for a in ang) > lim - step)
            assert all(abs(ang[j + 1] - ang[j] - (ang[1] - ang[0])) < 1e-9 for j in range(len(ang) - 1))
        # the shifts: exactly +-tolerance at the ends, 0 in the middle, no wider apart than the step the rule asks for
        sh = [float(x) for x in parts[4]]
        assert len(sh) == ns
        if ns > 1:
            assert sh[0] == -ts and sh[-1] == ts and sh[ns // 2] == 0.0 and sh[1] - sh[0] <= h_s + 1e-9, (name, sh)
        else:
            assert sh == [0.0]
        # the enumeration: the first axis slowest
        last, mid = [float(x) for x in parts[5]], [float(x) for x in parts[6]]
        ax = [[float(x) for x in parts[1 + kx]] for kx in range(3)]
        assert last == [ax[0][-1], ax[1][-1], ax[2][-1], sh[-1], sh[-1], sh[-1]]
        r, s = n_rot // 3, n_shift // 3
        assert mid == [ax[0][r // (n_angle[1] * n_angle[2])], ax[1][(r // n_angle[2]) % n_angle[1]], ax[2][r % n_angle[2]],
                       sh[s // (ns * ns)], sh[(s // ns) % ns], sh[s % ns]]
    by_name = {c[0]: l for c, l in zip(table, out)}
    assert by_name["tomography tutorial"].split()[2] == "7.5" and by_name["classification tutorial"].split()[2] == "9"
    g = by_name["the GPU test's plan"].split()
    assert g[2] == "15" and g[5:8] == ["24", "13", "24"] and g[12:14] == ["7488", "27"] and 84 > float(g[3]) ** 2 > 82
    assert len(seen_steps) >= 5


def test_the_budget_travels_from_the_config_file_to_the_refinement_settings(tmp_path):
    """csp_NumberOfRandomIterations of .pyp_config.toml, resolved through its schedule, arrives in CspCfg.search_points in the particle
    modes; the tilt modes and mode 4 ignore it."""
    from pyp_amd.abi import CSP_MICROGRAPHS, CSP_PARTICLES, CspCfg
    from pyp_amd.surface import csp_cli
    base = ('data_set = "tomo"\nscope_pixel = 2.0\nextract_box = 64\nparticle_rad = 51.2\nrefine_rhref = "5.3333333:4"\n'
            'csp_ToleranceParticlesPsi = 180.0\ncsp_ToleranceParticlesTheta = 180.0\ncsp_ToleranceParticlesPhi = 180.0\ncsp_ToleranceParticlesShifts = 8.0\n')
    for it, text, want in ((2, 'csp_NumberOfRandomIterations = 50000\ncsp_GridSearch = true\n', 50000), (2, 'csp_NumberOfRandomIterations = "5000000:0"\n', 5000000),
                           (3, 'csp_NumberOfRandomIterations = "5000000:0"\ncsp_GridSearch = false\n', 0), (2, '', 0)):
        (tmp_path / ".pyp_config.toml").write_text(base + f"refine_iter = {it}\n" + text)
        s = csp_cli._settings(csp_cli.read_flat_toml(str(tmp_path / ".pyp_config.toml")))
        assert s["search_points"] == want
        for mode in (1, 2, 5):
            cc = csp_cli.make_csp_cfg(s, mode, 0, -1, 2.0)
            assert cc.unit == CSP_PARTICLES and cc.search_points == want and cc.search_candidates == 0 and abs(cc.tol_shift - 4.0) < 1e-6
        for mode in (0, 3, 4, 6):
            cc = csp_cli.make_csp_cfg(s, mode, 0, -1, 2.0)
            assert cc.unit == CSP_MICROGRAPHS and cc.search_points == 0
    # the two fields sit at the end of the structure: what came before them keeps its place
    names = [f[0] for f in CspCfg._fields_]
    assert names[-2:] == ["search_points", "search_candidates"] and names[-3] == "defocus_step"
    assert CspCfg.make(CSP_PARTICLES).search_points == 0 and CspCfg.make(CSP_PARTICLES, search_points=7, search_candidates=3).search_candidates == 3
