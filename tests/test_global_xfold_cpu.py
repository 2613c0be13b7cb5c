"""k_global sums the register-held shift window of a full-wave slice over kx with the columns kx and kx + 32 folded first; where a lane's
value sits in the window is defined once, in pyp_amd/csrc/ppm_window.h (no HIP in it), which the kernel's tail and its arg-max go
through.  A few lines of C++ with their own main are compiled against the header with the host compiler under AddressSanitizer and
UBSan and print the mapping of every lane for R = 1, 2, 3; checked here: the valid (value index, half) pairs map one to one onto the
(2R+1)^2 window, the order key is iy * NS + ix, the upper half of the unpaired last row and every index beyond the values are invalid,
and the limits RSx / RSy cut the window as the kernel's other branches do.  A float64 numpy check restates the fold (S, D, P, Q and
the twiddles of column l < 32) and compares it with the direct sum over the 64 columns."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_window.h"
int main() {
    for (int R = 1; R <= 3; R++) {
        printf("WIN %d %d %d\n", R, ppm::win_slots(R), ppm::win_values(R));
        for (int lane = 0; lane < 64; lane++) {
            int iy = -1, ix = -1;
            const int vi = ppm::win_lane_value(lane), half = ppm::win_lane_half(lane);
            const bool ok = ppm::win_pos(R, vi, half, iy, ix);
            printf("LANE %d %d %d %d %d %d %d\n", lane, vi, half, ok ? 1 : 0, iy, ix, ok ? ppm::win_key(R, iy, ix) : -1);
        }
        for (int RSx = 0; RSx <= R; RSx++)
            for (int RSy = 0; RSy <= R; RSy++)
                for (int lane = 0; lane < 64; lane++) {
                    int iy = -1, ix = -1;
                    const bool ok = ppm::win_valid(R, ppm::win_lane_value(lane), ppm::win_lane_half(lane), RSx, RSy, iy, ix);
                    printf("CUT %d %d %d %d\n", RSx, RSy, lane, ok ? 1 : 0);
                }
        // indices no lane may claim
        int iy = 0, ix = 0;
        const int bad[] = { -1, ppm::win_values(R), ppm::win_values(R) + 1, 31, 32, 63, 64 };
        for (int b : bad) if (b < 0 || b >= ppm::win_values(R)) printf("BEYOND %d %d %d\n", b, ppm::win_pos(R, b, 0, iy, ix) ? 1 : 0, ppm::win_pos(R, b, 1, iy, ix) ? 1 : 0);
    }
    return 0;
}
'''


def bitrev5(x):
    return int("{:05b}".format(x)[::-1], 2)


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{R: (slots, values, lanes, cuts, beyond)}; lanes = [(vi, half, ok, iy, ix, key)] by lane, cuts = {(RSx, RSy): [ok by lane]}"""
    tmp = tmp_path_factory.mktemp("xfold")
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    res, cur = {}, None
    for line in subprocess.check_output([str(tmp / "t")]).decode().splitlines():
        v = line.split()
        n = [int(x) for x in v[1:]]
        if v[0] == "WIN":
            cur = res[n[0]] = (n[1], n[2], [], {}, [])
        elif v[0] == "LANE":
            assert n[0] == len(cur[2])
            cur[2].append((n[1], n[2], n[3] == 1, n[4], n[5], n[6]))
        elif v[0] == "CUT":
            cur[3].setdefault((n[0], n[1]), []).append(n[3] == 1)
            assert len(cur[3][(n[0], n[1])]) == n[2] + 1
        else:
            assert v[0] == "BEYOND"
            cur[4].append(tuple(n))
    assert sorted(res) == [1, 2, 3]
    return res


@pytest.mark.parametrize("R", [1, 2, 3])
def test_valid_lanes_map_one_to_one_onto_the_window(maps, R):
    slots, values, lanes, _, beyond = maps[R]
    NS = 2 * R + 1
    assert slots == R + 1 and values == slots * NS and values <= 32              # one output register pair per half
    assert len(lanes) == 64
    seen = {}
    for lane, (vi, half, ok, iy, ix, key) in enumerate(lanes):
        assert vi == bitrev5(lane & 31) and half == lane >> 5                    # what the halving reduction leaves in this lane
        slot = vi // NS
        want_ok = vi < values and 2 * slot + half < NS
        assert ok == want_ok, (lane, vi, half)
        if ok:
            assert (iy, ix) == (2 * slot + half, vi - slot * NS)
            assert 0 <= iy < NS and 0 <= ix < NS
            assert key == iy * NS + ix                                           # the arg-max order: the scan order of the window
            assert (iy, ix) not in seen, (lane, seen[(iy, ix)])
            seen[(iy, ix)] = lane
    assert sorted(seen) == [(iy, ix) for iy in range(NS) for ix in range(NS)]    # a bijection onto the (2R+1)^2 window
    # the unpaired last row: its slot is valid in the lower half only
    for lane, (vi, half, ok, _, _, _) in enumerate(lanes):
        if vi < values and vi // NS == R:
            assert ok == (half == 0), lane
    assert beyond and all(lo == 0 and hi == 0 for _, lo, hi in beyond)           # every index beyond the values is invalid


@pytest.mark.parametrize("R", [1, 2, 3])
def test_window_limits_cut_rows_and_columns(maps, R):
    _, _, lanes, cuts, _ = maps[R]
    assert sorted(cuts) == [(x, y) for x in range(R + 1) for y in range(R + 1)]
    for (RSx, RSy), oks in cuts.items():
        n = 0
        for lane, ok in enumerate(oks):
            _, _, pos, iy, ix, _ = lanes[lane]
            assert ok == (pos and abs(ix - R) <= RSx and abs(iy - R) <= RSy), (RSx, RSy, lane)
            n += ok
        assert n == (2 * RSx + 1) * (2 * RSy + 1)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_folded_columns_equal_the_direct_sum(R):
    """sum over kx = 0 .. 63 of Re(G(kx) e^{i jx theta kx}), theta = 2 pi / 128, from the fold of columns l and l + 32 as the kernel's
    tail forms it — S_x; D_x c2 -+ D_y s2; P / Q with c1, s1 and c3, s3 — against the direct sum, in float64."""
    rng = np.random.default_rng(7 + R)
    G = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    th = 2 * np.pi / 128
    g, h = G[:32], G[32:]
    gx, gy, hx, hy = g.real, g.imag, h.real, h.imag
    Sx, Dx, Dy = gx + hx, gx - hx, gy - hy
    Px, Py, Qx, Qy = gx - hy, gy + hx, gx + hy, gy - hx
    l = np.arange(32)
    got = {0: Sx.sum()}
    for j in range(1, R + 1):
        c, s = np.cos(j * th * l), np.sin(j * th * l)
        if j == 2:
            got[j], got[-j] = (Dx * c - Dy * s).sum(), (Dx * c + Dy * s).sum()
        else:
            (px, py), (mx, my) = ((Px, Py), (Qx, Qy)) if j == 1 else ((Qx, Qy), (Px, Py))
            got[j], got[-j] = (px * c - py * s).sum(), (mx * c + my * s).sum()
    kx = np.arange(64)
    for jx in range(-R, R + 1):
        want = (G * np.exp(1j * jx * th * kx)).real.sum()
        assert abs(got[jx] - want) < 1e-12, (jx, abs(got[jx] - want))
