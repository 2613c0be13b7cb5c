"""In which compass iterations k_local's full-band launch reuses the centre pose's taps is decided on the host, by one rule of
pyp_amd/csrc/ppm_geom.h (no HIP in it): near_move(), the voxels by which a neighbour pose moves the sample at the edge of the
iteration's band, against kNearMove.  with_schedule (host_refine.h) asks near_reuse_pays() per iteration with the step, the padding
factor and the marching band of that iteration.  A few lines of C++ with their own main are compiled against the header with the host
compiler under AddressSanitizer and UBSan and walk schedules the way with_schedule does; Python restates the rule independently."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_geom.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    printf("%.17g\n", ppm::kNearMove);
    double bf, rm, ha, hs, pad, rcap; int N, T, ang, sh;
    while (fscanf(f, "%lf %d %lf %lf %lf %d %d %lf %lf %d", &bf, &N, &rm, &ha, &hs, &ang, &sh, &pad, &rcap, &T) == 10) {
        unsigned bits = 0;
        for (int t = 0; t < T; t++) {              // with_schedule's loop
            const double rb = ppm::march_band(bf, N, rm, ha, hs, ang != 0, sh != 0, rcap);
            if (ppm::near_reuse_pays(ang != 0, ha, pad, rb)) bits |= 1u << t;
            ha *= 0.5; hs *= 0.5;
        }
        printf("%u\n", bits);
    }
    fclose(f);
    return 0;
}
'''

# name: band factor, box, mask radius (px), first angle step (deg), first shift step (px), any angle free, any shift free, padding, band cap (px), iterations
CASES = {
    "headline: final launch after two hit iterations at 15 degrees": (3.0, 256, 82.0, 1.875, 0.5, 1, 1, 1.0, 64.0, 7),
    "rows launch at the default steps": (3.0, 64, 25.6, 2.5, 2.0, 1, 1, 1.0, 24.0, 9),
    "marching off, 20 degrees": (-1.0, 64, 25.6, 20.0, 2.0, 1, 1, 1.0, 24.0, 9),
    "marching off, padding 4": (-1.0, 64, 25.6, 2.5, 2.0, 1, 1, 4.0, 24.0, 9),
    "padding 2 under marching": (3.0, 64, 25.6, 2.5, 2.0, 1, 1, 2.0, 24.0, 9),
    "0.02 degrees": (3.0, 64, 25.6, 0.02, 2.0, 1, 1, 1.0, 24.0, 9),
    "no free angle": (3.0, 64, 25.6, 2.5, 2.0, 0, 1, 1.0, 24.0, 9),
    "angles only": (3.0, 128, 40.0, 5.0, 1.0, 1, 0, 1.0, 48.0, 12),
    "all 24 iterations": (3.0, 256, 82.0, 40.0, 8.0, 1, 1, 1.0, 96.0, 24),
}


def band(bf, n, rm, ha, hs, ang, sh, rcap):
    """march_band of ppm_geom.h"""
    d = rm * math.radians(ha) if ang else 0.0
    if sh and hs > d:
        d = hs
    if bf < 0 or not d > 0:
        return rcap
    return min(max(bf * n / (2 * math.pi * d), 4.0), rcap)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reuse_rule")
    names = list(CASES)
    (tmp / "cases.txt").write_text("".join(" ".join(str(v) for v in CASES[k]) + "\n" for k in names))
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().splitlines()
    assert len(out) == len(names) + 1
    return float(out[0]), {k: int(line) for k, line in zip(names, out[1:])}


@pytest.mark.parametrize("name", list(CASES))
def test_iterations_that_reuse(answers, name):
    limit, got = answers
    bf, n, rm, ha, hs, ang, sh, pad, rcap, T = CASES[name]
    want = 0
    for t in range(T):
        move = math.radians(ha) * pad * band(bf, n, rm, ha, hs, ang, sh, rcap)      # voxels at the band's edge
        if ang and move <= limit:
            want |= 1 << t
        ha, hs = ha / 2, hs / 2
    assert got[name] == want


def test_the_limit_and_what_follows_from_it(answers):
    limit, got = answers
    assert 0.25 <= limit <= 2.0                   # beyond two voxels nothing stays in a cell; a quarter voxel keeps four lanes of five
    assert got["no free angle"] == 0              # a single group per sweep
    assert got["0.02 degrees"] == (1 << 9) - 1
    # once an iteration reuses, every later one does: the steps halve and the band stops growing at its cap
    for name, bits in got.items():
        T = CASES[name][-1]
        first = next((t for t in range(T) if bits >> t & 1), T)
        assert bits == ((1 << T) - 1) & ~((1 << first) - 1), name
    assert got["marching off, 20 degrees"] & 1 == 0 and got["marching off, 20 degrees"] >> 8 & 1 == 1     # 8.4 voxels, then 0.03
