"""When ppm_refine_batch runs the hit stage of a chunk beside the grid search of the next one is decided by one rule,
pyp_amd/csrc/ppm_overlap.h (no HIP in it): how many hit-stage blocks fit on a CU beside one k_global block, from the two kernels'
registers and LDS and the CU's, and which calls overlap at all.  A few lines of C++ with their own main are compiled against the header
with the host compiler under AddressSanitizer and UBSan and run over a table of cases."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_overlap.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int hv, ht, tv, tt, gs, fft, tiles, secs, chunks, hit, off;
    long hl, tl;
    while (fscanf(f, "%d %d %ld %d %d %ld %d %d %d %d %d %d %d", &hv, &ht, &hl, &tv, &tt, &tl, &gs, &fft, &tiles, &secs, &chunks, &hit, &off) == 13) {
        const ppm::OverlapKernel host = { hv, ht, hl }, tenant = { tv, tt, tl };
        const ppm::OverlapDevice dev = { 512, 4, 160 * 1024, 8, 1280 };          // gfx950
        const ppm::OverlapCall call = { gs != 0, fft != 0, tiles, secs, chunks, hit != 0, off != 0 };
        const int n = ppm::overlap_tenants(host, tenant, dev);
        printf("%d %d\n", n, ppm::overlap_on(n, call) ? 1 : 0);
    }
    fclose(f);
    return 0;
}
'''

KB = 1024
GLOBAL = (168, 512, 128 * KB)           # k_global<3, true, false>: 8 waves x 168 VGPRs, W tables of two particles
HIT = (128, 64, 6 * KB + 512)           # a one-wave k_local<true> block with address tables of the search band
PLAIN = (1, 0, 1, 1, 2, 1, 0)           # a k_global search of one tile and one section, two chunks, hits refined, the knob not set

# name: (k_global, hit stage, call) -> (blocks beside a k_global block, overlap used)
CASES = {
    "headline": (GLOBAL, HIT, PLAIN, (4, 1)),
    "tables of the full band": (GLOBAL, (128, 64, 9 * KB), PLAIN, (3, 1)),
    "k_global at 233 registers": ((233, 512, 128 * KB), HIT, PLAIN, (0, 0)),
    "hit stage beyond the LDS left": (GLOBAL, (128, 64, 40 * KB), PLAIN, (0, 0)),
    "k_global alone over a CU's LDS": ((168, 512, 161 * KB), HIT, PLAIN, (0, 0)),
    "two-wave hit stage": (GLOBAL, (128, 128, 10 * KB), PLAIN, (2, 1)),
    "hit stage too wide for the registers left": (GLOBAL, (184, 64, 6 * KB), PLAIN, (0, 0)),
    "small k_global, registers decide": ((96, 512, 16 * KB), HIT, PLAIN, (8, 1)),
    "nothing known of a kernel": ((0, 512, 128 * KB), HIT, PLAIN, (0, 0)),
    "one chunk": (GLOBAL, HIT, (1, 0, 1, 1, 1, 1, 0), (4, 0)),
    "three chunks": (GLOBAL, HIT, (1, 0, 1, 1, 3, 1, 0), (4, 1)),
    "k_gfft": (GLOBAL, HIT, (1, 1, 1, 1, 2, 1, 0), (4, 0)),
    "tiles": (GLOBAL, HIT, (1, 0, 4, 1, 2, 1, 0), (4, 0)),
    "sections": (GLOBAL, HIT, (1, 0, 1, 2, 2, 1, 0), (4, 0)),
    "no grid search": (GLOBAL, HIT, (0, 0, 1, 1, 2, 1, 0), (4, 0)),
    "hits kept at their grid points": (GLOBAL, HIT, (1, 0, 1, 1, 2, 0, 0), (4, 0)),
    "PPM_REFINE_OVERLAP=0": (GLOBAL, HIT, (1, 0, 1, 1, 2, 1, 1), (4, 0)),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("overlap")
    names = list(CASES)
    (tmp / "cases.txt").write_text("".join(" ".join(str(v) for v in CASES[k][0] + CASES[k][1] + CASES[k][2]) + "\n" for k in names))
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().splitlines()
    assert len(out) == len(names)
    return {k: tuple(int(x) for x in line.split()) for k, line in zip(names, out)}


@pytest.mark.parametrize("name", list(CASES))
def test_blocks_beside_k_global_and_when_the_overlap_is_used(answers, name):
    assert answers[name] == CASES[name][3]
