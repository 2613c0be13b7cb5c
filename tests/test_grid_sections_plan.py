"""The sections of the grid search are planned by one function, plan_sections of pyp_amd/csrc/ppm_sections.h (no HIP in it): contiguous
ranges of whole grid directions, each with a bank4 below 4 GB and all its banks within a byte budget.  A few lines of C++ with their
own main are compiled against the header with the host compiler under AddressSanitizer and UBSan and run over a table of cases; every
plan is checked here: contiguous, ascending, every direction once, inside both limits, and no more sections than the limits ask for."""
import math
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_sections.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int n_dir, npsi;
    unsigned long long b, b4, budget;
    while (fscanf(f, "%d %d %llu %llu %llu", &n_dir, &npsi, &b, &b4, &budget) == 5) {
        std::vector<ppm::GridSection> s;
        std::string err;
        if (!ppm::plan_sections(n_dir, npsi, b, b4, budget, s, err)) { printf("ERR %s\n", err.c_str()); continue; }
        printf("OK");
        for (const ppm::GridSection &g : s) printf(" %d %d", g.d0, g.nd);
        printf("\n");
    }
    fclose(f);
    return 0;
}
'''

GB4 = 1 << 32
UNLIMITED = 1 << 62


def grid_counts(step, phi_max=360.0, theta_max=180.0):
    """Directions and stored in-plane slices per direction of the global grid."""
    n_theta = max(2, int(math.floor(theta_max / step + 0.5)) + 1)
    n_dir = sum(max(1, int(math.floor(phi_max * math.sin(math.radians(theta_max * i / (n_theta - 1))) / step + 0.5))) for i in range(n_theta))
    n_psi = max(1, int(math.floor(360.0 / step + 0.5)))
    return n_dir, (n_psi // 2 if n_psi % 2 == 0 else n_psi)


def cases():
    c = []
    per = 12 * (1000 + 500)                                   # bytes of one direction: 12 stored slices in both banks
    c.append(("everything fits", 100, 12, 1000, 500, UNLIMITED, 1))
    c.append(("the whole grid exactly", 100, 12, 1000, 500, 100 * per, 1))
    c.append(("one byte short of the whole grid", 100, 12, 1000, 500, 100 * per - 1, 2))
    c.append(("exactly 7 directions", 100, 12, 1000, 500, 7 * per, 15))
    c.append(("one byte short of 7 directions", 100, 12, 1000, 500, 7 * per - 1, 17))
    c.append(("one byte more than 7 directions", 100, 12, 1000, 500, 7 * per + 1, 15))
    c.append(("exactly one direction", 100, 12, 1000, 500, per, 100))
    c.append(("below one direction", 100, 12, 1000, 500, per - 1, None))
    n_dir, npsi = grid_counts(24.0)                           # 15 in-plane angles: odd, every one stored
    assert npsi == 15
    c.append(("odd in-plane count", n_dir, npsi, 4096, 0, 3 * npsi * 4096 + 5, -(-n_dir // 3)))
    c.append(("odd in-plane count, one direction each", n_dir, npsi, 4096, 1024, npsi * 5120, n_dir))
    c.append(("k_global's bank alone, past 4 GB in one section", 3000, 40, 66560, 0, UNLIMITED, 1))
    n_dir, npsi = grid_counts(4.5)                            # 256^2, search band > 32 px: L = 64, 64 KB per slice in either bank
    assert n_dir * npsi > 65536
    c.append(("4 GB rule alone at 4.5 degrees, L = 64", n_dir, npsi, 128 * 64 * 8, 64 * 64 * 16, UNLIMITED, 2))
    c.append(("one direction of bank4 at 4 GB", 10, 65536, 0, 65536, UNLIMITED, None))
    c.append(("one direction of bank4 just below 4 GB", 10, 65535, 0, 65536, UNLIMITED, 10))
    return c


def test_sections_are_contiguous_cover_the_grid_and_stay_inside_both_limits(tmp_path):
    table = cases()
    (tmp_path / "cases.txt").write_text("".join("%d %d %d %d %d\n" % c[1:6] for c in table))
    (tmp_path / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp_path / "t"), str(tmp_path / "t.cpp")])
    out = subprocess.check_output([str(tmp_path / "t"), str(tmp_path / "cases.txt")]).decode().splitlines()
    assert len(out) == len(table)
    for (name, n_dir, npsi, b, b4, budget, want), line in zip(table, out):
        if want is None:
            assert line.startswith("ERR ") and "angular step" in line, (name, line)
            continue
        assert line.startswith("OK "), (name, line)
        v = [int(x) for x in line.split()[1:]]
        secs = list(zip(v[0::2], v[1::2]))
        assert len(secs) == want, (name, len(secs))
        nxt = 0
        for d0, nd in secs:
            assert d0 == nxt and nd >= 1, (name, secs)
            assert nd * npsi * (b + b4) <= budget, (name, d0, nd)
            assert nd * npsi * b4 < GB4, (name, d0, nd)
            nxt = d0 + nd
        assert nxt == n_dir, (name, secs)
        assert max(nd for _, nd in secs) - min(nd for _, nd in secs) <= 1, (name, secs)      # even: one allocation serves them all
