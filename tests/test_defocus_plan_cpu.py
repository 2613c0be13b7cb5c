"""The two host rules of the defocus refinement live in pyp_amd/csrc/ppm_defocus_plan.h (no HIP in it): the number of offsets either
side from (range, step), with the cap and the 1e-6, and the offsets one pass of k_defocus scores from (nt, nrings) and the test knob
PPM_DEFOCUS_CHUNK.  A few lines of C++ with their own main are compiled against the header with the host compiler under
AddressSanitizer and UBSan and run over a table of cases; the Python mirror the GPU tests plan with (tests/defocus_cases.py) is held
to the same answers."""
import os
import subprocess

import pytest

import defocus_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_defocus_plan.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 's') {              // range step -> steps as the refinement forms them (float / float), as csp does (float / double)
            float range, step;
            if (fscanf(f, "%f %f", &range, &step) != 2) return 3;
            printf("%d %d\n", ppm::defocus_steps(range, step, 20), ppm::defocus_steps(range, (double)step, 20));
        } else {                        // nt nrings knob -> offsets per pass, passes
            int nt, nrings; long knob;
            if (fscanf(f, "%d %d %ld", &nt, &nrings, &knob) != 3) return 3;
            const int tc = ppm::defocus_chunk(nt, nrings, knob);
            printf("%d %d\n", tc, ppm::defocus_chunks(nt, tc));
        }
    }
    fclose(f);
    return 0;
}
'''

# (range, step) -> nt; 0: no search
STEPS = {
    (400.0, 50.0): 8, (500.0, 50.0): 10, (750.0, 50.0): 15, (1050.0, 100.0): 10,
    (0.3, 0.1): 3,                      # 2.9999999 as a quotient: through the 1e-6
    (49.999, 50.0): 0, (5000.0, 50.0): 20, (5000.0, 100.0): 20, (400.0, 0.0): 0, (400.0, -50.0): 0,
    (850.0, 50.0): 17, (1000.0, 50.0): 20, (100.0, 33.3): 3, (50.0, 50.0): 1, (0.0, 50.0): 0, (-100.0, 50.0): 0,
}
# (T, nrings, knob) -> offsets per pass
CHUNKS = {
    (41, 97, 0): 38, (41, 121, 0): 30, (31, 121, 0): 30, (21, 193, 0): 19, (17, 33, 0): 17, (41, 3751, 0): 1,
    (41, 32, 1): 1, (41, 32, 7): 7, (41, 32, 32): 32, (41, 32, 33): 33, (41, 32, 100): 41,          # the knob lowers ...
    (41, 97, 40): 38, (41, 97, 7): 7, (41, 97, -3): 38, (1, 32, 0): 1, (1, 32, 5): 1,                # ... and never raises
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("defocus_plan")
    lines = [f"s {r!r} {s!r}" for r, s in STEPS] + [f"c {(T - 1) // 2} {nr} {knob}" for T, nr, knob in CHUNKS]
    (tmp / "cases.txt").write_text("\n".join(lines) + "\n")
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().splitlines()
    assert len(out) == len(lines)
    got = [tuple(int(x) for x in line.split()) for line in out]
    return dict(zip(STEPS, got[:len(STEPS)])), dict(zip(CHUNKS, got[len(STEPS):]))


@pytest.mark.parametrize("case", list(STEPS), ids=lambda c: f"{c[0]}/{c[1]}")
def test_offsets_either_side(answers, case):
    want = STEPS[case]
    assert answers[0][case] == (want, want)
    assert D.steps(*case) == want and D.steps(*case, wide=True) == want
    assert D.csp_steps(*case) == (want if case[1] > 0 else D.steps(case[0], 50.0, wide=True))      # csp: 50 A for a step that is not positive


@pytest.mark.parametrize("case", list(CHUNKS), ids=lambda c: f"T{c[0]}-rings{c[1]}-knob{c[2]}")
def test_offsets_per_pass(answers, case):
    T, nr, knob = case
    nt, tc = (T - 1) // 2, CHUNKS[case]
    assert tc >= 1
    assert answers[1][case] == (tc, -(-T // tc))
    assert D.chunk(nt, nr, knob) == tc and D.plan(nt, nr, knob) == (T, tc, -(-T // tc), -(-tc // 32))


def test_plans_of_the_shared_cases():
    """what tests/defocus_cases.py says its cases exercise follows from the rule"""
    for nt, pl in D.COUNTS.values():
        assert D.plan(nt, D.nrings_of(D.RHI64)) == pl
    for knob, pl in D.KNOBS.items():
        assert D.plan(20, D.nrings_of(D.RHI64), knob) == pl
    for n, rhi, nt, step, pl in D.LARGE.values():
        assert D.plan(nt, D.nrings_of(rhi)) == pl and pl[2] > 1
    # the second trip of the final reduction and the single-offset last chunk are both among them
    assert {pl[3] for _, pl in D.COUNTS.values()} == {1, 2} and D.LARGE["box240-nt15"][4][0] % D.LARGE["box240-nt15"][4][1] == 1
