"""The host rules of the sub-tomogram transforms and of ppm_sva_align's chunks live in pyp_amd/csrc/ppm_sva_plan.h (no HIP in it): the
lines a block of the two-step transforms takes, the partial sums their x pass writes, the extent of the pruned transform from (N, R),
and the chunk rule (n_vol, S, n3, residence, PPM_SVA_CHUNK, global, Kc) -> (CH, NB, states per chunk, staging buffers).  A few lines of
C++ with their own main are compiled against the header with the host compiler under AddressSanitizer and UBSan and run over a table;
the expected values are the formulas written out below, with spot literals worked out by hand from the rules as host_sva.h had them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_sva_plan.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'x') {              // N R nb -> lines per block, partial sums of the x pass, KX, KY
            int N, R, nb;
            if (fscanf(f, "%d %d %d", &N, &R, &nb) != 3) return 3;
            printf("%d %zu %d %d\n", ppm::sva_lines_per_block(N), ppm::sva_xpass_partials(N, nb), ppm::sva_kx(N, R), ppm::sva_ky(N, R));
        } else {                        // n_vol S n3 resident knob global Kc -> CH, NB, states per chunk, staging buffers
            int n_vol, resident, knob, global, Kc; unsigned long long S, n3;
            if (fscanf(f, "%d %llu %llu %d %d %d %d", &n_vol, &S, &n3, &resident, &knob, &global, &Kc) != 7) return 3;
            const ppm::SvaChunks c = ppm::sva_chunks(n_vol, (size_t)S, (size_t)n3, resident != 0, knob, global != 0, Kc);
            printf("%d %d %zu %d\n", c.CH, c.NB, c.states, c.staging);
        }
    }
    fclose(f);
    return 0;
}
'''

BOXES = (32, 40, 48, 192, 256, 272, 512)
GB = 1 << 30


def lines_per_block(n):
    return 16 if n <= 256 else 8


def xform(n, r, nb):
    return (lines_per_block(n), 2 * nb * (n * n // lines_per_block(n)), min(n // 2 + 1, r + 1), min(n, 2 * r + 1))


def chunks(n_vol, s, n3, resident, knob, glob, kc):
    ch = 4 * GB // (s * 8)
    if not resident:
        ch = min(ch, knob if knob > 0 else 7 * GB // (n3 * 4))
    ch = min(n_vol, max(1, ch))
    return (ch, min(ch, 32), ch * (kc if glob else 1), 0 if resident else (2 if n_vol > ch else 1))


# (N, R, nb): every box at its full transform (R = N / 2, the average's), at a pruned band, and at one and 32 sub-volumes per launch
XFORMS = [(n, n // 2, nb) for n in BOXES for nb in (1, 32)] + [(n, n // 4, 3) for n in BOXES] + [(192, 48, 32), (32, 15, 3), (512, 255, 32)]
XFORM_LITERALS = {
    (32, 16, 1): (16, 128, 17, 32), (256, 128, 32): (16, 262144, 129, 256), (272, 136, 1): (8, 18496, 137, 272), (512, 256, 32): (8, 2097152, 257, 512),
    (192, 48, 32): (16, 147456, 49, 97), (40, 20, 1): (16, 200, 21, 40), (32, 15, 3): (16, 384, 16, 31), (512, 255, 32): (8, 2097152, 256, 511),
}
S32, S192 = 2109, 452000                 # samples of a band at box 32 and at 192^3 (host_ctx.h: ~452 k)
# (n_vol, S, n3, resident, knob, global, Kc)
CHUNKS = [(nv, S32, 32 ** 3, res, knob, glob, 25) for nv in (1, 33) for res in (0, 1) for knob in (0, 3) for glob in (0, 1)] + [
    (1000, S192, 192 ** 3, 0, 0, 0, 25), (1000, S192, 192 ** 3, 1, 0, 0, 25), (2000, S192, 192 ** 3, 1, 0, 1, 25), (2000, S192, 192 ** 3, 0, 0, 1, 25),
    (33, 100_000_000, 32 ** 3, 1, 0, 0, 25), (33, 100_000_000, 32 ** 3, 0, 0, 1, 25), (33, 100_000_000, 32 ** 3, 0, 3, 0, 25),
    (33, 1 << 40, 32 ** 3, 1, 0, 1, 25), (40, S32, 32 ** 3, 0, 0, 0, 25), (64, S32, 512 ** 3, 0, 0, 0, 25), (3, S32, 32 ** 3, 0, 3, 0, 25), (4, S32, 32 ** 3, 0, 3, 0, 25),
]
CHUNK_LITERALS = {
    (1, S32, 32 ** 3, 0, 0, 0, 25): (1, 1, 1, 1), (1, S32, 32 ** 3, 1, 0, 1, 25): (1, 1, 25, 0),
    (33, S32, 32 ** 3, 1, 0, 0, 25): (33, 32, 33, 0), (33, S32, 32 ** 3, 1, 3, 0, 25): (33, 32, 33, 0),      # the knob is for host volumes only
    (33, S32, 32 ** 3, 0, 3, 1, 25): (3, 3, 75, 2), (33, S32, 32 ** 3, 1, 0, 1, 25): (33, 32, 825, 0),
    (1000, S192, 192 ** 3, 0, 0, 0, 25): (265, 32, 265, 2),      # 7 GB / (192^3 x 4 bytes) = 265.48
    (1000, S192, 192 ** 3, 1, 0, 0, 25): (1000, 32, 1000, 0), (2000, S192, 192 ** 3, 1, 0, 1, 25): (1187, 32, 29675, 0),      # 4 GB / (452000 x 8) = 1187.8
    (33, 100_000_000, 32 ** 3, 1, 0, 0, 25): (5, 5, 5, 0), (33, 100_000_000, 32 ** 3, 0, 3, 0, 25): (3, 3, 3, 2),
    (33, 1 << 40, 32 ** 3, 1, 0, 1, 25): (1, 1, 25, 0),          # never fewer than one sub-volume a chunk
    (64, S32, 512 ** 3, 0, 0, 0, 25): (14, 14, 14, 2),           # 7 GB / (512^3 x 4 bytes) = 14
    (3, S32, 32 ** 3, 0, 3, 0, 25): (3, 3, 3, 1), (4, S32, 32 ** 3, 0, 3, 0, 25): (3, 3, 3, 2),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sva_plan")
    lines = ["x %d %d %d" % c for c in XFORMS] + ["c %d %d %d %d %d %d %d" % c for c in CHUNKS]
    (tmp / "cases.txt").write_text("\n".join(lines) + "\n")
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().splitlines()
    assert len(out) == len(lines)
    got = [tuple(int(x) for x in line.split()) for line in out]
    return dict(zip(XFORMS, got[:len(XFORMS)])), dict(zip(CHUNKS, got[len(XFORMS):]))


@pytest.mark.parametrize("case", XFORMS, ids=lambda c: "box%d-R%d-nb%d" % c)
def test_transform_extent_and_partial_sums(answers, case):
    n, r, nb = case
    assert answers[0][case] == xform(*case)
    if case in XFORM_LITERALS:
        assert answers[0][case] == XFORM_LITERALS[case]
    L, partials, kx, ky = answers[0][case]
    if n % 16 == 0:                     # the two-step boxes: k_sva_x16 runs nb N^2 / L blocks of whole lines and writes two doubles each
        assert n * n % L == 0 and partials == 2 * nb * n * n // L


def test_the_literals_are_among_the_cases():
    assert set(XFORM_LITERALS) <= set(XFORMS) and set(CHUNK_LITERALS) <= set(CHUNKS)
    assert {lines_per_block(n) for n in BOXES if n <= 256} == {16} and {lines_per_block(n) for n in BOXES if n > 256} == {8}


@pytest.mark.parametrize("case", CHUNKS, ids=lambda c: "n%d-S%d-n3_%d-%s-knob%d-%s" % (c[0], c[1], c[2], "resident" if c[3] else "host", c[4], "global" if c[5] else "local"))
def test_chunk_rule(answers, case):
    n_vol = case[0]
    assert answers[1][case] == chunks(*case)
    if case in CHUNK_LITERALS:
        assert answers[1][case] == CHUNK_LITERALS[case]
    ch, nb, states, staging = answers[1][case]
    assert 1 <= nb <= min(ch, 32) and ch <= n_vol and states == ch * (25 if case[5] else 1)
    assert staging == (0 if case[3] else (2 if n_vol > ch else 1))
