"""The launch plan of k_prep is defined once, prep_plan / prep_lds of pyp_amd/csrc/ppm_geom.h: launch_prep launches from it and the
kernel takes its LDS pointers from the same function.  A few lines of C++ are compiled against the header; the Python restatement
that the box sweep chooses its ragged bands with (f64_ref.prep_plan) is held to it for every box and band, and the carve-up of the
LDS is checked region by region: disjoint, aligned for its element type, inside the bytes the launch asks for."""
import os
import subprocess

import f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_geom.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int N, B;
    while (fscanf(f, "%d %d", &N, &B) == 2) {
        const ppm::PrepPlan p = ppm::prep_plan(N, B, B + 1);
        const ppm::PrepLds &l = p.lds;
        const ppm::LdsRegion r[11] = { l.T, l.Wk, l.ringq, l.ringc, l.ringpw, l.red, l.stat, l.fmask, l.tw, l.perm, l.iperm };
        printf("%d %d %d %d %d %d %d %d %u %d", N, B, p.scratch_free ? 1 : 0, p.threads, p.L, p.nc, p.nchunks, p.TS * 1000 + p.WS, l.total, p.err ? 1 : 0);
        for (int i = 0; i < 11; i++) printf(" %u %u %u", r[i].off, r[i].bytes, r[i].elem);
        printf("\n");
    }
    return 0;
}
'''
REGIONS = ("T", "Wk", "ringq", "ringc", "ringpw", "red", "stat", "fmask", "tw", "perm", "iperm")
# what every region has to hold: elements x element size (PW = waves of the block)
NEED = {"T": lambda N, B, PW, L, nc, TS, WS: nc * TS * 8, "Wk": lambda N, B, PW, L, nc, TS, WS: L * WS * 8,
        "ringq": lambda N, B, PW, *_: (B + 2) * 8, "ringc": lambda N, B, PW, *_: (B + 2) * 4, "ringpw": lambda N, B, PW, *_: (B + 2) * 4,
        "red": lambda N, B, PW, *_: 5 * PW * 8, "stat": lambda N, B, PW, *_: (3 + PW) * 4, "fmask": lambda N, B, PW, *_: 6 * 4,
        "tw": lambda N, B, PW, *_: N * 8, "perm": lambda N, B, PW, *_: N * 2 if N != 256 else 0,
        "iperm": lambda N, B, PW, *_: N * 2 if N != 256 else 0}
# f64_ref.ragged_band of every supported box, as the sweep has used it since it was written
RAGGED = {32: 8, 36: 8, 40: 8, 42: 8, 48: 8, 50: 8, 54: 8, 56: 8, 60: 8, 64: 8, 70: 8, 72: 8, 80: 8, 84: 8, 90: 8, 96: 8, 98: 8, 100: 8,
          108: 8, 112: 8, 120: 8, 126: 8, 128: 8, 140: 8, 144: 8, 150: 8, 160: 8, 162: 18, 168: 16, 180: 16, 192: 91, 196: 91, 200: 99,
          210: 104, 216: 99, 224: 110, 240: 110, 250: 121, 252: 120, 256: 126, 270: 132, 280: 136, 288: 135, 294: 140, 300: 144,
          320: 152, 324: 161, 336: 162, 350: 168, 360: 174, 378: 182, 384: 186, 392: 192, 400: 195, 420: 204, 432: 215, 448: 220,
          450: 220, 480: 235, 486: 240, 490: 240, 500: 245, 504: 248, 512: 255}


def test_prep_plan_matches_its_python_restatement_and_the_lds_regions_fit(tmp_path):
    boxes = R.supported_boxes()
    cases = [(N, B) for N in boxes for B in range(8, N // 2)]
    (tmp_path / "cases.txt").write_text("".join("%d %d\n" % c for c in cases))
    (tmp_path / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp_path / "t"),
                           str(tmp_path / "t.cpp")])
    out = subprocess.check_output([str(tmp_path / "t"), str(tmp_path / "cases.txt")]).decode().splitlines()
    assert len(out) == len(cases)
    for (N, B), line in zip(cases, out):
        v = [int(x) for x in line.split()]
        n, b, scratch_free, threads, L, nc, nchunks, strides, total, err = v[:10]
        TS, WS = divmod(strides, 1000)
        reg = {name: tuple(v[10 + 3 * i:13 + 3 * i]) for i, name in enumerate(REGIONS)}
        W = B + 1
        assert (n, b, err) == (N, B, 0), line
        if N == 256:                                           # the scratch-free plan: fixed figures
            assert (scratch_free, threads, L, nc, nchunks, TS, WS) == (1, 512, 64, 64, -(-min(W, 128) // 64), 273, 272), line
            assert total <= 160 * 1024, line
            assert reg["Wk"][0] == reg["T"][0] == 0, line      # the row buffer shares T's storage; both precede every other region
            spans = [max(reg["T"], reg["Wk"], key=lambda r: r[1])] + [reg[k] for k in REGIONS[2:]]
        else:
            assert (scratch_free, threads, TS, WS) == (0, 256, N + 1, N), line
            assert (L, nc, nchunks, W - (nchunks - 1) * nc, total) == R.prep_plan(N, B), (line, R.prep_plan(N, B))
            assert (N // 2) % L == 0 and L * N <= 8 * threads and nc * N <= 12 * threads, line     # what the kernel's prefetch registers hold
            assert total <= 40 * 1024, line
            spans = [reg[k] for k in REGIONS]
        assert 1 <= W - (nchunks - 1) * nc <= nc, line
        for name in REGIONS:
            off, nbytes, elem = reg[name]
            assert off % elem == 0, (line, name)
            assert nbytes >= NEED[name](N, B, threads // 64, L, nc, TS, WS), (line, name)
            assert off + nbytes <= total, (line, name)
        spans = sorted(s for s in spans if s[1])
        for (o0, n0, _), (o1, _, _) in zip(spans, spans[1:]):
            assert o0 + n0 <= o1, (line, spans)
    # the sweep selects the bands and boxes it always did
    got = {N: R.ragged_band(N) for N in boxes}
    print("ragged_band:", got)
    print("SEARCH_ABOVE_256:", R.SEARCH_ABOVE_256, [R.prep_plan(N, got[N])[:4] for N in R.SEARCH_ABOVE_256])
    assert got == RAGGED
    assert R.SEARCH_ABOVE_256 == (270, 294, 384, 486, 490, 500, 512)
