"""The k-th value by two histogram passes of 16 bits each (ppm_postprocess: the volume-fraction threshold of the automatic mask, from the
top; ppm_local_resolution: tau, from the bottom) leaves its integer decisions to pyp_amd/csrc/ppm_rank.h (no HIP in it): the walk over
one histogram, the count that is a fraction of the total, the rank of a p-value, the float behind a key.  A few lines of C++ with their own
main are compiled against the header with the host compiler under AddressSanitizer and UBSan and run over a table of cases: the program
makes the keys (the two key rules of the kernels, restated here) and the two histograms on the CPU, walks them with the header and prints
the value found; numpy.sort says what it should be."""
import math
import os
import subprocess

import numpy as np
import pytest

from pyp_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ppm_rank.h"

static unsigned bits_of(float v) { unsigned u; std::memcpy(&u, &v, sizeof(u)); return u; }
// non-negative values, negatives and -0 count as 0: the key is the float's own bits (lr_key)
static unsigned key_nonneg(float v) { const unsigned u = bits_of(v); return (u & 0x80000000u) ? 0u : u; }
// signed values: negatives with every bit flipped, the others with the sign bit set (post_key)
static unsigned key_signed(float v) { const unsigned u = bits_of(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// the two passes over `v`; false: a histogram holds fewer values than wanted
static bool kth(const std::vector<float> &v, bool from_top, long long want, unsigned *key) {
    const int bins0 = from_top ? 65536 : 32768;
    unsigned prefix = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int bins = pass == 0 ? bins0 : 65536;
        std::vector<unsigned> hist((size_t)bins, 0u);             // exactly `bins` long: a walk past the end is a sanitizer error
        for (float x : v) {
            const unsigned k = from_top ? key_signed(x) : key_nonneg(x);
            if (pass == 0) hist[k >> 16]++;
            else if ((k >> 16) == prefix) hist[k & 0xffffu]++;
        }
        const ppm::RankBin r = ppm::rank_walk(hist.data(), bins, want, from_top);
        if (r.bin < 0) return false;
        want = r.want;
        if (pass == 0) prefix = (unsigned)r.bin; else *key = (prefix << 16) | (unsigned)r.bin;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char what[32], arg[512];
    long long k;
    while (fscanf(f, "%31s %511s %lld", what, arg, &k) == 3) {
        if (!strcmp(what, "fraction")) { printf("%lld\n", ppm::rank_of_fraction(strtod(arg, nullptr), k)); continue; }
        if (!strcmp(what, "locres")) { printf("%ld\n", ppm::locres_rank(strtod(arg, nullptr), (long)k)); continue; }
        FILE *d = fopen(arg, "rb");
        if (!d) return 3;
        std::vector<float> v;
        float x;
        while (fread(&x, sizeof(x), 1, d) == 1) v.push_back(x);
        fclose(d);
        const bool from_top = !strcmp(what, "largest");
        unsigned key = 0;
        if (!kth(v, from_top, k, &key)) { printf("notfound\n"); continue; }
        float out;
        if (from_top) out = ppm::rank_signed_key_value(key); else std::memcpy(&out, &key, sizeof(out));
        printf("%08x\n", bits_of(out));
    }
    fclose(f);
    return 0;
}
'''


def _sets():
    rng = np.random.default_rng(20)
    f32 = np.float32
    nonneg = np.exp(rng.normal(0.0, 3.0, 5000)).astype(f32)
    nonneg[::7] = -nonneg[::7]                       # negatives count as 0
    nonneg[3::50] = f32(-0.0)
    nonneg[4::50] = f32(0.0)
    signed = rng.normal(0.0, 2.0, 5000).astype(f32)
    signed[3::50] = f32(-0.0)
    signed[4::50] = f32(0.0)
    low = (np.uint32(0x3F800000) + rng.permutation(3000).astype(np.uint32) * np.uint32(17)).view(f32)     # one upper half, 3000 lower halves
    ties = np.concatenate([np.full(100, 1.5, f32), f32([0.25, 1.4999999, 1.5000001, 7.0])])
    return {"mixed": nonneg, "signed": signed, "one upper half": low, "one upper half, negative": -low, "ties": ties,
            "one bin": np.full(100, 1.5, f32), "one bin, negative": np.full(64, -3.25, f32), "single": f32([2.5]), "single, negative": f32([-2.5]),
            "zeros": f32([-0.0, 0.0]), "all below zero": f32([-1.0, -2.0, -0.0])}


# (mode, set, k): k = 1, the total, in between; a total + 1 is not found
KTH = [("smallest", s, k) for s, ks in (("mixed", (1, 2, 715, 716, 2500, 4999, 5000)), ("one upper half", (1, 1234, 3000)), ("ties", (1, 2, 3, 52, 102, 103, 104)),
                                       ("one bin", (1, 50, 100)), ("single", (1,)), ("all below zero", (1, 3)), ("zeros", (1, 2))) for k in ks]
KTH += [("largest", s, k) for s, ks in (("signed", (1, 2, 2500, 4999, 5000)), ("one upper half", (1, 1234, 3000)), ("one upper half, negative", (1, 1234, 3000)),
                                       ("ties", (1, 2, 3, 52, 102, 103, 104)), ("one bin", (1, 100)), ("one bin, negative", (1, 33, 64)), ("single", (1,)),
                                       ("single, negative", (1,)), ("zeros", (1, 2)), ("mixed", (1, 5000))) for k in ks]
MISSING = [("smallest", "mixed", 5001), ("smallest", "single", 2), ("largest", "signed", 5001), ("largest", "single, negative", 2), ("largest", "one bin", 101)]
# (f, total) -> count: f -> 0+, f = 1, f total an exact integer, and in between
FRACTION = [(5e-324, 1000, 1), (1e-300, 268435456, 1), (1.0, 1000, 1000), (1.0, 1, 1), (0.25, 1000, 250), (0.5, 8, 4), (0.1, 10, 1), (0.5, 7, 4),
            (0.3, 65267, 19581), (1.0, 134217728, 134217728), (0.999999999, 134217728, 134217728), (1e-9, 1, 1)]
# (p, n): p -> 0+, p -> 1-, and the cases of test_locres_cpu.test_rank_rule
LOCRES = [(1e-12, 1000, 1000), (1e-300, 7, 7), (1.0 - 1e-12, 1000, 1), (0.9999999, 5, 1), (0.05, 1, 1), (0.999, 1, 1), (1e-9, 1, 1), (0.05, 100, 95),
          (0.05, 101, 96), (0.5, 3, 2)] + [(p, n, None) for p in (0.05, 0.3, 0.01) for n in (1, 2, 57, 65267, 134217728)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rank")
    sets = _sets()
    files = {}
    for i, (name, v) in enumerate(sets.items()):
        files[name] = str(tmp / f"set{i}.f32")
        v.astype("<f4").tofile(files[name])
    lines = [f"{mode} {files[s]} {k}" for mode, s, k in KTH + MISSING]
    lines += [f"fraction {f!r} {total}" for f, total, _ in FRACTION] + [f"locres {p!r} {n}" for p, n, _ in LOCRES]
    (tmp / "cases.txt").write_text("\n".join(lines) + "\n")
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().split()
    assert len(out) == len(lines)
    keys = [("kth",) + c for c in KTH + MISSING] + [("fraction",) + c[:2] for c in FRACTION] + [("locres",) + c[:2] for c in LOCRES]
    return sets, dict(zip(keys, out))


def _value(text):
    return np.array([int(text, 16)], dtype=np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("mode,name,k", KTH, ids=[f"{m} {k} of {s}" for m, s, k in KTH])
def test_kth_value_is_what_a_sort_gives(answers, mode, name, k):
    sets, out = answers
    v = sets[name]
    got = _value(out[("kth", mode, name, k)])
    if mode == "smallest":
        want = np.sort(np.where(np.signbit(v), np.float32(0), v))[k - 1]
        assert got == want and not np.signbit(got)
    else:
        want = np.sort(v)[::-1][k - 1]
        assert got == want
        if want == 0:           # +0 ranks above -0
            zeros_above = int((v > 0).sum()) + int(((v == 0) & ~np.signbit(v)).sum())
            assert bool(np.signbit(got)) == (k > zeros_above)


@pytest.mark.parametrize("mode,name,k", MISSING, ids=[f"{m} {k} of {s}" for m, s, k in MISSING])
def test_a_request_above_the_total_is_not_found(answers, mode, name, k):
    sets, out = answers
    assert k == len(sets[name]) + 1 and out[("kth", mode, name, k)] == "notfound"


@pytest.mark.parametrize("f,total,want", FRACTION)
def test_fraction_rule(answers, f, total, want):
    assert int(answers[1][("fraction", f, total)]) == want == max(1, min(math.ceil(f * float(total)), total))


@pytest.mark.parametrize("p,n,want", LOCRES)
def test_locres_rank_agrees_with_the_rule_in_python(answers, p, n, want):
    got = int(answers[1][("locres", p, n)])
    assert got == abi.locres_rank(p, n) and 1 <= got <= n
    if want is not None:
        assert got == want
