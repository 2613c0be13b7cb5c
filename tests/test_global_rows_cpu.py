"""The row order of k_global's slice bank is planned by one function, row_plan of pyp_amd/csrc/ppm_rows.h (no HIP in it), which the
host, k_bank, k_slice_norms and k_global all go through.  A few lines of C++ with their own main are compiled against the header with
the host compiler under AddressSanitizer and UBSan and run over a table of (Ns, Bs); every plan is checked here: every ky of the band
stored exactly once, quads made of a pair t and its partner Ns/2 - t, t = 0 and t = Ns/4 never folded, HsP a multiple of 8, the step
count.  A float64 numpy check folds random rows by the plan, as the kernel's quad step does, and compares with the direct sum over ky."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "ppm_rows.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int Ns, Bs, fold;
    while (fscanf(f, "%d %d %d", &Ns, &Bs, &fold) == 3) {
        const ppm::RowPlan p = ppm::row_plan(Ns, Bs, fold != 0);
        printf("PLAN %d %d %d %d %d\n", p.HsP, p.plain_steps, p.quad_steps, p.n_pairs, p.n_quads);
        for (int r = 0; r < p.HsP; r++) {
            int ky = 0;
            const bool ok = ppm::row_ky(p, r, ky);
            printf("ROW %d %d %d %d %d\n", r, ok ? 1 : 0, ky, ppm::row_step_is_quad(p, r / 4) ? 1 : 0, ppm::row_slot_t(p, r / 2));
        }
    }
    fclose(f);
    return 0;
}
'''

# (Ns, Bs): the headline's plan, half folded, one quad, the last band without a quad, and the smaller search grids
TABLE = [(128, 63), (128, 47), (128, 33), (128, 32), (64, 31), (64, 20), (32, 15), (16, 7), (128, 34), (128, 62), (64, 17), (64, 16), (16, 4), (16, 5)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(Ns, Bs, fold): (HsP, plain_steps, quad_steps, n_pairs, n_quads, rows)}, rows = [(stored, ky, in a quad's step, t of the slot)]"""
    tmp = tmp_path_factory.mktemp("rows")
    cases = [(ns, bs, fold) for ns, bs in TABLE for fold in (1, 0)]
    (tmp / "cases.txt").write_text("".join("%d %d %d\n" % c for c in cases))
    (tmp / "t.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(tmp / "t"), str(tmp / "t.cpp")])
    out = subprocess.check_output([str(tmp / "t"), str(tmp / "cases.txt")]).decode().splitlines()
    res, it = {}, iter(out)
    for c in cases:
        head = next(it).split()
        assert head[0] == "PLAN"
        hsp, ps, qs, npairs, nquads = (int(x) for x in head[1:])
        rows = []
        for r in range(hsp):
            v = next(it).split()
            assert v[0] == "ROW" and int(v[1]) == r
            rows.append((int(v[2]) == 1, int(v[3]), int(v[4]) == 1, int(v[5])))
        res[c] = (hsp, ps, qs, npairs, nquads, rows)
    assert next(it, None) is None
    return res


def expected_counts(Ns, Bs, fold):
    """pairs, quads and steps from the rule: quads t = Ns/2 - Bs .. Ns/4 - 1 when the band goes beyond Ns/4, plain pairs two per
    step, one quad per step, an odd count padded with one empty step"""
    quads = max(0, Bs - Ns // 4) if fold else 0
    pairs = (Ns // 2 - Bs) + 1 if quads else Bs + 1
    steps = (pairs + 1) // 2 + quads
    return pairs, quads, steps + (steps & 1)


@pytest.mark.parametrize("Ns,Bs", TABLE)
def test_every_ky_once_quads_hold_a_pair_and_its_partner(plans, Ns, Bs):
    hsp, ps, qs, npairs, nquads, rows = plans[(Ns, Bs, 1)]
    pairs, quads, steps = expected_counts(Ns, Bs, True)
    assert (npairs, nquads) == (pairs, quads)
    assert ps + qs == steps and hsp == 4 * steps and hsp % 8 == 0
    assert quads == (0 if Bs < Ns // 4 + 1 else Bs - Ns // 4)
    kys = [ky for ok, ky, _, _ in rows if ok]
    assert sorted(kys) == list(range(-Bs, Bs + 1))                        # every ky of the band, once
    for s in range(hsp // 4):
        step = rows[4 * s:4 * s + 4]
        assert all(q == (s >= ps) for _, _, q, _ in step)                # plain steps first, then the quads
        if s < ps:
            for a in (0, 2):                                              # two pairs (+t, -t), or ky = 0 and an empty row, or padding
                (oka, kya, _, ta), (okb, kyb, _, _) = step[a], step[a + 1]
                if not oka:
                    assert not okb and ta == 0
                    continue
                assert kya == ta >= 0 and (kyb == -ta and okb if ta else not okb)
                if quads:
                    assert ta < Ns // 2 - Bs or ta == Ns // 4            # only what has no partner inside the band stays plain
        else:
            if not step[0][0]:
                assert not any(ok for ok, _, _, _ in step)                # the empty step that makes the count even
                continue
            assert all(ok for ok, _, _, _ in step)
            t = step[0][1]
            assert [ky for _, ky, _, _ in step] == [t, -t, Ns // 2 - t, -(Ns // 2 - t)]
            assert 0 < t < Ns // 4 < Ns // 2 - t <= Bs                    # both halves inside the band; never t = 0 or t = Ns/4
            assert step[0][3] == t                                        # the step's twiddles are those of t
    if quads == 0:                                                        # today's order: row 0 = ky 0, row 1 empty, rows 2t / 2t+1 = +t / -t
        assert rows == plans[(Ns, Bs, 0)][5]


@pytest.mark.parametrize("Ns,Bs", TABLE)
def test_without_the_fold_the_order_is_the_paired_one(plans, Ns, Bs):
    hsp, ps, qs, npairs, nquads, rows = plans[(Ns, Bs, 0)]
    assert qs == 0 and nquads == 0 and hsp == -(-(2 * (Bs + 1)) // 8) * 8
    for r, (ok, ky, quad, t) in enumerate(rows):
        tt = r >> 1
        assert not quad
        assert ok == (r != 1 and tt <= Bs)
        if ok:
            assert ky == (-tt if r & 1 else tt) and t == tt


@pytest.mark.parametrize("Ns,Bs", TABLE)
def test_folded_sums_equal_the_direct_transform(plans, Ns, Bs):
    """G[j] = sum_ky Q(ky) e^{2 pi i ky j / Ns}, j = -6 .. 6, accumulated step by step as k_global does — U + iV from the even and odd
    parts of the pairs, the quads folded first and multiplied by the twiddles of t alone — against the direct sum, in float64."""
    hsp, ps, qs, npairs, nquads, rows = plans[(Ns, Bs, 1)]
    rng = np.random.default_rng(Ns * 1000 + Bs)
    Q = {ky: complex(rng.standard_normal(), rng.standard_normal()) for ky in range(-Bs, Bs + 1)}
    stored = [Q[ky] if ok else 0j for ok, ky, _, _ in rows]
    R = 6
    s0, U, V = 0j, np.zeros(R + 1, complex), np.zeros(R + 1, complex)
    j = np.arange(1, R + 1)
    for s in range(hsp // 4):
        q = stored[4 * s:4 * s + 4]
        if s < ps:
            for a in (0, 2):
                th = 2 * np.pi * rows[4 * s + a][3] / Ns
                E, O = q[a] + q[a + 1], q[a] - q[a + 1]
                s0 += E
                U[1:] += E * np.cos(j * th); V[1:] += O * np.sin(j * th)
        else:
            th = 2 * np.pi * rows[4 * s][3] / Ns
            E, O, E2, O2 = q[0] + q[1], q[0] - q[1], q[2] + q[3], q[2] - q[3]
            even, odd = (E + E2, O - O2), (E - E2, O + O2)                # what the even and the odd shift rows take
            s0 += even[0]
            for jj in j:
                e, o = even if jj % 2 == 0 else odd
                U[jj] += e * np.cos(jj * th); V[jj] += o * np.sin(jj * th)
    ky = np.arange(-Bs, Bs + 1)
    q = np.array([Q[k] for k in ky])
    for jj in range(-R, R + 1):
        want = (q * np.exp(2j * np.pi * ky * jj / Ns)).sum()
        got = s0 if jj == 0 else U[abs(jj)] + (1j if jj > 0 else -1j) * V[abs(jj)]
        assert abs(got - want) < 1e-12, (Ns, Bs, jj, abs(got - want))
