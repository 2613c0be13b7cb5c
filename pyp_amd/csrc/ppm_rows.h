// ppm_rows.h — the row order of k_global's slice bank: one definition for the host (HsP, the row-twiddle table), k_bank, k_slice_norms
// and k_global.  Plain C++, no HIP types: compiled alone by tests/test_global_rows_cpu.py.
//
// k_global transforms the rows ky = -Bs .. Bs of a slice to a few shift rows j with twiddles cos / sin(j theta_t), theta_t = 2 pi t / Ns,
// from the even and odd parts E(t) = Q(+t) + Q(-t), O(t) = Q(+t) - Q(-t) of the row PAIR +-t.  The pair t' = Ns/2 - t has the same
// twiddles up to a sign that depends on the parity of j alone:
//     cos(j theta_t') = (-1)^j cos(j theta_t)          sin(j theta_t') = (-1)^(j+1) sin(j theta_t)
// so that the two pairs are FOLDED ahead of the multiply-adds (a radix-2 step of the ky transform):
//     U[j] += cos(j theta_t) (E(t) + (-1)^j E(t'))       V[j] += sin(j theta_t) (O(t) - (-1)^j O(t'))
// The bank stores a slice in STEPS of four rows, the rows k_global consumes together:
//     plain step   two pairs (+a, -a, +b, -b), each with its own twiddles;
//     quad         (+t, -t, +t', -t') with t' = Ns/2 - t, one set of twiddles.
// With t_lo = Ns/2 - Bs the quads are t = t_lo .. Ns/4 - 1 (partners Ns/4 + 1 .. Bs); t = 0 .. t_lo - 1 and t = Ns/4 have no partner
// inside the band and stay plain pairs.  Order: the plain pairs two per step (t ascending, Ns/4 last; the pair of t = 0 holds ky = 0 and
// an empty row; an odd count is padded with an empty pair), then the quads, t ascending.  k_global walks two steps per trip, so an odd
// step count is padded with one empty step: HsP = 4 steps is a multiple of 8.  Without quads (fold off, or Bs <= Ns/4) the order is the
// paired one: row 0 = ky 0, row 1 empty, rows 2t / 2t + 1 = ky +t / -t.
#pragma once

#ifndef PPM_HD
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif
#endif

namespace ppm {

struct RowPlan {
    int Ns, Bs;
    int t_lo;           // first folded t
    int n_pairs;        // plain pairs that hold rows (padding not counted)
    int n_quads;        // quads that hold rows
    int plain_steps;    // steps of two plain pairs, padding included
    int quad_steps;     // steps of one quad, padding included
    int HsP;            // stored rows of a slice: 4 (plain_steps + quad_steps)
};

// Ns: search grid (a multiple of 4, Ns >= 2 (Bs + 1)); Bs: search band; fold: false keeps the paired order whatever the band
PPM_HD inline RowPlan row_plan(int Ns, int Bs, bool fold) {
    RowPlan p;
    p.Ns = Ns; p.Bs = Bs;
    const bool quads = fold && Ns % 4 == 0 && Bs >= Ns / 4 + 1 && Bs < Ns / 2;
    p.t_lo = quads ? Ns / 2 - Bs : Ns / 4;
    p.n_quads = quads ? Ns / 4 - p.t_lo : 0;
    p.n_pairs = quads ? p.t_lo + 1 : Bs + 1;
    p.plain_steps = (p.n_pairs + 1) / 2;
    p.quad_steps = p.n_quads;
    if ((p.plain_steps + p.quad_steps) & 1) { if (quads) p.quad_steps++; else p.plain_steps++; }
    p.HsP = 4 * (p.plain_steps + p.quad_steps);
    return p;
}

PPM_HD inline int row_plan_steps(const RowPlan &p) { return p.plain_steps + p.quad_steps; }
PPM_HD inline bool row_step_is_quad(const RowPlan &p, int step) { return step >= p.plain_steps; }

// The t whose twiddles pair slot `slot` (= stored row / 2) uses; a quad reads those of its first slot.  Padding: 0.
PPM_HD inline int row_slot_t(const RowPlan &p, int slot) {
    if (slot < 2 * p.plain_steps) {
        if (slot >= p.n_pairs) return 0;
        return (p.n_quads > 0 && slot == p.n_pairs - 1) ? p.Ns / 4 : slot;
    }
    const int q = (slot - 2 * p.plain_steps) >> 1;
    if (q >= p.n_quads) return 0;
    const int t = p.t_lo + q;
    return (slot & 1) ? p.Ns / 2 - t : t;
}

// ky of stored row r (0 <= r < HsP); false: the row is empty (zeros in the bank and in k_global's W table)
PPM_HD inline bool row_ky(const RowPlan &p, int r, int &ky) {
    const int slot = r >> 1;
    if (slot < 2 * p.plain_steps) { if (slot >= p.n_pairs) return false; }
    else if (((slot - 2 * p.plain_steps) >> 1) >= p.n_quads) return false;
    const int t = row_slot_t(p, slot);
    if (t == 0 && (r & 1)) return false;
    ky = (r & 1) ? -t : t;
    return true;
}

}  // namespace ppm
