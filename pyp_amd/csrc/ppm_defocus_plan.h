// ppm_defocus_plan.h — the two host rules of the defocus refinement (k_defocus, ppm_kernels2.h): how many offsets lie either side of a
// row's defocus, and how many of them one pass over the samples scores.  Used by ppm_refine_batch (host_refine.h) and csp mode 4
// (host_csp.h).  Plain C++, no HIP types: compiled alone by tests/test_defocus_plan_cpu.py.
#pragma once

#include <cmath>

#ifndef PPM_HD
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif
#endif

namespace ppm {

// the per-wave ring tables of one pass (16 bytes per offset and ring: 4 waves x float) stay below this many bytes of dynamic LDS
constexpr long kDefocusTableBytes = 60000;

// Offsets tried on either side (2 nt + 1 in all) for a search of +-range in steps of step, at most `cap` (PPM_MAX_DEFOCUS_STEPS); 0: no
// search (a step that is not positive, a range below one step).  The 1e-6 keeps quotients such as 0.3 / 0.1 at 3.  The quotient is
// formed in the callers' own types (float / float in the refinement, float / double in csp), as the oracle forms it.
template <class R, class S>
PPM_HD inline int defocus_steps(R range, S step, int cap) {
    if (!(step > 0) || !(range >= step)) return 0;
    const int nt = (int)std::floor(range / step + 1e-6);
    return nt < cap ? nt : cap;
}

// Offsets one pass scores (k_defocus's TC): all 2 nt + 1 if their ring tables fit kDefocusTableBytes, never fewer than one.  `knob`
// (PPM_DEFOCUS_CHUNK, tests: every chunk shape at a small box) lowers it when positive and never raises it.
PPM_HD inline int defocus_chunk(int nt, int nrings, long knob) {
    const long T = 2L * nt + 1, fit = nrings > 0 ? kDefocusTableBytes / (16L * nrings) : T;
    long tc = T < fit ? T : fit;
    if (knob > 0 && knob < tc) tc = knob;
    return tc < 1 ? 1 : (int)tc;
}

// passes over the samples for 2 nt + 1 offsets in chunks of tc
PPM_HD inline int defocus_chunks(int nt, int tc) { return tc > 0 ? (2 * nt + tc) / tc : 0; }

}  // namespace ppm
