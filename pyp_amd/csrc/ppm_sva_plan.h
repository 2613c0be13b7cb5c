// ppm_sva_plan.h — the host rules of the sub-tomogram transforms and of ppm_sva_align's chunks (host_sva.h): lines per block of the
// two-step transforms, the partial sums their x pass writes, the pruned transform's extent, and how a call's sub-volumes are cut into
// chunks.  Plain C++, no HIP types: compiled alone by tests/test_sva_plan_cpu.py.
#pragma once

#include <cstddef>

namespace ppm {

// lines of length N one block of k_sva_x16 / k_sva_yz16 transforms (its LDS: L x (N + 1) float2)
inline int sva_lines_per_block(int N) { return N <= 256 ? 16 : 8; }

// Doubles the x pass of the two-step transform writes for `nb` sub-volumes: k_sva_x16 runs nb N^2 / L blocks and block b writes
// stats[2 b] and stats[2 b + 1] (sum and sum of squares of its lines).  Two-step boxes are multiples of 16, so L divides N^2.
inline size_t sva_xpass_partials(int N, int nb) { return (size_t)2 * nb * ((size_t)N * N / sva_lines_per_block(N)); }

// Extent of the pruned transform for a band of radius R: kx < KX and KY lines along y (and z), |ky| <= R.  R = N / 2: the full transform.
inline int sva_kx(int N, int R) { return N / 2 + 1 < R + 1 ? N / 2 + 1 : R + 1; }
inline int sva_ky(int N, int R) { return N < 2 * R + 1 ? N : 2 * R + 1; }

constexpr size_t kSvaBandBytes = (size_t)4 << 30;       // band transforms of a chunk (S float2 per sub-volume)
constexpr size_t kSvaHostChunkBytes = (size_t)7 << 30;  // one staging buffer of host volumes (2 x 7 GB at 192^3: small change on a 288 GB device)
constexpr int kSvaPerLaunch = 32;                       // sub-volumes per transform launch (work array: NB x N x N x KX complex)

// The chunks of a call.  The search runs one block per sub-volume, so a chunk should fill the chip; resident volumes are limited by the
// band transforms alone, host volumes also by the staging buffer, or by `knob` (PPM_SVA_CHUNK, tests: several chunks of a small call)
// when it is positive.  The global search refines Kc candidates per sub-volume, each a state of its own.  Host volumes in more than one
// chunk take two staging buffers (the next chunk travels while this one is searched), in one chunk one, resident volumes none.
struct SvaChunks { int CH = 0, NB = 0; size_t states = 0; int staging = 0; };
inline SvaChunks sva_chunks(int n_vol, size_t S, size_t n3, bool on_device, int knob, bool global, int Kc) {
    SvaChunks c;
    size_t ch = kSvaBandBytes / (S * 8);
    if (!on_device) {
        const size_t hc = knob > 0 ? (size_t)knob : kSvaHostChunkBytes / (n3 * 4);
        if (hc < ch) ch = hc;
    }
    if (ch < 1) ch = 1;
    c.CH = (size_t)n_vol < ch ? n_vol : (int)ch;
    c.NB = c.CH < kSvaPerLaunch ? c.CH : kSvaPerLaunch;
    c.states = (size_t)c.CH * (global ? Kc : 1);
    c.staging = on_device ? 0 : (n_vol > c.CH ? 2 : 1);
    return c;
}

}  // namespace ppm
