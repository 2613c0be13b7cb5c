// ppm_rank.h — the k-th value of a set of floats from two histograms of 16 bits each of an order-preserving 32-bit key: the integer
// decisions the host makes between the two passes (host_volume.h: rank_two_pass; ppm_postprocess for the volume-fraction threshold of
// the automatic mask, ppm_local_resolution for tau).  Plain C++, no HIP types: compiled alone by tests/test_rank_cpu.py.
//
// Pass 0 counts the keys by their upper half, pass 1 the keys whose upper half is the bin found in pass 0 by their lower half; the two
// bins together are the key of the value asked for.  The keys themselves are made on the device (post_key, lr_key).
#pragma once

#include <cmath>
#include <cstring>

namespace ppm {

struct RankBin {
    int bin;            // the bin that holds the value asked for; -1: the histogram holds fewer than `want` values
    long long want;     // which of that bin's values it is, counted from the side the walk came from (1 = the first)
};

// The bin of the want-th value (1 = the first), counted from bin 0 upwards or, from_top, from the last bin downwards
inline RankBin rank_walk(const unsigned *hist, int bins, long long want, bool from_top) {
    long long passed = 0;
    for (int i = 0; i < bins; i++) {
        const int b = from_top ? bins - 1 - i : i;
        if (passed + hist[b] >= want) return {b, want - passed};
        passed += hist[b];
    }
    return {-1, want - passed};
}

inline long long rank_total(const unsigned *hist, int bins) {
    long long total = 0;
    for (int b = 0; b < bins; b++) total += hist[b];
    return total;
}

// The count that is the fraction f of a total: ceil(f total), at least 1 and at most the total
inline long long rank_of_fraction(double f, long long total) {
    const long long want = (long long)std::ceil(f * (double)total);
    return want < 1 || total < 1 ? 1 : want > total ? total : want;
}

// The rank, from the bottom, of the value that a fraction p of n values exceed: ceil((1 - p) n) in [1, n]
inline long locres_rank(double p, long n) {
    const double r = std::ceil((1.0 - p) * (double)n);
    return r < 1.0 ? 1 : r > (double)n ? n : (long)r;
}

// The float behind a key of signed values (the inverse of post_key: sign bit set = a non-negative float with its sign bit set, sign bit
// clear = a negative float, every bit flipped)
inline float rank_signed_key_value(unsigned key) {
    const unsigned u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

}  // namespace ppm
