// ppm_resample_plan.h — the host rules of Fourier resampling (ppm_resample, ppm_fit_volume, host_resample.h): which
// lengths the transforms take, the (n_c, P, M) search that fits a reference to a box and a pixel size, and how many lines a block of
// k_resample_lines holds.  Plain C++, no HIP types: compiled alone by tests/test_resample_cpu.py; tests/f64_resample.py states the
// same rules in numpy.
#pragma once

#include <cmath>

namespace ppm {

// lengths the line transforms take (box_ok of ppm_geom.h): even, 32..512, prime factors 2, 3, 5, 7 only
inline bool resample_len_ok(int n) {
    if (n < 32 || n > 512 || n % 2) return false;
    while (n % 2 == 0) n /= 2;
    while (n % 3 == 0) n /= 3;
    while (n % 5 == 0) n /= 5;
    while (n % 7 == 0) n /= 7;
    return n == 1;
}

// the supported lengths next to n: the largest one <= n (0: none) and the smallest one >= n (0: none)
inline void resample_nearest_ok(int n, int *below, int *above) {
    *below = 0; *above = 0;
    for (int k = n < 512 ? n : 512; k >= 32; k--) if (resample_len_ok(k)) { *below = k; break; }
    for (int k = n > 32 ? n : 32; k <= 512; k++) if (resample_len_ok(k)) { *above = k; break; }
}

constexpr double kFitTolerance = 0.01;      // the caller's own "same sampling" tolerance (preprocess/core.py:810-812)

struct FitPlan {
    int n_c = 0, P = 0, M = 0;              // what the output box can show of the input; the padded / cropped input; its resampled length
    double scale = 0, pixel_achieved = 0, rel_error = 0;
    bool ok = false;                        // rel_error <= kFitTolerance
};

// fit(reference of n_in voxels at pixel_in -> box_out at pixel_out): s = pixel_in / pixel_out, n_c = min(n_in, 2 ceil(B / (2 s)) + 2);
// among the supported (P, M) with P >= n_c the pair with the smallest |M / (P s) - 1|, ties to the smaller P M, then the smaller P.
// Sizes are checked by the caller (8 <= n_in, box_out <= 512, pixels positive).
inline FitPlan fit_plan(int n_in, double pixel_in, double pixel_out, int box_out) {
    FitPlan f;
    f.scale = pixel_in / pixel_out;
    const int want = 2 * (int)std::ceil((double)box_out / (2.0 * f.scale)) + 2;
    f.n_c = n_in < want ? n_in : want;
    double best = 1e300;
    for (int P = 32; P <= 512; P += 2) {
        if (P < f.n_c || !resample_len_ok(P)) continue;
        for (int M = 32; M <= 512; M += 2) {
            if (!resample_len_ok(M)) continue;
            const double err = std::fabs((double)M / ((double)P * f.scale) - 1.0);
            const bool better = err < best || (err == best && ((long)P * M < (long)f.P * f.M || ((long)P * M == (long)f.P * f.M && P < f.P)));
            if (better) { best = err; f.P = P; f.M = M; }
        }
    }
    if (f.P) {
        f.rel_error = best;
        f.pixel_achieved = pixel_in * (double)f.P / (double)f.M;
        f.ok = best <= kFitTolerance;
    }
    return f;
}

// Lines (two real lines per complex transform) a block of k_resample_lines holds: both work arrays at the odd line stride plus both
// twiddle tables inside `lds_bytes`, at most 32 lines, a multiple of 4 where 4 fit (the 16-byte accesses of the tiled passes).
inline int resample_lines_per_block(int n, int m, long lds_bytes) {
    const long tw = 8L * (n + m), pair = 8L * ((n + 1) + (m + 1));
    long pairs = (lds_bytes - tw) / pair;
    if (pairs < 1) return 0;
    if (pairs > 16) pairs = 16;
    if (pairs >= 2) pairs &= ~1L;
    return (int)(2 * pairs);
}
inline long resample_lines_lds(int n, int m, int lines) { return 8L * (n + m) + 8L * (lines / 2) * ((n + 1) + (m + 1)); }

}  // namespace ppm
