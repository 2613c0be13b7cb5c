// ppm_ctf_plan.h — the host rules of CTF estimation (ppm_ctf_spectrum, ppm_ctf_fit, host_ctf.h): how the tiles walk
// an image, how the frames of a movie fall into groups, how a call's tiles are cut into chunks with a fixed order of summation, the
// sizes of the workspaces, and the crop, sample range and grid counts of a fit, all fixed before the first launch.
// Plain C++, no HIP types: compiled alone by tests/test_ctf_cpu.py; tests/f64_ctf.py states the same rules in numpy.
#pragma once

#include <algorithm>

#include "ppm_resample_plan.h"

namespace ppm {

constexpr int kCtfChunkTiles = 16;          // tiles one block of k_ctf_tile_cols sums, in walk order, into one partial
constexpr int kCtfRowsPerBlock = 16;        // real rows (two per complex transform) of one block of k_ctf_tile_rows
constexpr long kCtfHalfBudget = 256L << 20; // bytes of row-transformed tiles held between the two passes

// tile sizes the line transforms take (ensure_plan): those of the resampler
inline bool ctf_tile_ok(int t) { return resample_len_ok(t); }

// Tiles along an axis of n samples, as the reference's periodogram walks it with binning 1: origins 0, T/2, 2 T/2, ... (n / (T/2) of
// them), an origin whose tile would leave the image pulled back to n - T.  Where T/2 divides n the last origin is pulled back onto
// the one before it and that tile counts twice; the rule is kept as it is.  0: the axis is shorter than a tile.
inline int ctf_axis_tiles(int n, int t) { return n < t ? 0 : n / (t / 2); }
constexpr int ctf_tile_origin(int i, int n, int t) { const int o = i * (t / 2); return o + t > n ? n - t : o; }

// frames averaged together: groups of `group` frames in order, the last one holding what is left
inline int ctf_groups(int nframes, int group) { return (nframes + group - 1) / group; }

// columns of the half plane a block of k_ctf_tile_cols transforms at once, and the dynamic LDS of the two kernels
constexpr int ctf_cols_per_block(int t) { return t > 256 ? 8 : 16; }
inline long ctf_rows_lds(int t) { return 8L * t + 8L * (kCtfRowsPerBlock / 2) * (t + 1); }
inline long ctf_cols_lds(int t) { const long c = ctf_cols_per_block(t); return 8L * t + 8L * c * (t + 1) + 4L * c * t; }

struct CtfSpectrumPlan {
    int ok = 0;                 // 0: refused, `why` says so
    const char *why = "";
    int tile = 0, half_w = 0;   // T, T / 2 + 1
    int tiles_x = 0, tiles_y = 0, groups = 0;
    long tiles = 0;             // groups * tiles_y * tiles_x: what the average divides by
    long chunks = 0;            // partial sums, ceil(tiles / kCtfChunkTiles)
    long pass_tiles = 0;        // tiles transformed per trip through the two passes: a multiple of kCtfChunkTiles inside kCtfHalfBudget
    long half_floats2 = 0;      // workspace: complex half spectra of a trip, pass_tiles * T * (T / 2 + 1)
    long part_floats = 0;       // workspace: chunks * T * (T / 2 + 1)
    long out_floats = 0;        // the result, T * (T / 2 + 1)
    int vec = 0;                // 16-byte loads of the image (the pointer's own alignment is the caller's to add)
};

inline CtfSpectrumPlan ctf_spectrum_plan(int nx, int ny, int nframes, int group, int tile) {
    CtfSpectrumPlan p;
    p.tile = tile;
    if (!ctf_tile_ok(tile)) { p.why = "the tile is not a size the transforms take"; return p; }
    if (nx < 1 || ny < 1 || nframes < 1) { p.why = "the image is empty"; return p; }
    if (group < 1 || group > nframes) { p.why = "the number of frames to average must be 1 .. the number of frames"; return p; }
    if (nx < tile || ny < tile) { p.why = "the image is smaller than one tile"; return p; }
    if ((long)nx * ny > (1L << 31) - 1 - tile) { p.why = "the image has more than 2^31 pixels"; return p; }
    p.half_w = tile / 2 + 1;
    p.tiles_x = ctf_axis_tiles(nx, tile); p.tiles_y = ctf_axis_tiles(ny, tile); p.groups = ctf_groups(nframes, group);
    p.tiles = (long)p.groups * p.tiles_y * p.tiles_x;
    p.chunks = (p.tiles + kCtfChunkTiles - 1) / kCtfChunkTiles;
    const long per = (long)tile * p.half_w;
    long fit = kCtfHalfBudget / (8 * per) / kCtfChunkTiles * kCtfChunkTiles;
    if (fit < kCtfChunkTiles) fit = kCtfChunkTiles;
    p.pass_tiles = fit < p.chunks * kCtfChunkTiles ? fit : p.chunks * kCtfChunkTiles;
    p.half_floats2 = p.pass_tiles * per;
    p.part_floats = p.chunks * per;
    p.out_floats = per;
    p.vec = nx % 4 == 0 && tile % 8 == 0;       // every origin, the pulled-back one included, is then a multiple of 4 pixels
    p.ok = 1;
    return p;
}

// ---------------------------------------------------------------------------------- the fit (ppm_ctf_fit)
constexpr double kCtfResampleTarget = 1.4;  // ctffind's "target pixel size after resampling", which PYP leaves at its default
constexpr double kCtfAstigCap = 1000.0;     // largest astigmatism of the grid when no restraint is given (the pattern search may leave it)
constexpr int kCtfThetas = 12;              // grid angles, 15 degrees apart
constexpr int kCtfHalvings = 10, kCtfSweeps = 8;       // levels of the pattern search after the first, sweeps per level at most
constexpr int kCtfGridSpectra = 4;          // spectra of a batch with one shared window that a block of k_ctf_grid scores against one |c|
constexpr double kCtfFitThreshold = 0.5;     // the fit resolution is where the windowed correlation of data and fitted curve first falls below it
constexpr int kCtfSampleChunk = 256;        // samples a block of k_ctf_grid stages at a time; sums run per chunk, then over the chunks

struct CtfFitPlan {
    int ok = 0;
    const char *why = "";
    int B = 0;                  // B_fit: the centre crop in Fourier space that brings a pixel below 1.4 A up to it (T otherwise)
    double a = 0;               // a_fit = pixel T / B_fit
    int k2lo = 0, k2hi = 0;     // fitted samples: k2lo <= kx^2 + ky^2 <= k2hi (min_res >= 1 / s >= max_res, inside the ring B_fit / 2)
    int bg_w = 0;               // half width of the background's box average, in rings
    int nj = 0, nc = 0;         // astigmatism steps above 0; candidates per mean defocus, 1 + 12 nj
    long max_samples = 0;       // room for the sample list: (B_fit / 2 + 1) B_fit
};

inline CtfFitPlan ctf_fit_plan(int tile, double pixel, double min_res, double max_res, double step, double tol) {
    CtfFitPlan p;
    if (tile < 8 || tile > 512 || tile % 2) { p.why = "the spectrum's size must be even, 8 .. 512"; return p; }
    if (!(pixel > 0) || !(min_res > max_res) || !(max_res > 0) || !(step > 0) || !(tol >= 0)) { p.why = "pixel, resolutions (minimum > maximum > 0), step and restraint must be positive"; return p; }
    p.B = tile; p.a = pixel;
    if (pixel < kCtfResampleTarget) { p.B = 2 * (int)std::floor(tile * pixel / kCtfResampleTarget / 2.0); if (p.B >= 8) p.a = pixel * tile / p.B; }
    if (p.B < 8) { p.why = "the pixel is too small for this spectrum"; return p; }
    const double rlo = p.B * p.a / min_res, rhi = p.B * p.a / max_res, half = p.B / 2.0;
    p.k2lo = (int)std::ceil(rlo * rlo); if (p.k2lo < 1) p.k2lo = 1;
    p.k2hi = (int)std::floor(std::min(rhi * rhi, half * half));
    if (p.k2hi < p.k2lo) { p.why = "no sample lies between the two resolutions"; return p; }
    p.bg_w = (int)std::ceil(rlo);
    const double nj = std::floor((tol > 0 ? tol : kCtfAstigCap) / step + 1e-9);
    if (nj > 64) { p.why = "more than 64 astigmatism steps"; return p; }
    p.nj = (int)nj; p.nc = 1 + kCtfThetas * p.nj;
    p.max_samples = (long)(p.B / 2 + 1) * p.B;
    p.ok = 1;
    return p;
}

// mean-defocus steps of one window: lo, lo + step, ... <= hi; 0: an empty or oversized window
inline long ctf_window_steps(double lo, double hi, double step) {
    if (!(hi >= lo) || !(lo > 0)) return 0;
    const double n = std::floor((hi - lo) / step + 1e-9) + 1;
    return n > 100000 ? 0 : (long)n;
}

}  // namespace ppm
