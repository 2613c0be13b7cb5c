// ppm_frame_kernels.h — movie-frame refinement of libpypmatch (gfx950): per-frame score maps over a grid of shifts, their pooling over
// neighbouring frames and the peak of every pooled map (ppm_frame_refine, host_frames.h).
//
// A GROUP is the set of frame rows of one particle in one tilt (PIND, TIND), ordered by FIND.  The own map of a frame row r is
//     S_r(d) = sum_k al Re(I conj(m_d)) / sqrt(sum_k al |m|^2 sum_k al |I|^2),   m_d = w CTF slice e^{-2 pi i k.(s_r + d) / N}
// over the band r_lo <= |k| < r_hi, all rings signed, for d = (jx, jy) h, |j| <= W: the K5 local score (k_local, k_csp_eval) at the row's
// pose and defocus with its shift moved by d.  Image values and CTF weights come from k_prep unchanged (Il = w I, cw = w CTF).
#pragma once
#include "ppm_csp_kernels.h"
#include "ppm_frame_plan.h"

namespace ppm {

constexpr int kFrameThreads = 256;
constexpr int kFrameTile = 2048;                                      // samples a pass holds in LDS (X and the sample coordinates, 16 bytes each)
constexpr int kFrameMaxSide = 2 * PPM_FRAME_MAX_STEPS + 1;
constexpr int kFrameMaxPts = kFrameMaxSide * kFrameMaxSide;           // 289: at most two grid points per thread
constexpr size_t kFrameLdsLimit = (size_t)64 * 1024;                  // what one block may ask for: two blocks fit the 160 KiB of a CU
static_assert(kFrameMaxPts <= 2 * kFrameThreads, "two grid points per thread");
static_assert(kFrameTile % kFrameThreads == 0 && kFrameTile % 16 == 0, "a tile is whole trips of the block and whole 16-sample groups");

// dynamic LDS of k_frame_maps: X and coordinates of a tile, the waves' partial power sums, and the slice store when it is kept in LDS
__host__ __device__ inline size_t frame_lds_fixed() { return (size_t)kFrameTile * 16 + 64; }
__host__ __device__ inline bool frame_store_in_lds(int S_used) { return frame_lds_fixed() + (size_t)S_used * 8 <= kFrameLdsLimit; }
__host__ __device__ inline size_t frame_lds_bytes(int S_used) { return frame_lds_fixed() + (frame_store_in_lds(S_used) ? (size_t)S_used * 8 : 0); }

struct FrameMapP {
    CubeView cv; const uint32_t *samples; const float2 *Il; const float *cw;
    int S_pad, N, S_used; float rlo2, rmax2;
    int W; float h;                 // the grid: (2 W + 1)^2 points, h pixels apart
    const int *goff;                // [n_groups + 1] a group's frames in the frame list
    const int *frow;                // [n_frames] row (= image) of a frame; a group's frames ascend in FIND
    const int *fproc;               // [n_frames] the order in which a group's frames are scored: frames of equal pose and CTF parameters side by side
    const int *fnew;                // [n_frames] by position in that order: the frame starts a run, the slice is gathered for it
    const float *fm6;               // [n_frames][6] first two columns of the row's matrix M (m00 m01 m10 m11 m20 m21)
    const float *fsh;               // [n_frames][2] the row's shift, pixels
    float2 *scratch;                // [n_groups][S_used] slice store in global memory; null: the store is in LDS
    float *own;                     // [n_frames][(2 W + 1)^2] own maps, row-major (jy, jx)
};

// Block = one group, 256 threads.  Per run of frames the lanes take SAMPLES and gather the slice once into the store.  Per frame and tile of
// the ring-ordered list the lanes take samples again: X = al c I conj(slice) and the sample's coordinates go to LDS, the two power sums to
// the waves' cells; then the lanes take SHIFTS: a thread walks the tile out of LDS (every lane reads the same address: a broadcast) for
// its one or two grid points, 16 samples to a float partial, the partials to a double.  No atomics.  A grid point's sum runs in list
// order whatever thread holds it; the power sums are per-thread strided sums combined by wave_sum and then wave by wave, per tile, in tile
// order - the block size and the tile are constants, so a result depends on neither the grid nor the other groups of the launch.
__global__ void __launch_bounds__(kFrameThreads) k_frame_maps(FrameMapP P) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    float2 *const X = (float2 *)fsm, *const kxy = X + kFrameTile;
    float *const red = (float *)(kxy + kFrameTile);                // [2][4], 64 bytes reserved
    const int S_used = P.S_used;
    float2 *const store = P.scratch ? P.scratch + (size_t)blockIdx.x * S_used : (float2 *)(red + 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = P.goff[blockIdx.x], f1 = P.goff[blockIdx.x + 1];
    const int side = 2 * P.W + 1, npts = side * side;
    const float invN = 1.0f / (float)P.N;
    CubeView one = P.cv; one.scale = 1.f;
    for (int p = f0; p < f1; p++) {
        const int f = P.fproc[p], j = P.frow[f];
        if (P.fnew[p]) {            // block-uniform
            __syncthreads();        // the frame before has read the store to its end
            const float *m = P.fm6 + (size_t)f * 6;
            const float ma = m[0] * P.cv.scale, mb = m[1] * P.cv.scale, mc = m[2] * P.cv.scale, md = m[3] * P.cv.scale, me = m[4] * P.cv.scale, mf = m[5] * P.cv.scale;
            for (int s = tid; s < S_used; s += kFrameThreads) {
                int kx, ky, al, ring;
                unpack_sample(P.samples[s], kx, ky, al, ring);
                const float fkx = (float)kx, fky = (float)ky;
                store[s] = cube_interp(cube_fetch(one, ma * fkx + mb * fky, mc * fkx + md * fky, me * fkx + mf * fky));
            }
        }
        const float2 *Il = P.Il + (size_t)j * P.S_pad; const float *cw = P.cw + (size_t)j * P.S_pad;
        const float sx = P.fsh[2 * f], sy = P.fsh[2 * f + 1];
        double acc[2] = { 0.0, 0.0 }, sB = 0.0, sC = 0.0;
        for (int t0 = 0; t0 < S_used; t0 += kFrameTile) {
            const int nT = S_used - t0 < kFrameTile ? S_used - t0 : kFrameTile;
            __syncthreads();        // the store is written; the tile before has been walked
            // ---- lanes = samples
            float pB = 0.f, pC = 0.f;
            for (int s = t0 + tid; s < t0 + nT; s += kFrameThreads) {
                int kx, ky, al, ring;
                unpack_sample(P.samples[s], kx, ky, al, ring);
                const float k2 = (float)(kx * kx + ky * ky);
                if (!(k2 < P.rmax2 && k2 >= P.rlo2)) al = 0;
                const float2 iv = Il[s], v = store[s]; const float c = cw[s];
                const float fal = (float)al;
                pC += fal * (iv.x * iv.x + iv.y * iv.y);
                const float ac = fal * c, ax = ac * iv.x, ay = ac * iv.y, w = ac * c;
                pB += w * (v.x * v.x + v.y * v.y);
                X[s - t0] = make_float2(ax * v.x + ay * v.y, ay * v.x - ax * v.y);
                kxy[s - t0] = make_float2((float)kx, (float)ky);
            }
            pB = wave_sum(pB); pC = wave_sum(pC);
            if (lane == 0) { red[wave] = pB; red[4 + wave] = pC; }
            __syncthreads();
            sB += (double)(((red[0] + red[1]) + red[2]) + red[3]); sC += (double)(((red[4] + red[5]) + red[6]) + red[7]);
            // ---- lanes = shifts
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const int q = tid + c * kFrameThreads;
                if (q >= npts) continue;
                const int jy = q / side, jx = q - jy * side;
                const float nx = -(sx + (float)(jx - P.W) * P.h) * invN, ny = -(sy + (float)(jy - P.W) * P.h) * invN;
                double a = 0.0;
                for (int g0 = 0; g0 < nT; g0 += 16) {       // S_used is whole 16-sample groups (every ring is padded to them)
                    float part = 0.f;
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const float2 k = kxy[g0 + i], x = X[g0 + i];
                        float rev = k.x * nx + k.y * ny;                        // phase in revolutions
                        rev -= floorf(rev);
                        part += x.x * __cosf(6.283185307179586f * rev) + x.y * __sinf(6.283185307179586f * rev);
                    }
                    a += (double)part;
                }
                acc[c] += a;
            }
        }
        const double inv = (sB > 0 && sC > 0) ? 1.0 / sqrt(sB * sC) : 0.0;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int q = tid + c * kFrameThreads;
            if (q < npts) P.own[(size_t)f * npts + q] = (float)(acc[c] * inv);
        }
    }
}

struct FramePeakP {
    int W; float h; int half_width;
    const int *goff;                // [n_groups + 1]
    const int *ffind;               // [n_frames] FIND of a frame
    const double *gw;               // [n_gw] pooling weight by |FIND difference| (built on the host in double); beyond the table: not pooled
    int n_gw;
    const float *own;               // [n_frames][npts]
    float *pooled;                  // [n_frames][npts]
    int *amax;                      // [n_frames] arg-max of the pooled map
    double *delta;                  // [n_frames][2] shift found, pixels: grid point plus the parabolic offsets
    float *score;                   // [n_frames][2] own map at the arg-max, own map at d = 0
};

// Block = one group, one wave.  For every frame r: P_r(d) = sum g(FIND' - FIND_r) S_r'(d) / sum g over the group's frames within half_width,
// added in ascending FIND in double; the arg-max in row-major order with ties to the lower index; per axis the parabolic offset where the
// arg-max is off the window's edge and the three values are strictly concave.
__global__ void __launch_bounds__(64) k_frame_peak(FramePeakP P) {
    extern __shared__ __attribute__((aligned(16))) char psm[];
    double *const Pb = (double *)psm;           // [npts]
    const int lane = threadIdx.x, f0 = P.goff[blockIdx.x], f1 = P.goff[blockIdx.x + 1];
    const int side = 2 * P.W + 1, npts = side * side;
    for (int r = f0; r < f1; r++) {
        const int fr = P.ffind[r];
        double bv = -1e300; int bq = 0x7fffffff;
        for (int q = lane; q < npts; q += 64) {
            double num = 0.0, den = 0.0;
            for (int r2 = f0; r2 < f1; r2++) {
                long d = (long)P.ffind[r2] - (long)fr; if (d < 0) d = -d;
                if (d > (long)P.half_width || d >= (long)P.n_gw) continue;
                const double g = P.gw[d];
                num += g * (double)P.own[(size_t)r2 * npts + q]; den += g;
            }
            const double v = num / den;         // the frame itself is always in its pool: den >= 1
            Pb[q] = v; P.pooled[(size_t)r * npts + q] = (float)v;
            if (v > bv) { bv = v; bq = q; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bv, m, 64); const int oq = __shfl_xor(bq, m, 64);
            if (ov > bv || (ov == bv && oq < bq)) { bv = ov; bq = oq; }
        }
        __syncthreads();
        if (lane == 0) {
            const int jy = bq / side, jx = bq - jy * side;
            double dx = (double)(jx - P.W) * (double)P.h, dy = (double)(jy - P.W) * (double)P.h;
            const double c = Pb[bq];
            if (jx > 0 && jx < side - 1) {
                const double l = Pb[bq - 1], rr = Pb[bq + 1], cur = l - 2.0 * c + rr;
                if (cur < 0.0) dx += 0.5 * (l - rr) / cur * (double)P.h;
            }
            if (jy > 0 && jy < side - 1) {
                const double l = Pb[bq - side], rr = Pb[bq + side], cur = l - 2.0 * c + rr;
                if (cur < 0.0) dy += 0.5 * (l - rr) / cur * (double)P.h;
            }
            P.amax[r] = bq; P.delta[2 * r] = dx; P.delta[2 * r + 1] = dy;
            P.score[2 * r] = P.own[(size_t)r * npts + bq]; P.score[2 * r + 1] = P.own[(size_t)r * npts + (size_t)P.W * side + P.W];
        }
        __syncthreads();
    }
}

}  // namespace ppm
