// ppm_ctf_kernels.h — the averaged periodogram of a micrograph or a movie (ppm_ctf_spectrum) and the fit of defocus and astigmatism to
// spectra (ppm_ctf_fit, second half of this file); DESIGN.md §2g.  gfx950 / CDNA4, wave64.
//
//   k_ctf_tile_rows   gathers 16 rows of one tile from the image (the mean of the group's frames), two real rows per complex transform,
//                     transforms them in LDS (lds_fft), untangles the pair and writes the rows' half spectra
//   k_ctf_tile_cols   a block owns a strip of columns of the half plane and one CHUNK of tiles: per tile the column transforms in LDS,
//                     |F|^2 added into the block's own sums in walk order; the chunk's partial goes out with plain stores
//   k_ctf_fold        the chunks' partials summed in order, divided by the number of tiles
//   k_ctf_normalise   the reference's own scaling: [0, 0] = 0, then divide by the maximum (one block)
//
// Every sum has a fixed order that depends on the plan alone (ppm_ctf_plan.h): no floating-point atomics, two calls agree bit for bit.
#pragma once
#include "ppm_dev.h"
#include "ppm_ctf_plan.h"

namespace ppm {

struct CtfTilesP {
    const float *img;                // [nframes][ny][nx]
    float2 *half;                    // [tiles of this trip][T][W] row-transformed tiles
    float *part;                     // [chunks][T][W]
    FftPlan plan;                    // of length T
    int T, W;                        // tile, T / 2 + 1
    int nx, ny, nframes, group;
    int tiles_x, tiles_y;
    long tile0, ntiles;              // first tile of this trip (walk order: group, tile row, tile column) and how many it holds
    int vec;                         // 16-byte loads: the host has checked alignment and divisibility (host_ctf.h)
};

__global__ void __launch_bounds__(256) k_ctf_tile_rows(CtfTilesP P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, T = P.T, W = P.W, LS = T + 1;
    float2 *tw = (float2 *)smem, *A = tw + T;                                    // [pairs][LS]
    const long t = P.tile0 + blockIdx.y;                                          // tile in walk order
    const int r0 = blockIdx.x * kCtfRowsPerBlock;
    const int nl = min(kCtfRowsPerBlock, T - r0), np = nl >> 1;                  // T and the rows per block are even
    if (blockIdx.y >= P.ntiles || nl <= 0) return;
    const int per_g = P.tiles_x * P.tiles_y;
    const int gi = (int)(t / per_g), ti = (int)(t - (long)gi * per_g), ty = ti / P.tiles_x, tx = ti - ty * P.tiles_x;
    const int x0 = ctf_tile_origin(tx, P.nx, T), y0 = ctf_tile_origin(ty, P.ny, T);
    const int f0 = gi * P.group, nf = min(P.group, P.nframes - f0);
    const float inv_nf = 1.0f / (float)nf, inv_t = 1.0f / (float)T;
    const size_t plane = (size_t)P.nx * P.ny;
    for (int i = tid; i < T; i += 256) tw[i] = P.plan.tw[i];
    const float *src = P.img + (size_t)f0 * plane + (size_t)(y0 + r0) * P.nx + x0;

    // ---- gather: row 2 p is the real part of pair p, row 2 p + 1 the imaginary part; the frames of the group are added in order
    if (P.vec) {
        const int q = T >> 2;
        const float inv_q = 1.0f / (float)q;
        for (int i = tid; i < nl * q; i += 256) {
            const int line = fast_div(i, q, inv_q), e = 4 * (i - line * q);
            const float *s = src + (size_t)line * P.nx + e;
            float4 v = *(const float4 *)s;
            for (int f = 1; f < nf; f++) { const float4 u = *(const float4 *)(s + f * plane); v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w; }
            const float c[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; k++) ((float *)&A[(line >> 1) * LS + P.plan.perm[e + k]])[line & 1] = nf > 1 ? c[k] * inv_nf : c[k];
        }
    } else {
        for (int i = tid; i < nl * T; i += 256) {
            const int line = fast_div(i, T, inv_t), e = i - line * T;
            const float *s = src + (size_t)line * P.nx + e;
            float v = *s;
            for (int f = 1; f < nf; f++) v += s[f * plane];
            ((float *)&A[(line >> 1) * LS + P.plan.perm[e]])[line & 1] = nf > 1 ? v * inv_nf : v;
        }
    }
    lds_fft(A, P.plan, np, LS, false, tid, 256, tw);                             // opens with a barrier

    // ---- untangle Z = FFT(a + i b): A[k] = (Z[k] + conj Z[T - k]) / 2, B[k] = -i (Z[k] - conj Z[T - k]) / 2, k = 0 .. T / 2
    float2 *dst = P.half + ((size_t)blockIdx.y * T + r0) * W;
    const float inv_w = 1.0f / (float)W;
    for (int i = tid; i < nl * W; i += 256) {
        const int line = fast_div(i, W, inv_w), k = i - line * W;
        const float2 z = A[(line >> 1) * LS + k], zc = A[(line >> 1) * LS + (k ? T - k : 0)];
        float2 o;
        if (line & 1) o = make_float2(0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x));
        else o = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
        dst[i] = o;
    }
}

__global__ void __launch_bounds__(256) k_ctf_tile_cols(CtfTilesP P, int chunk0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, T = P.T, W = P.W, LS = T + 1, C = ctf_cols_per_block(T);
    float2 *tw = (float2 *)smem, *A = tw + T;                                    // [C][LS]
    float *acc = (float *)(A + (size_t)C * LS);                                  // [T][C]
    const int c0 = blockIdx.x * C, nc = min(C, W - c0);
    const long first = (long)blockIdx.y * kCtfChunkTiles;                        // the chunk's first tile within this trip
    if (nc <= 0 || first >= P.ntiles) return;
    const int nt = (int)min((long)kCtfChunkTiles, P.ntiles - first);
    const float inv_nc = 1.0f / (float)nc;
    for (int i = tid; i < T; i += 256) tw[i] = P.plan.tw[i];
    for (int i = tid; i < T * nc; i += 256) acc[i] = 0.f;
    for (int j = 0; j < nt; j++) {
        const float2 *src = P.half + (size_t)(first + j) * T * W + c0;
        lds_barrier();                                                           // the sums of the last tile have read A
        for (int i = tid; i < T * nc; i += 256) {
            const int ky = fast_div(i, nc, inv_nc), c = i - ky * nc;
            A[c * LS + P.plan.perm[ky]] = src[(size_t)ky * W + c];
        }
        lds_fft(A, P.plan, nc, LS, false, tid, 256, tw);
        for (int i = tid; i < T * nc; i += 256) {                                // element i stays with its thread: the order is the tiles'
            const int ky = fast_div(i, nc, inv_nc), c = i - ky * nc;
            const float2 v = A[c * LS + ky];
            acc[i] += v.x * v.x + v.y * v.y;
        }
    }
    float *dst = P.part + (size_t)(chunk0 + blockIdx.y) * T * W + c0;
    for (int i = tid; i < T * nc; i += 256) {
        const int ky = fast_div(i, nc, inv_nc), c = i - ky * nc;
        dst[(size_t)ky * W + c] = acc[i];
    }
}

// out[i] = (part[0][i] + part[1][i] + ...) / tiles
__global__ void __launch_bounds__(256) k_ctf_fold(const float *__restrict__ part, float *__restrict__ out, long per, long chunks, float tiles) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    float s = part[i];
    for (long c = 1; c < chunks; c++) s += part[c * per + i];
    out[i] = s / tiles;
}

// out[0] = 0; out /= max(out).  One block; the maximum of a set does not depend on the order it is taken in.
__global__ void __launch_bounds__(1024) k_ctf_normalise(float *__restrict__ out, long per) {
    __shared__ float red[16];
    float m = 0.f;                                                               // powers are >= 0
    for (long i = threadIdx.x; i < per; i += 1024) if (i > 0) m = fmaxf(m, out[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < 16; w++) m = fmaxf(m, red[w]);
    for (long i = threadIdx.x; i < per; i += 1024) out[i] = i > 0 ? out[i] / m : 0.f;
}

// ================================================================================== the fit (ppm_ctf_fit)
//   k_ctf_condition   one block per spectrum: ring means of sqrt(P) over the cropped half plane (a thread per ring walks the rows in order,
//                     in double), the box-averaged background, the fitted samples minus background minus their mean, their sum of squares
//   k_ctf_grid        the hot path: a thread per candidate, the samples staged through LDS 256 at a time; |c| of a (candidate, sample)
//                     pair is formed once and used against up to four spectra that share the window; no reduction across threads at all
//   k_ctf_argmax      per spectrum the best grid score, ties to the lowest candidate index
//   k_ctf_refine      one block per spectrum runs the whole pattern search: seven trials per pass over the samples (the current point, scored
//                     once, and its six neighbours)
//   k_ctf_profile     one block per spectrum, in double: fit resolution, the six avrot rows and the diagnostic image for the refined parameters
struct CtfFitP {
    const float *spectra;            // [n][T][W] powers
    const float4 *geo;               // [ns] (s^2 in 1/A^2, cos 2 phi, sin 2 phi, 0) of the fitted samples, scan order
    const int *pos, *ring;           // [ns] index into a spectrum, ring
    float *v, *V;                    // [n][ns] conditioned samples, [n] their sums of squares
    const double *lo;                // [n] first mean defocus of every spectrum's window
    const int *ni;                   // [n] mean-defocus steps of every window
    float *scores; long scores_ld;   // [n][scores_ld] grid scores
    int *best; float *best_score; double *refined;      // [n] grid winner and its score, [n][4] (mean defocus, astigmatism, angle in degrees, score)
    int n, T, W, B, R, ns, bg_w, nc, nj, group;       // R = B / 2 rings above 0; group: spectra per block of k_ctf_grid
    double step, tol;
    float k1, k2, extra;             // pi lambda, Cs lambda^2 / 2, the amplitude-contrast phase
    float c2a[kCtfThetas], s2a[kCtfThetas];
};

// block sum of a double in a fixed order: lanes by xor shuffles, then the four waves in order; every thread gets the result
__device__ __forceinline__ double block_sum_d(double a, double *red) {
    a = wave_sum_d(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ring means of sqrt(P) over the cropped half plane (a thread per ring walks the rows in order) and the box-averaged background without
// ring 0; all threads of the block must call; ends with a barrier
__device__ inline void ctf_rings(const float *pw, const CtfFitP &P, double *mean, double *bg) {
    const int tid = threadIdx.x, R = P.R, W = P.W, T = P.T;
    for (int r = tid; r <= R; r += 256) {
        const int lo2 = r ? r * r - r + 1 : 0, hi2 = r * r + r;                  // ring r: lo2 <= kx^2 + ky^2 <= hi2
        double sum = 0.0; int cnt = 0;
        for (int ky = -R; ky < R; ky++) {
            const int y2 = ky * ky, need = lo2 - y2;
            if (y2 > hi2) continue;
            int kx = need <= 0 ? 0 : (int)sqrtf((float)need);
            while (kx * kx < need) kx++;
            while (kx > 0 && (kx - 1) * (kx - 1) >= need) kx--;
            const float *row = pw + (size_t)(ky < 0 ? ky + T : ky) * W;
            for (; kx <= R && kx * kx + y2 <= hi2; kx++) { sum += sqrt((double)row[kx]); cnt++; }
        }
        mean[r] = cnt ? sum / cnt : 0.0;
    }
    __syncthreads();
    for (int r = tid; r <= R; r += 256) {
        const int a = max(1, r - P.bg_w), b = max(a, min(R, r + P.bg_w));         // ring 0 is the image's mean, not background
        double sum = 0.0;
        for (int q = a; q <= b; q++) sum += mean[q];
        bg[r] = sum / (b - a + 1);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) k_ctf_condition(CtfFitP P) {
    __shared__ double mean[257], bg[257], red[4];
    const int tid = threadIdx.x, s = blockIdx.x, T = P.T, W = P.W;
    const float *pw = P.spectra + (size_t)s * T * W;
    ctf_rings(pw, P, mean, bg);
    double part = 0.0;
    for (int i = tid; i < P.ns; i += 256) part += sqrt((double)pw[P.pos[i]]) - bg[P.ring[i]];
    const double m = block_sum_d(part, red) / P.ns;
    part = 0.0;
    float *v = P.v + (size_t)s * P.ns;
    for (int i = tid; i < P.ns; i += 256) {
        const float x = (float)(sqrt((double)pw[P.pos[i]]) - bg[P.ring[i]] - m);
        v[i] = x; part += (double)x * x;
    }
    const double V = block_sum_d(part, red);
    if (tid == 0) P.V[s] = (float)V;
}

// |CTF| of ppm_dev.h's ctf_eval_fast at a sample: the phase reduced to one revolution, the hardware sine
__device__ __forceinline__ float ctf_abs_fast(const float4 g, float dsum, float ddif, float c2a, float s2a, float k1, float k2, float extra) {
    const float df = 0.5f * (dsum + ddif * (g.y * c2a + g.z * s2a));
    const float chi = k1 * g.x * (df - k2 * g.x) + extra;
    float rev = chi * 0.15915494309189535f; rev -= floorf(rev);
    return fabsf(__sinf(6.283185307179586f * rev));
}

__global__ void __launch_bounds__(256) k_ctf_grid(CtfFitP P) {
    __shared__ float4 geo[kCtfSampleChunk];
    __shared__ float vv[kCtfGridSpectra][kCtfSampleChunk];
    const int tid = threadIdx.x, s0 = blockIdx.y * P.group, nsp = min(P.group, P.n - s0);
    const int idx = blockIdx.x * 256 + tid, ncand = P.ni[s0] * P.nc;                // spectra of one block share the window
    if (idx >= ncand && idx < P.scores_ld)                                          // past this window's candidates: the map says so
        for (int q = 0; q < nsp; q++) P.scores[(size_t)(s0 + q) * P.scores_ld + idx] = __builtin_nanf("");
    if (blockIdx.x * 256 >= ncand) return;
    const int i = idx / P.nc, c = idx - i * P.nc, j = c ? (c - 1) / kCtfThetas + 1 : 0, k = c ? (c - 1) % kCtfThetas : 0;
    const float dsum = (float)(2.0 * (P.lo[s0] + i * P.step)), ddif = (float)(j * P.step), c2a = P.c2a[k], s2a = P.s2a[k];
    float N[kCtfGridSpectra] = { 0.f, 0.f, 0.f, 0.f }, C = 0.f;
    for (int b0 = 0; b0 < P.ns; b0 += kCtfSampleChunk) {
        const int m = min(kCtfSampleChunk, P.ns - b0);
        __syncthreads();
        if (tid < m) {
            geo[tid] = P.geo[b0 + tid];
            for (int q = 0; q < nsp; q++) vv[q][tid] = P.v[(size_t)(s0 + q) * P.ns + b0 + tid];
        }
        __syncthreads();
        float n4[kCtfGridSpectra] = { 0.f, 0.f, 0.f, 0.f }, cc = 0.f;
        for (int t = 0; t < m; t++) {
            const float a = ctf_abs_fast(geo[t], dsum, ddif, c2a, s2a, P.k1, P.k2, P.extra);
            cc += a * a;
#pragma unroll
            for (int q = 0; q < kCtfGridSpectra; q++) if (q < nsp) n4[q] += vv[q][t] * a;
        }
        C += cc;
#pragma unroll
        for (int q = 0; q < kCtfGridSpectra; q++) N[q] += n4[q];
    }
    if (idx >= ncand) return;
    const float pen = P.tol > 0 ? (float)((j * P.step / P.tol) * (j * P.step / P.tol) / (2.0 * P.ns)) : 0.f;
#pragma unroll
    for (int q = 0; q < kCtfGridSpectra; q++)
        if (q < nsp) {
            const float den = P.V[s0 + q] * C;
            P.scores[(size_t)(s0 + q) * P.scores_ld + idx] = (den > 0.f ? N[q] / sqrtf(den) : 0.f) - pen;
        }
}

__global__ void __launch_bounds__(256) k_ctf_argmax(CtfFitP P) {
    __shared__ float rv[4]; __shared__ int ri[4];
    const int tid = threadIdx.x, s = blockIdx.x, ncand = P.ni[s] * P.nc;
    const float *sc = P.scores + (size_t)s * P.scores_ld;
    float bv = -3.0e38f; int bi = 0x7fffffff;
    for (int o = tid; o < ncand; o += 256) { const float v = sc[o]; if (v > bv) { bv = v; bi = o; } }      // ascending: the first of equals stays
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, 64); const int oi = __shfl_xor(bi, m, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
        P.best_score[s] = bi < ncand ? bv : 0.f;
        P.best[s] = bi < ncand ? bi : 0;                                      // nothing comparable (NaN scores): stay inside the grid
    }
}

__global__ void __launch_bounds__(256) k_ctf_refine(CtfFitP P) {
    __shared__ float redN[4][7], redC[4][7];
    const int tid = threadIdx.x, s = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *v = P.v + (size_t)s * P.ns;
    const float Vs = P.V[s];
    const int idx = P.best[s], gi = idx / P.nc, gc = idx - gi * P.nc;
    double cur[3] = { P.lo[s] + gi * P.step, gc ? ((gc - 1) / kCtfThetas + 1) * P.step : 0.0, gc ? ((gc - 1) % kCtfThetas) * (180.0 / kCtfThetas) : 0.0 };
    double steps[3] = { P.step, P.step, 180.0 / kCtfThetas };
    float best = 0.f;
    // trial 0 is the current point (first pass only), trials 1 .. 6 its neighbours: axis (q - 1) / 2, + before -
    for (int level = -1; level <= kCtfHalvings; level++) {
        for (int sweep = 0; sweep < (level < 0 ? 1 : kCtfSweeps); sweep++) {
            float dsum[7], ddif[7], c2a[7], s2a[7]; bool ok[7];
#pragma unroll
            for (int q = 0; q < 7; q++) {
                double t[3] = { cur[0], cur[1], cur[2] };
                ok[q] = level < 0 ? q == 0 : q > 0;
                if (q > 0) {
                    const int ax = (q - 1) >> 1;
                    t[ax] += ((q - 1) & 1) ? -steps[ax] : steps[ax];
                    if (t[1] < 0.0 || (ax == 2 && cur[1] == 0.0)) ok[q] = false;
                }
                const float th2 = (float)(t[2] * (2.0 * 3.14159265358979323846 / 180.0));
                dsum[q] = (float)(2.0 * t[0]); ddif[q] = (float)t[1]; c2a[q] = cosf(th2); s2a[q] = sinf(th2);
            }
            float N[7] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, C[7] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
            for (int i = tid; i < P.ns; i += 256) {
                const float4 g = P.geo[i]; const float x = v[i];
#pragma unroll
                for (int q = 0; q < 7; q++) {
                    const float a = ctf_abs_fast(g, dsum[q], ddif[q], c2a[q], s2a[q], P.k1, P.k2, P.extra);
                    N[q] += x * a; C[q] += a * a;
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 7; q++) {
                const float a = wave_sum(N[q]), b = wave_sum(C[q]);
                if (lane == 0) { redN[wave][q] = a; redC[wave][q] = b; }
            }
            __syncthreads();
            int mv = -1; float ms = best;
#pragma unroll
            for (int q = 0; q < 7; q++) {
                const float n = redN[0][q] + redN[1][q] + redN[2][q] + redN[3][q], c = redC[0][q] + redC[1][q] + redC[2][q] + redC[3][q];
                const float den = Vs * c;
                float sc = den > 0.f ? n / sqrtf(den) : 0.f;
                if (P.tol > 0) sc -= (float)((double)ddif[q] / P.tol * ((double)ddif[q] / P.tol) / (2.0 * P.ns));
                if (level < 0) { if (q == 0) best = sc; }
                else if (ok[q] && sc > ms) { ms = sc; mv = q; }
            }
            if (level < 0) break;
            if (mv < 0) break;
#pragma unroll
            for (int ax = 0; ax < 3; ax++)                                       // compile-time indices: the state stays in registers
                if (ax == (mv - 1) >> 1) cur[ax] += ((mv - 1) & 1) ? -steps[ax] : steps[ax];
            best = ms;
        }
        if (level >= 0) { steps[0] *= 0.5; steps[1] *= 0.5; steps[2] *= 0.5; }
    }
    if (tid == 0) { double *o = P.refined + (size_t)s * 4; o[0] = cur[0]; o[1] = cur[1]; o[2] = cur[2]; o[3] = (double)best; }
}

// k_ctf_profile: for the refined parameters of every spectrum, in double (one block per spectrum; nothing here is hot):
//   prof[s][0][r] = r / (B a)                        frequency of ring r, 1/A
//   prof[s][1][r] = mean(A) - background             rotational average of the conditioned spectrum (0 at r = 0)
//   prof[s][2][r]                                    the same averaged along equiphase lines: a pixel at |k|, phi counts for ring
//                                                    floor(|k| sqrt(df(phi) / dbar) + 1/2), where the mean-defocus CTF has its phase (Cs aside)
//   prof[s][3][r] = |CTF|(r / (B a); dbar)           the fitted 1-D curve
//   prof[s][4][r]                                    quality: correlation of rows 2 and 3 over the rings r - w .. r + w inside 1 .. B/2
//   prof[s][5][r] = 1 / sqrt(pixels of that window)  noise level: the deviation of such a correlation under noise alone
//   prof[s][6][0]                                    fit resolution: 1 / s of the first ring beyond min_res whose quality is below
//                                                    kCtfFitThreshold (of the last ring when none is)
// diag (may be null): [s][B][B] centred image, conditioned spectrum where kx >= 0, fitted |CTF| (with astigmatism) where kx < 0.
__global__ void __launch_bounds__(256) k_ctf_profile(CtfFitP P, double *prof, float *diag, double a_fit, double min_res) {
    __shared__ double mean[257], bg[257], eq[257], fit[257], cnt[257];
    const int tid = threadIdx.x, s = blockIdx.x, R = P.R, W = P.W, T = P.T, NR = R + 1, B = P.B;
    const float *pw = P.spectra + (size_t)s * T * W;
    ctf_rings(pw, P, mean, bg);
    const double *rf = P.refined + (size_t)s * 4;
    const double dbar = rf[0], delta = rf[1], th2 = rf[2] * (2.0 * 3.14159265358979323846 / 180.0), c2a = cos(th2), s2a = sin(th2);
    const bool warp = dbar > 0.0 && dbar - 0.5 * delta > 0.0;
    const double fmin = warp ? sqrt((dbar - 0.5 * delta) / dbar) : 1.0, fmax = warp ? sqrt((dbar + 0.5 * delta) / dbar) : 1.0;
    const double k1 = (double)P.k1, k2c = (double)P.k2, extra = (double)P.extra, inv_ba = 1.0 / (B * a_fit);
    for (int r = tid; r <= R; r += 256) {
        const double klo = (r - 0.5) / fmax - 1.0 > 0.0 ? (r - 0.5) / fmax - 1.0 : 0.0, khi = (r + 0.5) / fmin + 1.0;   // |k| of the pixels that can land in ring r, with a margin
        double sum = 0.0; int n = 0;
        for (int ky = -R; ky < R; ky++) {
            const double y2 = (double)ky * ky;
            if (y2 > khi * khi) continue;
            int kx = klo * klo > y2 ? (int)sqrt(klo * klo - y2) : 0;
            const float *row = pw + (size_t)(ky < 0 ? ky + T : ky) * W;
            for (; kx <= R && (double)kx * kx + y2 <= khi * khi; kx++) {
                const int k2 = kx * kx + ky * ky, ring = (int)floor(sqrt((double)k2) + 0.5);
                if (ring > R) continue;
                double f = 1.0;
                if (warp && k2 > 0) f = sqrt((dbar + 0.5 * delta * (((double)(kx * kx - ky * ky) * c2a + 2.0 * kx * ky * s2a) / k2)) / dbar);
                if ((int)floor(sqrt((double)k2) * f + 0.5) != r) continue;
                sum += sqrt((double)row[kx]) - bg[ring]; n++;
            }
        }
        eq[r] = n && r ? sum / n : 0.0; cnt[r] = (double)n;
        const double s2 = (r * inv_ba) * (r * inv_ba);
        fit[r] = fabs(sin(k1 * s2 * (dbar - k2c * s2) + extra));
    }
    __syncthreads();
    double *o = prof + (size_t)s * (6 * NR + 1);
    for (int r = tid; r <= R; r += 256) {
        const int a = max(1, r - P.bg_w), b = max(a, min(R, r + P.bg_w)), m = b - a + 1;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0, np = 0;
        for (int q = a; q <= b; q++) { sx += eq[q]; sy += fit[q]; np += cnt[q]; }
        sx /= m; sy /= m;
        for (int q = a; q <= b; q++) { const double x = eq[q] - sx, y = fit[q] - sy; sxx += x * x; syy += y * y; sxy += x * y; }
        o[r] = r * inv_ba; o[NR + r] = r ? mean[r] - bg[r] : 0.0; o[2 * NR + r] = eq[r]; o[3 * NR + r] = fit[r];
        o[4 * NR + r] = sxx > 0.0 && syy > 0.0 ? sxy / sqrt(sxx * syy) : 0.0;
        o[5 * NR + r] = np > 0.0 ? 1.0 / sqrt(np) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double res = 1.0 / (R * inv_ba);
        for (int r = 1; r <= R; r++)
            if (r * inv_ba > 1.0 / min_res && o[4 * NR + r] < kCtfFitThreshold) { res = 1.0 / (r * inv_ba); break; }
        o[6 * NR] = res;
    }
    if (!diag) return;
    float *d = diag + (size_t)s * B * B;
    for (int i = tid; i < B * B; i += 256) {
        const int y = i / B, x = i - y * B, ky = y - R, kx = x - R;
        float val = 0.f;
        const int k2 = kx * kx + ky * ky, ring = (int)floor(sqrt((double)k2) + 0.5);
        if (kx >= 0) { if (ring <= R && ring > 0) val = (float)(sqrt((double)pw[(size_t)(ky < 0 ? ky + T : ky) * W + kx]) - bg[ring]); }
        else {
            const double s2 = k2 * inv_ba * inv_ba, df = dbar + 0.5 * delta * (((double)(kx * kx - ky * ky) * c2a + 2.0 * kx * ky * s2a) / k2);
            val = (float)fabs(sin(k1 * s2 * (df - k2c * s2) + extra));
        }
        d[i] = val;
    }
}

}  // namespace ppm
