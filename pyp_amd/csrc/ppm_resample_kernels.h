// ppm_resample_kernels.h — Fourier resampling and real-space resizing of maps and image stacks (ppm_resample, ppm_resize,
// ppm_fit_volume) for gfx950 / CDNA4, wave64.
//
//   k_resample_lines   batched strided 1-D resampling N -> M of real lines, out of place: two lines per complex transform, the
//                      forward transform of length N, the crop / pad of the spectrum and the inverse of length M all in LDS
//   k_face_sums        per item (volume or image): sums over the face / edge voxels and the first two moments, in double, in a
//   k_face_stats       fixed order (block partials, then one block per item): pad value, mean, standard deviation
//   k_resize           crop / pad about the centre, optionally normalised
//
// The 1-D rule (X = unnormalised DFT of x, K = min(N, M), h = K / 2): Y[k mod M] = X[k mod N] for |k| < h; the Nyquist term of the
// smaller grid Y[h] = X[h] + X[N - h] (M < N), Y[h] = Y[M - h] = X[h] / 2 (M > N); everything else 0; y = (1 / N) IDFT_M(Y).  It is
// linear over the complex numbers, so z = a + i b carries two real lines through both transforms with nothing to untangle.
#pragma once
#include "ppm_dev.h"

namespace ppm {

struct ResampleLinesP {
    const float *src; float *dst;
    FftPlan pn, pm;                  // plans of the lengths N and M
    int N, M, L;                     // L: lines per block, even
    int line_major;                  // 0: a block's lines are rows, contiguous in src and in dst; 1: a tile of adjacent lines (stride 1 between lines)
    int vec;                         // 16-byte accesses: the host has checked alignment and divisibility (host_resample.h)
    long nlines, inner;              // line l starts at (l / inner) * outer + (l % inner) * inner_stride, its elements are `elem` apart
    long s_inner, s_outer, s_elem, d_inner, d_outer, d_elem;
    float scale;                     // 1 / N, applied once, to the spectrum on its way from one work array to the other
};

// where output frequency k2 of the length-M spectrum comes from: the index into X and a factor (0: no source, Y = 0; the second
// index serves the folded Nyquist term of a crop)
__device__ __forceinline__ void resample_source(int k2, int N, int M, int &ia, int &ib, float &f) {
    ib = -1; f = 1.f;
    if (M == N) { ia = k2; return; }
    const int h = (M < N ? M : N) >> 1;
    if (k2 < h) { ia = k2; return; }
    if (k2 > M - h) { ia = N - (M - k2); return; }
    if (M < N) { ia = h; ib = N - h; return; }           // k2 == h == M - h
    if (k2 == h || k2 == M - h) { ia = h; f = 0.5f; return; }
    ia = -1; f = 0.f;
}

// `np` packed lines held in A at the staging positions of the first plan -> their resampled lines in B, natural order: the forward
// transform, the spectrum's crop or pad into the staging positions of the second plan (times `scale`), the inverse transform.  All
// 256 threads of the block must call.
__device__ inline void resample_core(float2 *A, float2 *B, int np, const FftPlan &pn, const FftPlan &pm, float scale, int tid,
                                     const float2 *twn, const float2 *twm) {
    const int N = pn.n, M = pm.n, LSA = N + 1, LSB = M + 1;
    lds_fft(A, pn, np, LSA, false, tid, 256, twn);
    const float inv_m = 1.0f / (float)M;
    for (int i = tid; i < np * M; i += 256) {
        const int p = fast_div(i, M, inv_m), k2 = i - p * M;
        int ia, ib; float f;
        resample_source(k2, N, M, ia, ib, f);
        float2 v = make_float2(0.f, 0.f);
        if (ia >= 0) {
            v = A[p * LSA + ia];
            if (ib >= 0) v = cadd(v, A[p * LSA + ib]);
            f *= scale;
            v.x *= f; v.y *= f;
        }
        B[p * LSB + pm.perm[k2]] = v;
    }
    lds_fft(B, pm, np, LSB, true, tid, 256, twm);
}

__global__ void __launch_bounds__(256) k_resample_lines(ResampleLinesP P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, N = P.N, M = P.M, LSA = N + 1, LSB = M + 1;      // odd line strides: the tiled passes touch many lines at one element
    const int maxp = P.L >> 1;
    float2 *twn = (float2 *)smem, *twm = twn + N;                                 // the stages' twiddles of both plans
    float2 *A = twm + M, *B = A + (size_t)maxp * LSA;                             // [pairs][LSA], [pairs][LSB]
    const long l0 = (long)blockIdx.x * P.L;
    const int nl = (int)((P.nlines - l0) < P.L ? (P.nlines - l0) : P.L);
    if (nl <= 0) return;
    const int np = (nl + 1) >> 1, nl2 = 2 * np;                                   // an unpaired last line pairs with zero
    // (line, element) of work item i by a float quotient with one fix-up (fast_div), not an integer division per element
    const float inv_n = 1.0f / (float)N, inv_m = 1.0f / (float)M, inv_ng = 1.0f / (float)(nl >> 2 ? nl >> 2 : 1), inv_nl = 1.0f / (float)nl, inv_nl2 = 1.0f / (float)nl2;
    for (int i = tid; i < N; i += 256) twn[i] = P.pn.tw[i];
    for (int i = tid; i < M; i += 256) twm[i] = P.pm.tw[i];
    auto sbase = [&](int line) { const long l = l0 + line; return (l / P.inner) * P.s_outer + (l % P.inner) * P.s_inner; };
    auto dbase = [&](int line) { const long l = l0 + line; return (l / P.inner) * P.d_outer + (l % P.inner) * P.d_inner; };

    // ---- load: line 2 p is the real part of pair p, line 2 p + 1 the imaginary part, at the staging positions of the first plan
    if (P.line_major) {
        if (P.vec) {                                                              // nl % 4 == 0, four adjacent lines are 16 aligned bytes
            const int ng = nl >> 2;
            for (int i = tid; i < ng * N; i += 256) {
                const int e = fast_div(i, ng, inv_ng), g = i - e * ng;
                const float4 v = *(const float4 *)(P.src + sbase(4 * g) + (long)e * P.s_elem);
                const int pos = P.pn.perm[e];
                A[(2 * g) * LSA + pos] = make_float2(v.x, v.y);
                A[(2 * g + 1) * LSA + pos] = make_float2(v.z, v.w);
            }
        } else {
            for (int i = tid; i < nl2 * N; i += 256) {
                const int e = fast_div(i, nl2, inv_nl2), line = i - e * nl2;
                const float v = line < nl ? P.src[sbase(line) + (long)e * P.s_elem] : 0.f;
                ((float *)&A[(line >> 1) * LSA + P.pn.perm[e]])[line & 1] = v;
            }
        }
    } else {
        const float *s = P.src + sbase(0);                                        // nl rows, contiguous
        const int tot = nl * N, nv = P.vec ? tot >> 2 : 0;
        for (int i = tid; i < nv; i += 256) {
            const float4 v = *(const float4 *)(s + 4 * i);
            const float c[4] = { v.x, v.y, v.z, v.w };
            int line = fast_div(4 * i, N, inv_n), e = 4 * i - line * N;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                ((float *)&A[(line >> 1) * LSA + P.pn.perm[e]])[line & 1] = c[q];
                if (++e == N) { e = 0; line++; }
            }
        }
        for (int i = 4 * nv + tid; i < nl2 * N; i += 256) {                       // the rest, and the zeros of an unpaired line
            const int line = fast_div(i, N, inv_n), e = i - line * N;
            ((float *)&A[(line >> 1) * LSA + P.pn.perm[e]])[line & 1] = line < nl ? s[i] : 0.f;
        }
    }
    __syncthreads();
    resample_core(A, B, np, P.pn, P.pm, P.scale, tid, twn, twm);

    // ---- store
    if (P.line_major) {
        if (P.vec) {
            const int ng = nl >> 2;
            for (int i = tid; i < ng * M; i += 256) {
                const int e = fast_div(i, ng, inv_ng), g = i - e * ng;
                const float2 a = B[(2 * g) * LSB + e], b = B[(2 * g + 1) * LSB + e];
                *(float4 *)(P.dst + dbase(4 * g) + (long)e * P.d_elem) = make_float4(a.x, a.y, b.x, b.y);
            }
        } else {
            for (int i = tid; i < nl * M; i += 256) {
                const int e = fast_div(i, nl, inv_nl), line = i - e * nl;
                P.dst[dbase(line) + (long)e * P.d_elem] = ((const float *)&B[(line >> 1) * LSB + e])[line & 1];
            }
        }
    } else {
        float *d = P.dst + dbase(0);
        const int tot = nl * M, nv = P.vec ? tot >> 2 : 0;
        for (int i = tid; i < nv; i += 256) {
            float c[4];
            int line = fast_div(4 * i, M, inv_m), e = 4 * i - line * M;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                c[q] = ((const float *)&B[(line >> 1) * LSB + e])[line & 1];
                if (++e == M) { e = 0; line++; }
            }
            *(float4 *)(d + 4 * i) = make_float4(c[0], c[1], c[2], c[3]);
        }
        for (int i = 4 * nv + tid; i < tot; i += 256) {
            const int line = fast_div(i, M, inv_m), e = i - line * M;
            d[i] = ((const float *)&B[(line >> 1) * LSB + e])[line & 1];
        }
    }
}

// ---------------------------------------------------------------------------------- face means and moments
constexpr int kFaceChunk = 256 * 64;         // elements of an item one block of k_face_sums adds up

// is voxel i of an n^dims item on a face (3-D) or an edge (2-D)?  Every voxel counts once.
__device__ __forceinline__ bool on_face(long i, int n, int dims) {
    const int x = (int)(i % n), y = (int)((i / n) % n);
    bool f = x == 0 || x == n - 1 || y == 0 || y == n - 1;
    if (dims == 3) { const int z = (int)(i / ((long)n * n)); f = f || z == 0 || z == n - 1; }
    return f;
}

// block sum of three doubles in a fixed order: lanes by xor shuffles, then the four waves in order
__device__ __forceinline__ void block_sum3_d(double &a, double &b, double &c, double *red) {
    a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave * 3] = a; red[wave * 3 + 1] = b; red[wave * 3 + 2] = c; }
    __syncthreads();
    a = red[0] + red[3] + red[6] + red[9]; b = red[1] + red[4] + red[7] + red[10]; c = red[2] + red[5] + red[8] + red[11];
}

// part[(item * nchunk + chunk) * 3 + {0, 1, 2}] = sum over the chunk's face voxels, sum over all its voxels, sum of their squares
__global__ void __launch_bounds__(256) k_face_sums(const float *__restrict__ src, double *__restrict__ part, int n, int dims, long per, int nchunk) {
    __shared__ double red[12];
    const long item = blockIdx.y, c0 = (long)blockIdx.x * kFaceChunk;
    const float *s = src + item * per;
    double sf = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < kFaceChunk / 256; j++) {
        const long i = c0 + (long)j * 256 + threadIdx.x;
        if (i < per) {
            const double v = (double)s[i];
            s1 += v; s2 += v * v;
            if (on_face(i, n, dims)) sf += v;
        }
    }
    block_sum3_d(sf, s1, s2, red);
    if (threadIdx.x == 0) { double *o = part + (item * nchunk + blockIdx.x) * 3; o[0] = sf; o[1] = s1; o[2] = s2; }
}

// stats[item * 3 + {0, 1, 2}] = face mean, mean, standard deviation (of all voxels, divisor = their number)
__global__ void __launch_bounds__(256) k_face_stats(const double *__restrict__ part, double *__restrict__ stats, int n, int dims, long per, int nchunk) {
    __shared__ double red[12];
    const long item = blockIdx.x;
    double sf = 0.0, s1 = 0.0, s2 = 0.0;
    for (int c = threadIdx.x; c < nchunk; c += 256) { const double *p = part + (item * nchunk + c) * 3; sf += p[0]; s1 += p[1]; s2 += p[2]; }
    block_sum3_d(sf, s1, s2, red);
    if (threadIdx.x == 0) {
        const double inner = dims == 3 ? (double)(n - 2) * (n - 2) * (n - 2) : (double)(n - 2) * (n - 2);
        const double mean = s1 / (double)per, var = s2 / (double)per - mean * mean;
        stats[item * 3] = sf / ((double)per - inner); stats[item * 3 + 1] = mean; stats[item * 3 + 2] = var > 0.0 ? sqrt(var) : 0.0;
    }
}

// ---------------------------------------------------------------------------------- crop / pad about the centre
// out[i] = in[i - B / 2 + N / 2] per axis where that lies inside the input, the pad value elsewhere; normalize: (v - mean) / sd first, on
// the voxels and on the pad value alike (in double, rounded once).  pad_out[item] = the pad value as written.
__global__ void __launch_bounds__(256) k_resize(const float *__restrict__ src, float *__restrict__ dst, const double *__restrict__ stats,
                                                float *__restrict__ pad_out, int n, int b, int dims, int normalize) {
    const long per_out = dims == 3 ? (long)b * b * b : (long)b * b, per_in = dims == 3 ? (long)n * n * n : (long)n * n;
    const long i = (long)blockIdx.x * 256 + threadIdx.x, item = blockIdx.y;
    const double *st = stats + item * 3;
    const double mean = normalize ? st[1] : 0.0, inv = normalize ? 1.0 / st[2] : 1.0;
    const float pad = (float)((st[0] - mean) * inv);
    if (i == 0) pad_out[item] = pad;
    if (i >= per_out) return;
    const int off = n / 2 - b / 2;
    const int x = (int)(i % b) + off, y = (int)((i / b) % b) + off, z = dims == 3 ? (int)(i / ((long)b * b)) + off : 0;
    float v = pad;
    if (x >= 0 && x < n && y >= 0 && y < n && z >= 0 && z < n) {
        const float s = src[item * per_in + ((long)z * n + y) * n + x];
        v = normalize ? (float)(((double)s - mean) * inv) : s;
    }
    dst[item * per_out + i] = v;
}

}  // namespace ppm
