// ppm_locres_kernels.h — local resolution of two half maps (ppm_local_resolution) for gfx950 / CDNA4, wave64.
//
//   k_lr_init      inside / alive byte map (mask > 0.5, or the sphere |x - c| < N/2), the map filled with 100, the inside count
//   k_lr_pack      Z = A + i D, A = (H1 + H2) / 2, D = (H1 - H2) / 2
//   k_lr_band      out = Z^ x b[|k|^2], out of place: Z^ stays resident for the next level
//   k_lr_square    (re, im) -> (re^2, im^2) in place
//   k_lr_window    Z^ x W[|k|^2] in place
//   k_lr_key_hist  histogram of 16 bits of the order-preserving integer image of E_D (the imaginary parts) over the inside voxels
//   k_lr_assign    pass test E_A > tau, alive update, level write, count of the voxels still alive
//
// All of them stream: every access to a map is 16 bytes per lane (two complex numbers, four floats or four bytes of the byte map), lanes
// side by side.  N is even, so a row of complex numbers starts on a 16-byte boundary and N^3 is a multiple of 8.  The filters are tables
// over the integer |k|^2 (at most 3 x 256^2 + 1 floats = 768 KB), which stay in L2; a thread takes a run of two x, steps |k|^2 from one
// to the next and uses the pair of weights for the four rows (+-ky, +-kz).  The only atomics add integers, so two calls agree bit for bit.
#pragma once
#include "ppm_dev.h"

namespace ppm {

constexpr int kLrBlocks = 1024;                // k_lr_init, k_lr_key_hist1, k_lr_assign: at most this many blocks of 256 threads
constexpr int kLrHist0Blocks = 256;            // k_lr_key_hist0: at most this many blocks of 1024 threads
constexpr int kLrHist0Bins = 32768;            // pass 0: the upper 16 bits of a non-negative float (sign bit clear)
constexpr unsigned char kLrInside = 1, kLrAlive = 2;

__device__ __forceinline__ int lr_signed(int i, int n) { return i < n / 2 ? i : i - n; }

// a block's count into one 64-bit counter: a fixed tree over its 256 threads, then one integer atomic
__device__ __forceinline__ void lr_block_count(unsigned c, unsigned long long *__restrict__ counter) {
    __shared__ unsigned s_c[256];
    s_c[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_c[threadIdx.x] += s_c[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_c[0]) atomicAdd(counter, (unsigned long long)s_c[0]);
}

// One thread per four voxels of the linear array at a time (N^3 is a multiple of 8).
__global__ void __launch_bounds__(256) k_lr_init(const float *__restrict__ mask, unsigned char *__restrict__ state, float *__restrict__ res, int n, float fill,
                                                 unsigned long long *__restrict__ n_inside) {
    const size_t n3 = (size_t)n * n * n, quads = n3 / 4;
    const int c = n / 2;
    unsigned cnt = 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
        const size_t i = q * 4;
        bool in[4];
        if (mask) {
            const float4 m = *(const float4 *)(mask + i);
            in[0] = m.x > 0.5f; in[1] = m.y > 0.5f; in[2] = m.z > 0.5f; in[3] = m.w > 0.5f;
        } else {
            for (int j = 0; j < 4; j++) {
                const size_t v = i + j;
                const int x = (int)(v % n), y = (int)((v / n) % n), z = (int)(v / ((size_t)n * n));
                const int d2 = (x - c) * (x - c) + (y - c) * (y - c) + (z - c) * (z - c);
                in[j] = 4 * d2 < n * n;
            }
        }
        const unsigned char on = kLrInside | kLrAlive;
        for (int j = 0; j < 4; j++) cnt += in[j] ? 1u : 0u;
        *(uchar4 *)(state + i) = make_uchar4(in[0] ? on : 0, in[1] ? on : 0, in[2] ? on : 0, in[3] ? on : 0);
        *(float4 *)(res + i) = make_float4(fill, fill, fill, fill);
    }
    lr_block_count(cnt, n_inside);
}

// One thread per four voxels: two 16-byte loads, two 16-byte stores
__global__ void __launch_bounds__(256) k_lr_pack(const float *__restrict__ h1, const float *__restrict__ h2, float2 *__restrict__ z, size_t quads) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const size_t i = q * 4;
    const float4 a = *(const float4 *)(h1 + i), b = *(const float4 *)(h2 + i);
    float4 *o = (float4 *)(z + i);
    o[0] = make_float4(0.5f * (a.x + b.x), 0.5f * (a.x - b.x), 0.5f * (a.y + b.y), 0.5f * (a.y - b.y));
    o[1] = make_float4(0.5f * (a.z + b.z), 0.5f * (a.z - b.z), 0.5f * (a.w + b.w), 0.5f * (a.w - b.w));
}

// out[k] = in[k] x tab[|k|^2].  Grid (pairs of x, ky = 0 .. N/2, kz = 0 .. N/2): a thread takes the run x, x + 1 in the up to four rows
// (+-ky, +-kz), which share |k|^2, so one pair of table look-ups serves 64 bytes of the map; without the sharing the look-ups (64 lines
// of L2 per wavefront and load) cost more than the map's own traffic.  All loads are issued ahead of the stores.
__device__ __forceinline__ void lr_filter_rows(const float2 *in, float2 *out, const float *__restrict__ tab, int n) {
    const int half = n / 2;
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= half) return;
    const int x = 2 * px, y = blockIdx.y, z = blockIdx.z;                 // y, z <= N/2: their squares are those of the signed indices
    const int my = (n - y) % n, mz = (n - z) % n;
    const int sx = lr_signed(x, n);
    const int k2 = sx * sx + y * y + z * z;
    // x + 1 follows x on the same side of N/2 unless it is N/2 itself (odd N/2), where the index turns to -N/2
    const int k2n = x + 1 == half ? k2 - sx * sx + half * half : k2 + 2 * sx + 1;
    const float w0 = tab[k2], w1 = tab[k2n];
    const bool ty = my != y, tz = mz != z;
    const size_t r0 = ((size_t)z * n + y) * n + x, r1 = ((size_t)z * n + my) * n + x, r2 = ((size_t)mz * n + y) * n + x, r3 = ((size_t)mz * n + my) * n + x;
    float4 v0 = *(const float4 *)(in + r0), v1, v2, v3;
    if (ty) v1 = *(const float4 *)(in + r1);
    if (tz) v2 = *(const float4 *)(in + r2);
    if (ty && tz) v3 = *(const float4 *)(in + r3);
    *(float4 *)(out + r0) = make_float4(v0.x * w0, v0.y * w0, v0.z * w1, v0.w * w1);
    if (ty) *(float4 *)(out + r1) = make_float4(v1.x * w0, v1.y * w0, v1.z * w1, v1.w * w1);
    if (tz) *(float4 *)(out + r2) = make_float4(v2.x * w0, v2.y * w0, v2.z * w1, v2.w * w1);
    if (ty && tz) *(float4 *)(out + r3) = make_float4(v3.x * w0, v3.y * w0, v3.z * w1, v3.w * w1);
}

__global__ void __launch_bounds__(256) k_lr_band(const float2 *__restrict__ zin, float2 *__restrict__ zout, const float *__restrict__ btab, int n) {
    lr_filter_rows(zin, zout, btab, n);
}

__global__ void __launch_bounds__(256) k_lr_window(float2 *z, const float *__restrict__ wtab, int n) {
    lr_filter_rows(z, z, wtab, n);
}

__global__ void __launch_bounds__(256) k_lr_square(float2 *__restrict__ z, size_t pairs) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    float4 *q = (float4 *)(z + p * 2);
    const float4 v = *q;
    *q = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
}

// non-negative floats order as their bits do; anything with the sign bit set (round-off below zero, -0) counts as 0
__device__ __forceinline__ unsigned lr_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? 0u : u;
}

// Pass 0: hist[key >> 16], 32768 bins.  A block counts into its own LDS bins first (neighbouring voxels of a smoothed map share their
// upper bits, which would queue up on a few addresses of global memory) and adds its non-empty bins to the global ones at the end.
// Dynamic LDS: kLrHist0Bins x 4 bytes = 128 KB, so one block of 1024 threads per compute unit.  One thread per four voxels at a time.
__global__ void __launch_bounds__(1024) k_lr_key_hist0(const float2 *__restrict__ e, const unsigned char *__restrict__ state, size_t quads, unsigned *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *bins = (unsigned *)smem;
    for (int i = threadIdx.x; i < kLrHist0Bins; i += 1024) bins[i] = 0u;
    __syncthreads();
    for (size_t q = (size_t)blockIdx.x * 1024 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 1024) {
        const uchar4 s = *(const uchar4 *)(state + q * 4);
        if (!(s.x | s.y | s.z | s.w)) continue;
        const float4 *p = (const float4 *)(e + q * 4);
        const float4 v0 = p[0], v1 = p[1];
        if (s.x) atomicAdd(&bins[lr_key(v0.y) >> 16], 1u);
        if (s.y) atomicAdd(&bins[lr_key(v0.w) >> 16], 1u);
        if (s.z) atomicAdd(&bins[lr_key(v1.y) >> 16], 1u);
        if (s.w) atomicAdd(&bins[lr_key(v1.w) >> 16], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLrHist0Bins; i += 1024) { const unsigned c = bins[i]; if (c) atomicAdd(&hist[i], c); }
}

// Pass 1: hist[key & 0xffff], 65536 bins, over the inside voxels whose upper half equals `prefix`: few voxels, spread over many bins
__global__ void __launch_bounds__(256) k_lr_key_hist1(const float2 *__restrict__ e, const unsigned char *__restrict__ state, size_t quads, unsigned prefix,
                                                      unsigned *__restrict__ hist) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
        const uchar4 s = *(const uchar4 *)(state + q * 4);
        if (!(s.x | s.y | s.z | s.w)) continue;
        const float4 *p = (const float4 *)(e + q * 4);
        const float4 v0 = p[0], v1 = p[1];
        const unsigned k0 = lr_key(v0.y), k1 = lr_key(v0.w), k2 = lr_key(v1.y), k3 = lr_key(v1.w);
        if (s.x && (k0 >> 16) == prefix) atomicAdd(&hist[k0 & 0xffffu], 1u);
        if (s.y && (k1 >> 16) == prefix) atomicAdd(&hist[k1 & 0xffffu], 1u);
        if (s.z && (k2 >> 16) == prefix) atomicAdd(&hist[k2 & 0xffffu], 1u);
        if (s.w && (k3 >> 16) == prefix) atomicAdd(&hist[k3 & 0xffffu], 1u);
    }
}

// alive <- alive and E_A > tau; a voxel still alive takes `level`; alive_count += the voxels still alive.  One thread per four voxels at
// a time; a group with no voxel alive reads and writes nothing else.
__global__ void __launch_bounds__(256) k_lr_assign(const float2 *__restrict__ e, unsigned char *__restrict__ state, float *__restrict__ res, size_t quads, float tau,
                                                   float level, unsigned long long *__restrict__ alive_count) {
    unsigned cnt = 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
        uchar4 s = *(const uchar4 *)(state + q * 4);
        if (!((s.x | s.y | s.z | s.w) & kLrAlive)) continue;
        const float4 *p = (const float4 *)(e + q * 4);
        const float4 v0 = p[0], v1 = p[1];
        float4 r = *(const float4 *)(res + q * 4);
        if (s.x & kLrAlive) { if (v0.x > tau) { r.x = level; cnt++; } else s.x = kLrInside; }
        if (s.y & kLrAlive) { if (v0.z > tau) { r.y = level; cnt++; } else s.y = kLrInside; }
        if (s.z & kLrAlive) { if (v1.x > tau) { r.z = level; cnt++; } else s.z = kLrInside; }
        if (s.w & kLrAlive) { if (v1.z > tau) { r.w = level; cnt++; } else s.w = kLrInside; }
        *(uchar4 *)(state + q * 4) = s;
        *(float4 *)(res + q * 4) = r;
    }
    lr_block_count(cnt, alive_count);
}

}  // namespace ppm
