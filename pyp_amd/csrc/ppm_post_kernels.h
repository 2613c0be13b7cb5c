// ppm_post_kernels.h — post-processing of two half maps (ppm_postprocess) for gfx950 / CDNA4, wave64.
//
//   k_post_pack        Z = H1 + i H2, times the clamped mask where there is one
//   k_post_scale_mask  Z *= scale x clamped mask: the back-transformed randomised halves, ahead of their masked transform
//   k_post_shells      per shell: sum Re F1 F2*, sum |F1|^2, sum |F2|^2 and the number of coefficients, as per-block partials
//   k_post_shell_sum   the partials added in block order
//   k_post_randomise   new phases for every conjugate pair from shell s_r on, out of place
//   k_post_weight      Z *= W[shell] / N^3, zero beyond shell N/2
//   k_post_out         the two output maps, with the flips
//   k_post_mean        A = (H1 + H2) / 2 for the automatic mask;  k_post_fill, k_post_count: a constant map, voxels with M >= 0.5
//   k_post_sphere_sums block partials of sum L, sum L^2 (double) and the voxel count over the sphere; k_post_sphere_total adds them in block order
//   k_post_key_hist    histogram of 16 bits of the order-preserving integer image of L over the sphere (integer atomics only)
//
// One complex transform carries both halves: with p the index-space partner of k ((N - i) mod N per axis),
//   F1(k) = (Z(k) + conj Z(p)) / 2,   F2(k) = (Z(k) - conj Z(p)) / 2i.
// Nothing here adds floating-point numbers with an atomic: every sum has one order, fixed by N alone, so two calls agree bit for bit.
#pragma once
#include "ppm_dev.h"

namespace ppm {

constexpr int kPostYSplit = 4;                 // k_post_shells: blocks per kz plane; a block's 4 wavefronts take every 16th ky row
constexpr unsigned short kPostNoShell = 0xffffu;   // shell table: beyond shell N/2
constexpr int kPostSumBlocks = 1024;           // k_post_sphere_sums, k_post_count: blocks, whatever the box

__device__ __forceinline__ float post_clamp01(float m) { return fminf(fmaxf(m, 0.f), 1.f); }

__global__ void k_post_pack(const float *__restrict__ h1, const float *__restrict__ h2, const float *__restrict__ mask, float2 *__restrict__ z, size_t n3) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    float a = h1[i], b = h2[i];
    if (mask) { const float m = post_clamp01(mask[i]); a *= m; b *= m; }
    z[i] = make_float2(a, b);
}

__global__ void k_post_scale_mask(float2 *__restrict__ z, const float *__restrict__ mask, float scale, size_t n3) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const float2 v = z[i];
    float a = v.x * scale, b = v.y * scale;
    if (mask) { const float m = post_clamp01(mask[i]); a *= m; b *= m; }
    z[i] = make_float2(a, b);
}

__device__ __forceinline__ int post_signed(int i, int n) { return i < n / 2 ? i : i - n; }

// Grid (N, kPostYSplit), 256 threads.  A wavefront walks kx = 0 .. N/2 of its (ky, kz) rows 64 at a time.  Along x the shell does not
// decrease, so equal shells are runs of neighbouring lanes: an inclusive segmented sum over the lanes (six fixed shuffle steps), then
// the last lane of every run adds the run's four numbers into the wavefront's own LDS bins.  The runs of one step have different shells,
// the steps follow each other in program order, so no two lanes ever add into one bin at a time.  Interior kx stand for the pair (k, p)
// and count twice; the planes kx = 0 and N/2 meet both members (at (ky, kz) and at its partner row) and count once.
// partial: [gridDim.x * gridDim.y][ns][4] doubles.
__global__ void __launch_bounds__(256) k_post_shells(const float2 *__restrict__ z, const unsigned short *__restrict__ shell_of, int n, int ns,
                                                     double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *bins = (double *)smem;                                     // [4 wavefronts][ns + 1][4]; bin ns takes what lies beyond shell N/2
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = (ns + 1) * 4;
    for (int i = threadIdx.x; i < 4 * nb; i += 256) bins[i] = 0.0;
    __syncthreads();
    double *mine = bins + wave * nb;
    const int kz = blockIdx.x, pz = (n - kz) % n, sz = post_signed(kz, n);
    const int half = n / 2;
    for (int ky = blockIdx.y * 4 + wave; ky < n; ky += 4 * kPostYSplit) {
        const int py = (n - ky) % n, sy = post_signed(ky, n);
        const float2 *row = z + ((size_t)kz * n + ky) * n, *prow = z + ((size_t)pz * n + py) * n;
        const int k2yz = sy * sy + sz * sz;
        for (int x0 = 0; x0 <= half; x0 += 64) {
            const int kx = x0 + lane;
            int s = ns;
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
            if (kx <= half) {
                const unsigned short sh = shell_of[k2yz + kx * kx];
                if (sh != kPostNoShell) {
                    s = sh;
                    const float2 zk = row[kx], zp = prow[(n - kx) % n];
                    const double a = zk.x, b = zk.y, c = zp.x, d = zp.y;
                    const double w = (kx == 0 || kx == half) ? 0.25 : 0.5;                 // (1 or 2 members) / 4
                    const double f1r = a + c, f1i = b - d, f2r = b + d, f2i = c - a;      // 2 F1, 2 F2
                    v0 = w * (f1r * f2r + f1i * f2i);
                    v1 = w * (f1r * f1r + f1i * f1i);
                    v2 = w * (f2r * f2r + f2i * f2i);
                    v3 = w * 4.0;
                }
            }
            for (int o = 1; o < 64; o <<= 1) {
                const int so = __shfl_up(s, o);
                const double u0 = __shfl_up(v0, o), u1 = __shfl_up(v1, o), u2 = __shfl_up(v2, o), u3 = __shfl_up(v3, o);
                if (lane >= o && so == s) { v0 += u0; v1 += u1; v2 += u2; v3 += u3; }
            }
            const int sn = __shfl_down(s, 1);
            if (lane == 63 || sn != s) {
                double *bin = mine + s * 4;
                bin[0] += v0; bin[1] += v1; bin[2] += v2; bin[3] += v3;
            }
        }
    }
    __syncthreads();
    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ns * 4;
    for (int i = threadIdx.x; i < ns * 4; i += 256) out[i] = ((bins[i] + bins[nb + i]) + bins[2 * nb + i]) + bins[3 * nb + i];
}

// sums[ns][4] = the partials of k_post_shells, block 0 first
__global__ void k_post_shell_sum(const double *__restrict__ partial, int nblocks, int ns4, double *__restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns4) return;
    double a = 0.0;
    for (int b = 0; b < nblocks; b++) a += partial[(size_t)b * ns4 + i];
    sums[i] = a;
}

__device__ __forceinline__ unsigned post_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// One thread per coefficient; the member of a pair with the smaller linear index does the work of both.  From shell s_r on (what lies
// beyond shell N/2 included) F1 and F2 keep their moduli and take the phases of the pair's hash; the partner gets the conjugates.
__global__ void k_post_randomise(const float2 *__restrict__ zin, float2 *__restrict__ zout, const unsigned short *__restrict__ shell_of, int n, int s_r,
                                 unsigned seed_mul) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int y = blockIdx.y, zc = blockIdx.z;
    const int px = (n - x) % n, py = (n - y) % n, pz = (n - zc) % n;
    const size_t i = ((size_t)zc * n + y) * n + x, p = ((size_t)pz * n + py) * n + px;
    if (i > p) return;
    const float2 zi = zin[i];
    if (i == p) { zout[i] = zi; return; }
    const float2 zp = zin[p];
    const int sx = post_signed(x, n), sy = post_signed(y, n), sz = post_signed(zc, n);
    const int sh = shell_of[sx * sx + sy * sy + sz * sz];
    if (sh < s_r) { zout[i] = zi; zout[p] = zp; return; }
    const float f1r = 0.5f * (zi.x + zp.x), f1i = 0.5f * (zi.y - zp.y), f2r = 0.5f * (zi.y + zp.y), f2i = 0.5f * (zp.x - zi.x);
    const float m1 = sqrtf(f1r * f1r + f1i * f1i), m2 = sqrtf(f2r * f2r + f2i * f2i);
    const unsigned h1 = post_mix32((unsigned)i ^ seed_mul), h2 = post_mix32(h1 ^ 0x85EBCA6Bu);
    float s1, c1, s2, c2;
    sincospif((float)(h1 >> 8) * (1.0f / 8388608.0f), &s1, &c1);       // 2 pi (h >> 8) / 2^24
    sincospif((float)(h2 >> 8) * (1.0f / 8388608.0f), &s2, &c2);
    const float g1r = m1 * c1, g1i = m1 * s1, g2r = m2 * c2, g2i = m2 * s2;
    zout[i] = make_float2(g1r - g2i, g1i + g2r);                       // F1 + i F2
    zout[p] = make_float2(g1r + g2i, g2r - g1i);                       // conj F1 + i conj F2
}

__global__ void k_post_weight(float2 *__restrict__ z, const unsigned short *__restrict__ shell_of, const float *__restrict__ wtab, int n) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int y = blockIdx.y, zc = blockIdx.z;
    const int sx = post_signed(x, n), sy = post_signed(y, n), sz = post_signed(zc, n);
    const unsigned short sh = shell_of[sx * sx + sy * sy + sz * sz];
    const float w = sh != kPostNoShell ? wtab[sh] : 0.f;
    const size_t i = ((size_t)zc * n + y) * n + x;
    const float2 v = z[i];
    z[i] = make_float2(v.x * w, v.y * w);
}

// unmasked = (Re + Im) / 2 of the filtered pair, masked = the stored unmasked value times the clamped mask; a flip writes the voxel at
// the mirrored index of both maps
__global__ void k_post_out(const float2 *__restrict__ z, const float *__restrict__ mask, float *__restrict__ unmasked, float *__restrict__ masked, int n,
                           int fx, int fy, int fz) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int y = blockIdx.y, zc = blockIdx.z;
    const size_t i = ((size_t)zc * n + y) * n + x;
    const size_t o = ((size_t)(fz ? n - 1 - zc : zc) * n + (fy ? n - 1 - y : y)) * n + (fx ? n - 1 - x : x);
    const float2 v = z[i];
    const float u = 0.5f * (v.x + v.y);
    unmasked[o] = u;
    masked[o] = mask ? u * post_clamp01(mask[i]) : u;
}

__global__ void k_post_mean(const float *__restrict__ h1, const float *__restrict__ h2, float *__restrict__ a, size_t n3) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) a[i] = 0.5f * (h1[i] + h2[i]);
}

__global__ void k_post_fill(float *__restrict__ a, float v, size_t n3) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) a[i] = v;
}

__global__ void __launch_bounds__(256) k_post_count(const float *__restrict__ mask, size_t n3, unsigned long long *__restrict__ count) {
    __shared__ unsigned s_c[256];
    unsigned c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (size_t)gridDim.x * 256) c += mask[i] >= 0.5f ? 1u : 0u;
    s_c[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_c[threadIdx.x] += s_c[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_c[0]) atomicAdd(count, (unsigned long long)s_c[0]);
}

__device__ __forceinline__ bool post_in_sphere(size_t i, int n, long long r2) {
    const int x = (int)(i % n), y = (int)((i / n) % n), zc = (int)(i / ((size_t)n * n));
    const int c = n / 2;
    const long long d2 = (long long)(x - c) * (x - c) + (long long)(y - c) * (y - c) + (long long)(zc - c) * (zc - c);
    return d2 <= r2;
}

// src: the real parts of the complex work array.  Block b takes the voxels b * 256 + t, then every gridDim.x * 256 further on; a thread
// adds its own in that order, the block adds its threads in a fixed tree.  partial: [gridDim.x][3] doubles.
__global__ void __launch_bounds__(256) k_post_sphere_sums(const float2 *__restrict__ src, int n, long long r2, double *__restrict__ partial) {
    __shared__ double s0[256], s1[256], s2[256];
    const size_t n3 = (size_t)n * n * n;
    double a = 0.0, q = 0.0, c = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (size_t)gridDim.x * 256) {
        if (post_in_sphere(i, n, r2)) { const double v = src[i].x; a += v; q += v * v; c += 1.0; }
    }
    s0[threadIdx.x] = a; s1[threadIdx.x] = q; s2[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s0[threadIdx.x] += s0[threadIdx.x + o]; s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[blockIdx.x * 3] = s0[0]; partial[blockIdx.x * 3 + 1] = s1[0]; partial[blockIdx.x * 3 + 2] = s2[0]; }
}

__global__ void k_post_sphere_total(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
    if (threadIdx.x >= 3 || blockIdx.x) return;
    double a = 0.0;
    for (int b = 0; b < nblocks; b++) a += partial[b * 3 + threadIdx.x];
    out[threadIdx.x] = a;
}

// the integers order as the floats do (-0 below +0; the low-passed map holds no NaN)
__device__ __forceinline__ unsigned post_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// pass 0: hist[key >> 16]; pass 1: hist[key & 0xffff] over the voxels whose upper half equals `prefix`
__global__ void k_post_key_hist(const float2 *__restrict__ src, int n, long long r2, int pass, unsigned prefix, unsigned *__restrict__ hist) {
    const size_t n3 = (size_t)n * n * n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3 || !post_in_sphere(i, n, r2)) return;
    const unsigned k = post_key(src[i].x);
    if (pass == 0) atomicAdd(&hist[k >> 16], 1u);
    else if ((k >> 16) == prefix) atomicAdd(&hist[k & 0xffffu], 1u);
}

}  // namespace ppm
