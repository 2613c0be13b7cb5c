// ppm_mask_kernels.h — shape masking of a reference map (ppm_mask_volume) for gfx950 / CDNA4, wave64.
//
//   k_mask_dx        core = {M >= 0.5}; windowed squared distance to the core along x, 16-bit, saturated at w^2
//   k_mask_dline     the same min-plus step along y (d2 -> d2) and along z; the z instance looks the cosine edge up by the
//                    integer d^2, takes the maximum with the clamped mask and writes the blended map (k_mask_dline<true>)
//   k_mask_r2c       map -> complex work array of the outside filter (no pre-compensation, unlike k_ref_load)
//   k_mask_lowpass   transform *= H(|k|) / N^3, H looked up by the integer |k|^2
//
// The distances are integers throughout: every voxel nearer than w to the core gets its exact squared Euclidean distance (each
// component of the offset to the nearest core voxel is below w, so the three windows hold it), everything else gets w^2.
#pragma once
#include "ppm_dev.h"

namespace ppm {

constexpr int kMaskMaxW = 64;            // widest cosine edge (voxels)
constexpr int kMaskTX = 64;              // x extent of a tile: one wavefront per row
constexpr int kMaskTL = 64;              // voxels of a tile along the axis of the pass
constexpr int kMaskLines = 8;            // x lines per block of k_mask_dx

// x pass.  A block takes kMaskLines consecutive lines (contiguous in memory); the core flags of the lines sit in LDS, a thread
// walks outwards from its voxel until it meets the core or the window ends.
__global__ void __launch_bounds__(256) k_mask_dx(const float *__restrict__ mask, unsigned short *__restrict__ d1, int n, long nlines, int w) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned char *core = (unsigned char *)smem;                     // [nl][n]
    const long l0 = (long)blockIdx.x * kMaskLines;
    const int nl = (int)((nlines - l0) < kMaskLines ? (nlines - l0) : kMaskLines);
    if (nl <= 0) return;
    const size_t base = (size_t)l0 * n;
    const int tot = nl * n;
    for (int i = threadIdx.x; i < tot; i += 256) core[i] = mask[base + i] >= 0.5f ? 1 : 0;
    __syncthreads();
    const int w2 = w * w;
    for (int i = threadIdx.x; i < tot; i += 256) {
        const int line = i / n, x = i - line * n;
        const unsigned char *c = core + line * n;
        int best = w2;
        for (int k = 0; k <= w; k++) {
            const bool lo = x - k >= 0 && c[x - k], hi = x + k < n && c[x + k];
            if (lo || hi) { best = k * k < w2 ? k * k : w2; break; }
        }
        d1[base + i] = (unsigned short)best;
    }
}

struct MaskBlendP {
    const float *map, *mask; const float2 *outside;      // outside: the filtered map (real parts), or null: the map itself
    const float *edge;                                   // edge[d^2], d^2 < w^2
    float *out; float weight;
};

// One min-plus step along an axis of stride `sa` (elements), over tiles of kMaskTX x-voxels by kMaskTL voxels of the axis; the third
// coordinate (stride `sb`) is blockIdx.z.  The tile and its halo of w rows on either side are staged in LDS (rows outside the box
// count as "no core": there is no wrap-around), every row is one coalesced run along x.  A thread walks outwards from its row and
// stops as soon as k^2 cannot improve the minimum any more.  din == nullptr (edge width 0): no distances, the blend alone.
template <bool BLEND>
__global__ void __launch_bounds__(256) k_mask_dline(const unsigned short *__restrict__ din, unsigned short *__restrict__ dout, int n, int w,
                                                    size_t sa, size_t sb, MaskBlendP B) {
    __shared__ unsigned short tile[(kMaskTL + 2 * kMaskMaxW) * kMaskTX];
    const int lane = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int x = blockIdx.x * kMaskTX + lane;
    const int a0 = blockIdx.y * kMaskTL;
    const size_t boff = (size_t)blockIdx.z * sb;
    const int w2 = w * w;
    const int rows = kMaskTL + 2 * w;
    if (din) {
        for (int r = r0; r < rows; r += 4) {
            const int a = a0 - w + r;
            unsigned short v = (unsigned short)w2;
            if (a >= 0 && a < n && x < n) v = din[boff + (size_t)a * sa + x];
            tile[r * kMaskTX + lane] = v;
        }
    }
    __syncthreads();
    if (x >= n) return;
    for (int t = r0; t < kMaskTL; t += 4) {
        const int a = a0 + t;
        if (a >= n) break;
        int best = w2;
        if (din) {
            const unsigned short *c = tile + (t + w) * kMaskTX + lane;
            best = c[0];
            for (int k = 1; k <= w && k * k < best; k++) {
                const int lo = c[-k * kMaskTX], hi = c[k * kMaskTX];
                const int m = (lo < hi ? lo : hi) + k * k;
                best = m < best ? m : best;
            }
        }
        const size_t idx = boff + (size_t)a * sa + x;
        if (!BLEND) {
            dout[idx] = (unsigned short)best;
        } else {
            const float m = B.mask[idx], v = B.map[idx];
            float s = fminf(fmaxf(m, 0.f), 1.f);
            if (best < w2) s = fmaxf(s, B.edge[best]);
            const float o = B.outside ? B.outside[idx].x : v;
            B.out[idx] = s * v + (1.f - s) * (B.weight * o);
        }
    }
}

__global__ void k_mask_r2c(const float *__restrict__ map, float2 *__restrict__ f, size_t n3) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) f[i] = make_float2(map[i], 0.f);
}

// f[kz][ky][kx] *= h[kx^2 + ky^2 + kz^2] (signed indices in [-n/2, n/2)); the table ends where the filter has reached zero
__global__ void k_mask_lowpass(float2 *__restrict__ f, const float *__restrict__ h, int nh, int n) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int y = blockIdx.y, z = blockIdx.z;
    const int kx = x < (n + 1) / 2 ? x : x - n, ky = y < (n + 1) / 2 ? y : y - n, kz = z < (n + 1) / 2 ? z : z - n;
    const int k2 = kx * kx + ky * ky + kz * kz;
    const float s = k2 < nh ? h[k2] : 0.f;
    const size_t i = ((size_t)z * n + y) * n + x;
    const float2 v = f[i];
    f[i] = make_float2(v.x * s, v.y * s);
}

}  // namespace ppm
