// ppm_label_kernels.h — largest connected body of a thresholded map (ppm_create_mask) for gfx950 / CDNA4, wave64.
//
//   k_label_threshold   B = sphere ∩ {L >= t} as bit rows (one 64-bit word per 64 x voxels, from __ballot), the number of run heads of
//                       every word, and per block: min / max of L over the sphere and |B|
//   k_label_scan_*      exclusive sum of the head counts in word order: a run's id is the rank of its head in linear voxel order
//   k_label_totals      the block partials of k_label_threshold reduced in block order
//   k_label_init        parent[i] = i, size[i] = 0
//   k_label_union       every run head unites its run with the runs of the four earlier neighbour rows that overlap the run widened by
//                       one voxel on each side: (y-1, z), (y-1, z-1), (y, z-1), (y+1, z-1) - that is 26-connectivity
//   k_label_flatten     parent[i] = root of i, by pointer jumping
//   k_label_sizes       size[root] += voxels of the run, one integer add per distinct root of a wavefront
//   k_label_best        (largest size, smallest id) over the roots by one 64-bit integer atomicMax; number of roots
//   k_label_select      1_C as floats (the output) or as the real parts of the complex work array (the re-bin transform)
//   k_label_expand      bit rows -> floats 0 / 1
//
// The unit of work is the run - a maximal stretch of set voxels along x - not the voxel.  Run ids ascend with the linear index of the
// run's first voxel, so the smallest id of a body is the run that holds the body's smallest linear index.  The union-find is the
// lock-free one: parent[i] <= i always, a root is linked by an integer atomicMin on its own entry, every loop strictly lowers an id and
// no thread waits for another.  What the forest looks like on the way depends on scheduling; the partition it ends with does not, the
// roots are the minima of the bodies, the sizes are integer sums: two calls agree bit for bit.  The launch count is fixed.
#pragma once
#include "ppm_dev.h"

namespace ppm {

typedef unsigned long long u64;

constexpr int kLabelRowsPerBlock = 16;    // k_label_threshold: 4 wavefronts of 4 rows
constexpr int kLabelScanItems = 2048;     // words per block of the scan: 256 threads x 8; 512^3 has 1024 such blocks, one block scans their sums
constexpr unsigned kLabelNone = 0xffffffffu;

// what the host reads back: [0] after the threshold stage, [1] after the re-bin threshold
struct LabelTotals { float mn, mx; u64 above; unsigned runs; unsigned pad; };
// what the labelling leaves for k_label_select and the host
struct LabelBest { u64 key; unsigned components; unsigned pad; };      // key = size << 32 | (0xffffffff - root id)

__device__ __forceinline__ u64 run_heads(u64 word, u64 prev) { return word & ~((word << 1) | (prev >> 63)); }

// src: the map (stride 1) or the real parts of the complex work array (stride 2)
__global__ void __launch_bounds__(256) k_label_threshold(const float *__restrict__ src, int stride, int n, int W, long long r2, float t,
                                                         u64 *__restrict__ bits, unsigned *__restrict__ hcount,
                                                         float *__restrict__ pmin, float *__restrict__ pmax, unsigned *__restrict__ pabove) {
    __shared__ float s_mn[4], s_mx[4];
    __shared__ unsigned s_ab[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long nrows = (long)n * n;
    const int c = n / 2;
    float mn = INFINITY, mx = -INFINITY;
    unsigned above = 0;
    for (int k = 0; k < kLabelRowsPerBlock / 4; k++) {
        const long row = (long)blockIdx.x * kLabelRowsPerBlock + wave * (kLabelRowsPerBlock / 4) + k;      // wave-uniform
        if (row >= nrows) break;
        const int z = (int)(row / n), y = (int)(row - (long)z * n);
        const long long dyz = (long long)(y - c) * (y - c) + (long long)(z - c) * (z - c);
        u64 prev = 0;
        for (int w = 0; w < W; w++) {
            const int x = w * 64 + lane;
            bool set = false;
            if (x < n && dyz + (long long)(x - c) * (x - c) <= r2) {
                const float v = src[((size_t)row * n + x) * stride];
                mn = fminf(mn, v); mx = fmaxf(mx, v);
                set = v >= t;
            }
            const u64 word = __ballot(set);
            if (lane == 0) {
                bits[(size_t)row * W + w] = word;
                hcount[(size_t)row * W + w] = (unsigned)__popcll(run_heads(word, prev));
            }
            above += (unsigned)__popcll(word);
            prev = word;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_ab[wave] = above; }
    __syncthreads();
    if (threadIdx.x == 0) {
        pmin[blockIdx.x] = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
        pmax[blockIdx.x] = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
        pabove[blockIdx.x] = s_ab[0] + s_ab[1] + s_ab[2] + s_ab[3];
    }
}

// one block: the partials of k_label_threshold in block order
__global__ void __launch_bounds__(1024) k_label_totals(const float *__restrict__ pmin, const float *__restrict__ pmax, const unsigned *__restrict__ pabove,
                                                       int np, LabelTotals *__restrict__ out) {
    __shared__ float s_mn[1024], s_mx[1024];
    __shared__ u64 s_ab[1024];
    float mn = INFINITY, mx = -INFINITY;
    u64 ab = 0;
    for (int i = threadIdx.x; i < np; i += 1024) { mn = fminf(mn, pmin[i]); mx = fmaxf(mx, pmax[i]); ab += pabove[i]; }
    s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx; s_ab[threadIdx.x] = ab;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_mn[threadIdx.x] = fminf(s_mn[threadIdx.x], s_mn[threadIdx.x + o]);
            s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + o]);
            s_ab[threadIdx.x] += s_ab[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out->mn = s_mn[0]; out->mx = s_mx[0]; out->above = s_ab[0]; }
}

// ---- exclusive sum of cnt[0 .. nw) in three launches: block sums, one block over the sums, the blocks again with their bases
__global__ void __launch_bounds__(256) k_label_scan_sums(const unsigned *__restrict__ cnt, long nw, unsigned *__restrict__ bsum) {
    __shared__ unsigned s[256];
    const long b0 = (long)blockIdx.x * kLabelScanItems;
    unsigned v = 0;
    for (int j = 0; j < kLabelScanItems / 256; j++) {
        const long i = b0 + j * 256 + threadIdx.x;
        if (i < nw) v += cnt[i];
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = s[0];
}

// nb <= 1024 block sums -> their exclusive sums in place; the total is the number of runs
__global__ void __launch_bounds__(1024) k_label_scan_top(unsigned *__restrict__ bsum, int nb, LabelTotals *__restrict__ out) {
    __shared__ unsigned s[1024];
    const int t = threadIdx.x;
    const unsigned own = t < nb ? bsum[t] : 0;
    s[t] = own;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned add = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    if (t < nb) bsum[t] = s[t] - own;
    if (t == 1023) out->runs = s[1023];
}

__global__ void __launch_bounds__(256) k_label_scan_write(const unsigned *__restrict__ cnt, long nw, const unsigned *__restrict__ bbase,
                                                          unsigned *__restrict__ wordbase) {
    __shared__ unsigned s[256];
    constexpr int per = kLabelScanItems / 256;
    const int t = threadIdx.x;
    const long i0 = (long)blockIdx.x * kLabelScanItems + (long)t * per;
    unsigned c[per], own = 0;
    for (int j = 0; j < per; j++) { c[j] = i0 + j < nw ? cnt[i0 + j] : 0; own += c[j]; }
    s[t] = own;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned add = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    unsigned run = bbase[blockIdx.x] + s[t] - own;
    for (int j = 0; j < per; j++) {
        if (i0 + j < nw) wordbase[i0 + j] = run;
        run += c[j];
    }
}

__global__ void k_label_init(unsigned *__restrict__ parent, unsigned *__restrict__ size, unsigned nruns) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nruns) { parent[i] = i; size[i] = 0; }
}

// ---- union-find
__device__ __forceinline__ unsigned uf_load(const unsigned *parent, unsigned i) {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of i as far as this thread can see it (a stale entry is an earlier ancestor: still a member of i's body); parent[x] < x on
// the way, so the walk ends.  A walk of two steps or more leaves a shortcut behind, by atomicMin: entries only ever fall.
__device__ __forceinline__ unsigned uf_find(unsigned *parent, unsigned i) {
    unsigned p = uf_load(parent, i);
    if (p == i) return i;
    const unsigned first = p;
    for (;;) {
        const unsigned g = uf_load(parent, p);
        if (g == p) break;
        p = g;
    }
    if (p != first) atomicMin(parent + i, p);
    return p;
}

// Links the bodies of a and b.  Each turn either ends or replaces the larger of two roots by a strictly smaller id.
__device__ __forceinline__ void uf_unite(unsigned *parent, unsigned a, unsigned b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const unsigned s = a; a = b; b = s; }
        const unsigned old = atomicMin(parent + a, b);         // a > b
        if (old == a) return;                                  // a was a root and now hangs below b
        a = old;                                               // a had been linked meanwhile (old < a): its former parent and b remain to be united
    }
}

// last voxel of the run that starts at bit hb of word w (cur) of the row rb; bits past the box are never set
__device__ __forceinline__ int run_last(const u64 *__restrict__ rb, int W, int w, int hb, u64 cur) {
    const u64 gap = ~cur >> hb;
    if (gap) return w * 64 + hb + __builtin_ctzll(gap) - 1;
    for (int w2 = w + 1; w2 < W; w2++) {
        const u64 inv = ~rb[w2];
        if (inv) return w2 * 64 + __builtin_ctzll(inv) - 1;
    }
    return W * 64 - 1;
}

// one thread per word; the heads of the word are its runs
__global__ void __launch_bounds__(256) k_label_union(const u64 *__restrict__ bits, const unsigned *__restrict__ wordbase, unsigned *__restrict__ parent,
                                                     unsigned nruns, int n, int W, long nw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw) return;
    const u64 cur = bits[i];
    if (!cur) return;
    const long row = i / W;
    const int w = (int)(i - row * W);
    const int z = (int)(row / n), y = (int)(row - (long)z * n);
    u64 heads = run_heads(cur, w > 0 ? bits[i - 1] : 0);
    unsigned id = wordbase[i];
    const u64 *rb = bits + (size_t)row * W;
    for (; heads; heads &= heads - 1, id++) {
        const int hb = __builtin_ctzll(heads);
        const int first = w * 64 + hb, last = run_last(rb, W, w, hb, cur);
        const int lo = first > 0 ? first - 1 : 0, hi = last + 1 < n ? last + 1 : n - 1;
        for (int q = 0; q < 4; q++) {
            const int ny = y + (q == 3 ? 1 : q == 2 ? 0 : -1), nz = z - (q == 0 ? 0 : 1);
            if (ny < 0 || ny >= n || nz < 0) continue;
            const size_t nrow = (size_t)nz * n + ny;
            const u64 *nb = bits + nrow * W;
            const unsigned *nbase = wordbase + nrow * W;
            for (int wq = lo >> 6; wq <= (hi >> 6); wq++) {
                const u64 full = nb[wq];
                if (!full) continue;
                const u64 before = wq > 0 ? nb[wq - 1] : 0;
                const int a = lo - wq * 64 > 0 ? lo - wq * 64 : 0, b = hi - wq * 64 < 63 ? hi - wq * 64 : 63;
                const u64 window = (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1)) & (~0ull << a);
                const u64 m = full & window;
                // a run that came in from the previous word of the window has been united there
                const u64 carry = wq > (lo >> 6) ? before >> 63 : 0;
                u64 starts = m & ~((m << 1) | carry);
                const u64 nheads = run_heads(full, before);
                for (; starts; starts &= starts - 1) {
                    const int p = __builtin_ctzll(starts);
                    // heads at or below p, minus one: the run that holds p (its head may lie in an earlier word: nbase[wq] - 1)
                    const unsigned nid = nbase[wq] + (unsigned)__popcll(nheads & ((2ull << p) - 1)) - 1u;
                    if (id < nruns && nid < nruns) uf_unite(parent, id, nid);       // always, by the scan; the entries are never indexed unchecked
                }
            }
        }
    }
}

// parent[i] = root.  Only thread i writes parent[i] here, and every value it writes is an ancestor; it publishes its progress so that a
// walk through i jumps: on a chain this is pointer doubling.
__global__ void __launch_bounds__(256) k_label_flatten(unsigned *__restrict__ parent, unsigned nruns) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nruns) return;
    unsigned p = uf_load(parent, i);
    for (;;) {
        const unsigned g = uf_load(parent, p);
        if (g == p) break;
        p = g;
        __hip_atomic_store(parent + i, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// size[root] += length of the run.  The lanes of a wavefront that hold the same root add once.
__global__ void __launch_bounds__(256) k_label_sizes(const u64 *__restrict__ bits, const unsigned *__restrict__ wordbase, const unsigned *__restrict__ parent,
                                                     unsigned *__restrict__ size, unsigned nruns, int W, long nw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 cur = 0, heads = 0;
    unsigned id = 0;
    long row = 0;
    int w = 0;
    if (i < nw) {
        cur = bits[i];
        row = i / W;
        w = (int)(i - row * W);
        if (cur) { heads = run_heads(cur, w > 0 ? bits[i - 1] : 0); id = wordbase[i]; }
    }
    const u64 *rb = bits + (size_t)row * W;
    while (__ballot(heads != 0)) {                                   // wave-uniform
        unsigned root = kLabelNone, len = 0;
        if (heads) {
            const int hb = __builtin_ctzll(heads);
            heads &= heads - 1;
            len = (unsigned)(run_last(rb, W, w, hb, cur) - (w * 64 + hb) + 1);
            root = id < nruns ? parent[id] : kLabelNone;
            id++;
        }
        u64 pend = __ballot(root != kLabelNone);
        while (pend) {                                               // wave-uniform
            const int leader = __builtin_ctzll(pend);
            const unsigned lr = (unsigned)__shfl((int)root, leader);
            const bool mine = root == lr;
            unsigned s = mine ? len : 0;
            for (int o = 32; o > 0; o >>= 1) s += (unsigned)__shfl_xor((int)s, o);
            if (lane == leader) atomicAdd(size + lr, s);
            pend &= ~__ballot(mine);
        }
    }
}

__global__ void __launch_bounds__(256) k_label_best(const unsigned *__restrict__ parent, const unsigned *__restrict__ size, unsigned nruns,
                                                    LabelBest *__restrict__ best) {
    u64 key = 0;
    unsigned roots = 0;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < nruns; i += gridDim.x * 256) {
        if (parent[i] == i) {
            roots++;
            const u64 k = ((u64)size[i] << 32) | (u64)(0xffffffffu - i);
            key = k > key ? k : key;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = (u64)__shfl_xor((long long)key, o);
        key = other > key ? other : key;
        roots += (unsigned)__shfl_xor((int)roots, o);
    }
    if ((threadIdx.x & 63) == 0 && roots) { atomicMax(&best->key, key); atomicAdd(&best->components, roots); }
}

// one wavefront per word; out_c: the complex work array of the re-bin transform, else out_f
__global__ void __launch_bounds__(256) k_label_select(const u64 *__restrict__ bits, const unsigned *__restrict__ wordbase, const unsigned *__restrict__ parent,
                                                      const LabelBest *__restrict__ best, unsigned nruns, int n, int W, long nw, float *__restrict__ out_f,
                                                      float2 *__restrict__ out_c) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nw) return;
    const int lane = threadIdx.x & 63;
    const long row = i / W;
    const int w = (int)(i - row * W);
    const int x = w * 64 + lane;
    if (x >= n) return;
    const u64 cur = bits[i];
    float v = 0.f;
    if ((cur >> lane) & 1) {
        const u64 heads = run_heads(cur, w > 0 ? bits[i - 1] : 0);
        const unsigned id = wordbase[i] + (unsigned)__popcll(heads & ((2ull << lane) - 1)) - 1u;
        const unsigned want = 0xffffffffu - (unsigned)(best->key & 0xffffffffu);
        v = id < nruns && parent[id] == want ? 1.f : 0.f;
    }
    const size_t o = (size_t)row * n + x;
    if (out_c) out_c[o] = make_float2(v, 0.f);
    else out_f[o] = v;
}

__global__ void __launch_bounds__(256) k_label_expand(const u64 *__restrict__ bits, int n, int W, long nw, float *__restrict__ out) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nw) return;
    const int lane = threadIdx.x & 63;
    const long row = i / W;
    const int x = (int)(i - row * W) * 64 + lane;
    if (x < n) out[(size_t)row * n + x] = (float)((bits[i] >> lane) & 1);
}

}  // namespace ppm
