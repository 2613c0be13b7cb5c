// ppm_overlap.h — when ppm_refine_batch runs the hit stage of chunk i (one-wave k_local blocks, a second stream) beside the grid search of
// chunk i + 1 (k_global, a resident grid of one block per CU): one rule, used by the host only.  Plain C++, no HIP types: compiled alone
// by tests/test_overlap_plan_cpu.py.
//
// A k_global block owns most of a CU (its W tables take 128 KB of the LDS, its waves two thirds of the registers) but leaves the
// CU's vector memory path nearly idle; the hit stage is bound by exactly that path and by latency.  What the resident block leaves free —
// registers per SIMD, LDS per CU — decides how many hit-stage blocks ("tenants") a CU takes beside it.  The figures are the kernels'
// own (the runtime's function attributes plus the dynamic LDS of the launch), not constants of one build.
#pragma once

#ifndef PPM_HD
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif
#endif

namespace ppm {

struct OverlapKernel {
    int vgprs;          // registers per lane
    int threads;        // per block
    long lds_bytes;     // static + dynamic, per block
};
struct OverlapDevice {
    int vgprs_per_simd;     // register file of one SIMD, per lane (gfx950: 512)
    int simds_per_cu;       // 4
    long lds_per_cu;        // bytes (gfx950: 160 KB)
    int vgpr_granule;       // registers are handed out in multiples of this (gfx950: 8)
    long lds_granule;       // ... and LDS in multiples of this many bytes
};

PPM_HD inline long overlap_round_up(long v, long g) { return g > 1 ? (v + g - 1) / g * g : v; }

// Blocks of `tenant` that fit on a CU beside ONE block of `host`; 0: none (or the host block itself does not fit)
PPM_HD inline int overlap_tenants(const OverlapKernel &host, const OverlapKernel &tenant, const OverlapDevice &dev) {
    if (host.threads <= 0 || tenant.threads <= 0 || host.vgprs <= 0 || tenant.vgprs <= 0 || dev.simds_per_cu <= 0) return 0;
    const long hv = overlap_round_up(host.vgprs, dev.vgpr_granule), tv = overlap_round_up(tenant.vgprs, dev.vgpr_granule);
    const long hl = overlap_round_up(host.lds_bytes, dev.lds_granule), tl = overlap_round_up(tenant.lds_bytes, dev.lds_granule);
    // waves are spread evenly over the SIMDs: the fullest SIMD carries ceil(waves / SIMDs) of them
    const long hw = ((host.threads + 63) / 64 + dev.simds_per_cu - 1) / dev.simds_per_cu;
    const long tw = (tenant.threads + 63) / 64;
    const long free_v = dev.vgprs_per_simd - hw * hv, free_l = dev.lds_per_cu - hl;
    if (free_v < 0 || free_l < 0) return 0;
    const long waves = (free_v / tv) * dev.simds_per_cu;       // tenant waves the CU's free registers hold
    long by_regs = waves / tw;
    // a block of several waves needs them on one CU but may spread them over its SIMDs: nothing more to check than the wave count
    const long by_lds = tl > 0 ? free_l / tl : by_regs;
    const long n = by_regs < by_lds ? by_regs : by_lds;
    return n > 1024 ? 1024 : (int)n;
}

// What a call looks like to the rule
struct OverlapCall {
    bool global_search;     // the call searches the grid ...
    bool use_fft;           // ... with k_gfft (full-window transform) instead of k_global
    int ntiles, nsections;  // tiles of the shift window, sections of the orientation grid
    int nchunks;            // chunks of the call
    bool hit_stage;         // the hits are refined (Tb > 0)
    bool forced_off;        // PPM_REFINE_OVERLAP=0
};

// The overlap is used when a hit-stage block fits beside a k_global block and the call is a plain k_global search (one tile, one
// section) of at least two chunks; every other call keeps the serial order on one stream
PPM_HD inline bool overlap_on(int tenants, const OverlapCall &c) {
    return !c.forced_off && tenants >= 1 && c.global_search && !c.use_fft && c.ntiles == 1 && c.nsections == 1 && c.hit_stage && c.nchunks >= 2;
}

}  // namespace ppm
