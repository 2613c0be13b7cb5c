// host_label.h — ppm_create_mask: binary mask of a map's largest body (the work of frealignx/create_mask).
// Included by ppm_lib.hip only, after host_mask.h (mask_lowpass_table).
#pragma once

extern "C" int ppm_create_mask(const void *map, int on_device, int n, const ppm_create_mask_cfg *cfg, void *mask_out, ppm_create_mask_info *info) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!map || !cfg || !mask_out) return fail(-22, "null argument");
    if (n < 8 || n > 512) return fail(-22, "create_mask: box must be 8..512, got " + std::to_string(n));
    if (!(cfg->pixel_size > 0)) return fail(-22, "create_mask: the pixel size must be positive");
    if (!(cfg->outer_radius_A > 0)) return fail(-22, "create_mask: the outer radius must be positive");
    if (!(cfg->lowpass_A >= 0)) return fail(-22, "create_mask: the low-pass resolution must not be negative (0 = no low-pass)");
    if (!(cfg->lowpass_edge_px >= 0)) return fail(-22, "create_mask: the width of the low-pass edge must not be negative");
    if (!std::isfinite(cfg->threshold)) return fail(-22, "create_mask: the threshold must be a finite number");
    const bool lp = cfg->lowpass_A != 0;
    if (lp) {
        if (!box_ok(n)) return fail(-22, "create_mask: the low-pass needs an even box, 32..512, with prime factors 2, 3, 5, 7 (resolution 0 = none)");
        if (!(cfg->rebin > 0 && cfg->rebin < 1)) return fail(-22, "create_mask: the re-bin value must lie strictly between 0 and 1");
    }
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const int W = (n + 63) / 64;
    const long nrows = (long)n * n, nw = nrows * W;
    const size_t n3 = (size_t)n * n * n;
    const int np = (int)((nrows + kLabelRowsPerBlock - 1) / kLabelRowsPerBlock);
    const int nb = (int)((nw + kLabelScanItems - 1) / kLabelScanItems);           // 1024 at 512^3: one block scans the block sums
    const double rr = (cfg->outer_radius_A / cfg->pixel_size) * (cfg->outer_radius_A / cfg->pixel_size);
    const long long r2 = rr >= 3.0 * 512 * 512 ? 3LL * 512 * 512 : (long long)std::floor(rr);       // integer left side: <= rr is <= floor(rr)
    const float t32 = (float)cfg->threshold, b32 = (float)cfg->rebin;

    DevTmp<float> t_map, t_h, t_pmin, t_pmax;
    DevTmp<float2> t_f;
    DevTmp<u64> t_bits;
    DevTmp<unsigned> t_cnt, t_base, t_bsum, t_pabove, t_parent, t_size;
    DevTmp<LabelTotals> t_tot;
    DevTmp<LabelBest> t_best;
    const float *d_map = (const float *)map;
    float *d_out = (float *)mask_out;
    if (!on_device) {
        HIPCHK(t_map.alloc(n3));
        HIPCHK(hipMemcpyAsync(t_map.p, map, n3 * sizeof(float), hipMemcpyHostToDevice, st));
        d_map = t_map.p; d_out = t_map.p;            // the map has been read in full before the mask is written
    }
    std::vector<float> h;                            // outlives the asynchronous upload
    if (lp) {
        h = mask_lowpass_table(n, n * cfg->pixel_size / cfg->lowpass_A, cfg->lowpass_edge_px);
        HIPCHK(t_h.alloc(h.size()));
        HIPCHK(t_f.alloc(n3));
    }
    HIPCHK(t_bits.alloc((size_t)nw)); HIPCHK(t_cnt.alloc((size_t)nw)); HIPCHK(t_base.alloc((size_t)nw)); HIPCHK(t_bsum.alloc((size_t)nb));
    HIPCHK(t_pmin.alloc((size_t)np)); HIPCHK(t_pmax.alloc((size_t)np)); HIPCHK(t_pabove.alloc((size_t)np));
    HIPCHK(t_tot.alloc(2)); HIPCHK(t_best.alloc(1));
    HIPCHK(hipMemsetAsync(t_tot.p, 0, 2 * sizeof(LabelTotals), st));
    HIPCHK(hipMemsetAsync(t_best.p, 0, sizeof(LabelBest), st));

    // PPM_TRACE: device time per stage, by events on the call's stream
    const bool trace = getenv("PPM_TRACE") != nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (trace) for (auto &e : ev) e = ev_get();
    auto mark = [&](int k) { if (trace) (void)hipEventRecord(ev[k], st); };
    auto release = [&]() {
        if (!trace) return;
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto e : ev) g.pool.push_back(e);
    };
    const dim3 b256(256), g_lowpass((unsigned)((n + 63) / 64), (unsigned)n, (unsigned)n), g_words((unsigned)((nw + 255) / 256)),
        g_wavewords((unsigned)((nw + 3) / 4));
    auto band_limit = [&]() -> int {
        if (int rc = fft3d(t_f.p, n, false)) return rc;
        hipLaunchKernelGGL(k_mask_lowpass, g_lowpass, dim3(64), 0, st, t_f.p, t_h.p, (int)h.size(), n);
        if (hipGetLastError() != hipSuccess) return fail(-5, "create_mask: k_mask_lowpass did not launch");
        return fft3d(t_f.p, n, true);
    };
    auto threshold = [&](const float *src, int stride, float t, LabelTotals *tot) {
        hipLaunchKernelGGL(k_label_threshold, dim3((unsigned)np), b256, 0, st, src, stride, n, W, r2, t, t_bits.p, t_cnt.p, t_pmin.p, t_pmax.p, t_pabove.p);
        hipLaunchKernelGGL(k_label_totals, dim3(1), dim3(1024), 0, st, t_pmin.p, t_pmax.p, t_pabove.p, np, tot);
    };

    mark(0);
    // ---- low-pass
    if (lp) {
        HIPCHK(hipMemcpyAsync(t_h.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mask_r2c, dim3((unsigned)((n3 + 255) / 256)), b256, 0, st, d_map, t_f.p, n3);
        HIPCHK(hipGetLastError());
        if (int rc = band_limit()) { release(); return rc; }
    }
    mark(1);
    // ---- threshold: bit rows, density range, run ids
    threshold(lp ? (const float *)t_f.p : d_map, lp ? 2 : 1, t32, t_tot.p);
    hipLaunchKernelGGL(k_label_scan_sums, dim3((unsigned)nb), b256, 0, st, t_cnt.p, nw, t_bsum.p);
    hipLaunchKernelGGL(k_label_scan_top, dim3(1), dim3(1024), 0, st, t_bsum.p, nb, t_tot.p);
    hipLaunchKernelGGL(k_label_scan_write, dim3((unsigned)nb), b256, 0, st, t_cnt.p, nw, t_bsum.p, t_base.p);
    HIPCHK(hipGetLastError());
    mark(2);
    LabelTotals tot[2];
    memset(tot, 0, sizeof(tot));
    HIPCHK(hipMemcpyAsync(&tot[0], t_tot.p, sizeof(LabelTotals), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (tot[0].above == 0) {
        release();
        char msg[256];
        snprintf(msg, sizeof(msg), "create_mask: no voxel inside the outer radius reaches the threshold %g: the density there ranges from %g to %g",
                 (double)t32, (double)tot[0].mn, (double)tot[0].mx);
        return fail(-22, msg);
    }
    // ---- labelling: the number of launches does not depend on the map; the two arrays have one entry per run
    const unsigned nruns = tot[0].runs;
    HIPCHK(t_parent.alloc(nruns)); HIPCHK(t_size.alloc(nruns));
    const dim3 g_runs((nruns + 255) / 256);
    hipLaunchKernelGGL(k_label_init, g_runs, b256, 0, st, t_parent.p, t_size.p, nruns);
    hipLaunchKernelGGL(k_label_union, g_words, b256, 0, st, t_bits.p, t_base.p, t_parent.p, nruns, n, W, nw);
    hipLaunchKernelGGL(k_label_flatten, g_runs, b256, 0, st, t_parent.p, nruns);
    hipLaunchKernelGGL(k_label_sizes, g_words, b256, 0, st, t_bits.p, t_base.p, t_parent.p, t_size.p, nruns, W, nw);
    hipLaunchKernelGGL(k_label_best, dim3(std::min(g_runs.x, 2048u)), b256, 0, st, t_parent.p, t_size.p, nruns, t_best.p);
    hipLaunchKernelGGL(k_label_select, g_wavewords, b256, 0, st, t_bits.p, t_base.p, t_parent.p, t_best.p, nruns, n, W, nw, lp ? (float *)nullptr : d_out,
                       lp ? t_f.p : (float2 *)nullptr);
    HIPCHK(hipGetLastError());
    mark(3);
    // ---- re-bin: the same low-pass on 1_C, thresholded inside the sphere; no second labelling
    if (lp) {
        if (int rc = band_limit()) { release(); return rc; }
        threshold((const float *)t_f.p, 2, b32, t_tot.p + 1);
        hipLaunchKernelGGL(k_label_expand, g_wavewords, b256, 0, st, t_bits.p, n, W, nw, d_out);
        HIPCHK(hipGetLastError());
    }
    mark(4);
    LabelBest best;
    HIPCHK(hipMemcpyAsync(&best, t_best.p, sizeof(best), hipMemcpyDeviceToHost, st));
    if (lp) HIPCHK(hipMemcpyAsync(&tot[1], t_tot.p + 1, sizeof(LabelTotals), hipMemcpyDeviceToHost, st));
    if (!on_device) HIPCHK(hipMemcpyAsync(mask_out, d_out, n3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
        info->density_min = tot[0].mn; info->density_max = tot[0].mx;
        info->above = (long)tot[0].above; info->components = (long)best.components; info->largest = (long)(best.key >> 32);
        info->mask_voxels = lp ? (long)tot[1].above : info->largest;
    }
    if (trace) {
        float ms[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4; k++) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        fprintf(stderr, "ppm_create_mask: box %d, %u runs: low-pass %.3f ms, threshold %.3f ms, labelling %.3f ms, re-bin %.3f ms on the device\n", n, nruns,
                ms[0], ms[1], ms[2], ms[3]);
        release();
    }
    return 0;
}
