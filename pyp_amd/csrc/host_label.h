// host_label.h — ppm_create_mask: binary mask of a map's largest body (the work of frealignx/create_mask).
// Included by ppm_lib.hip only, after host_volume.h.
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

    StagedMap s_map;
    DevTmp<float> t_pmin, t_pmax;
    DevTmp<float2> t_f;
    DevTmp<u64> t_bits;
    DevTmp<unsigned> t_cnt, t_base, t_bsum, t_pabove, t_parent, t_size;
    DevTmp<LabelTotals> t_tot;
    DevTmp<LabelBest> t_best;
    if (int rc = s_map.in(map, n3, on_device)) return rc;
    const float *d_map = s_map.p;
    float *d_out = on_device ? (float *)mask_out : s_map.copy.p;     // the map has been read in full before the mask is written
    LowPass lowpass;
    if (lp) {
        if (int rc = lowpass.init(n, n * cfg->pixel_size / cfg->lowpass_A, cfg->lowpass_edge_px)) return rc;
        HIPCHK(t_f.alloc(n3));
    }
    HIPCHK(t_bits.alloc((size_t)nw)); HIPCHK(t_cnt.alloc((size_t)nw)); HIPCHK(t_base.alloc((size_t)nw)); HIPCHK(t_bsum.alloc((size_t)nb));
    HIPCHK(t_pmin.alloc((size_t)np)); HIPCHK(t_pmax.alloc((size_t)np)); HIPCHK(t_pabove.alloc((size_t)np));
    HIPCHK(t_tot.alloc(2)); HIPCHK(t_best.alloc(1));
    HIPCHK(hipMemsetAsync(t_tot.p, 0, 2 * sizeof(LabelTotals), st));
    HIPCHK(hipMemsetAsync(t_best.p, 0, sizeof(LabelBest), st));

    StageTimer timer;
    const dim3 b256(256), g_words((unsigned)((nw + 255) / 256)), g_wavewords((unsigned)((nw + 3) / 4));
    auto threshold = [&](const float *src, int stride, float t, LabelTotals *tot) {
        hipLaunchKernelGGL(k_label_threshold, dim3((unsigned)np), b256, 0, st, src, stride, n, W, r2, t, t_bits.p, t_cnt.p, t_pmin.p, t_pmax.p, t_pabove.p);
        hipLaunchKernelGGL(k_label_totals, dim3(1), dim3(1024), 0, st, t_pmin.p, t_pmax.p, t_pabove.p, np, tot);
    };

    // ---- low-pass
    timer.begin("low-pass");
    if (lp) {
        if (int rc = real_to_complex(d_map, t_f.p, n3)) return rc;
        if (int rc = lowpass.apply(t_f.p)) return rc;
    }
    timer.end();
    // ---- threshold: bit rows, density range, run ids
    timer.begin("threshold");
    threshold(lp ? (const float *)t_f.p : d_map, lp ? 2 : 1, t32, t_tot.p);
    hipLaunchKernelGGL(k_label_scan_sums, dim3((unsigned)nb), b256, 0, st, t_cnt.p, nw, t_bsum.p);
    hipLaunchKernelGGL(k_label_scan_top, dim3(1), dim3(1024), 0, st, t_bsum.p, nb, t_tot.p);
    hipLaunchKernelGGL(k_label_scan_write, dim3((unsigned)nb), b256, 0, st, t_cnt.p, nw, t_bsum.p, t_base.p);
    HIPCHK(hipGetLastError());
    timer.end();
    LabelTotals tot[2];
    memset(tot, 0, sizeof(tot));
    HIPCHK(hipMemcpyAsync(&tot[0], t_tot.p, sizeof(LabelTotals), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (tot[0].above == 0) {
        char msg[256];
        snprintf(msg, sizeof(msg), "create_mask: no voxel inside the outer radius reaches the threshold %g: the density there ranges from %g to %g",
                 (double)t32, (double)tot[0].mn, (double)tot[0].mx);
        return fail(-22, msg);
    }
    // ---- labelling: the number of launches does not depend on the map; the two arrays have one entry per run
    const unsigned nruns = tot[0].runs;
    HIPCHK(t_parent.alloc(nruns)); HIPCHK(t_size.alloc(nruns));
    const dim3 g_runs((nruns + 255) / 256);
    timer.begin("labelling");
    hipLaunchKernelGGL(k_label_init, g_runs, b256, 0, st, t_parent.p, t_size.p, nruns);
    hipLaunchKernelGGL(k_label_union, g_words, b256, 0, st, t_bits.p, t_base.p, t_parent.p, nruns, n, W, nw);
    hipLaunchKernelGGL(k_label_flatten, g_runs, b256, 0, st, t_parent.p, nruns);
    hipLaunchKernelGGL(k_label_sizes, g_words, b256, 0, st, t_bits.p, t_base.p, t_parent.p, t_size.p, nruns, W, nw);
    hipLaunchKernelGGL(k_label_best, dim3(std::min(g_runs.x, 2048u)), b256, 0, st, t_parent.p, t_size.p, nruns, t_best.p);
    hipLaunchKernelGGL(k_label_select, g_wavewords, b256, 0, st, t_bits.p, t_base.p, t_parent.p, t_best.p, nruns, n, W, nw, lp ? (float *)nullptr : d_out,
                       lp ? t_f.p : (float2 *)nullptr);
    HIPCHK(hipGetLastError());
    timer.end();
    // ---- re-bin: the same low-pass on 1_C, thresholded inside the sphere; no second labelling
    timer.begin("re-bin");
    if (lp) {
        if (int rc = lowpass.apply(t_f.p)) return rc;
        threshold((const float *)t_f.p, 2, b32, t_tot.p + 1);
        hipLaunchKernelGGL(k_label_expand, g_wavewords, b256, 0, st, t_bits.p, n, W, nw, d_out);
        HIPCHK(hipGetLastError());
    }
    timer.end();
    LabelBest best;
    HIPCHK(hipMemcpyAsync(&best, t_best.p, sizeof(best), hipMemcpyDeviceToHost, st));
    if (lp) HIPCHK(hipMemcpyAsync(&tot[1], t_tot.p + 1, sizeof(LabelTotals), hipMemcpyDeviceToHost, st));
    if (int rc = copy_out(mask_out, d_out, n3, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
        info->density_min = tot[0].mn; info->density_max = tot[0].mx;
        info->above = (long)tot[0].above; info->components = (long)best.components; info->largest = (long)(best.key >> 32);
        info->mask_voxels = lp ? (long)tot[1].above : info->largest;
    }
    timer.report("ppm_create_mask", "box " + std::to_string(n) + ", " + std::to_string(nruns) + " runs");
    return 0;
}
