// host_mask.h — ppm_mask_volume: shape masking of a reference map (the work of frealign_v9.11's apply_mask.exe).
// Included by ppm_lib.hip only.
#pragma once

namespace {

// edge[d^2] = (1 + cos(pi d / w)) / 2 for the integer squared distances below w^2: float64 here, rounded once
std::vector<float> mask_edge_table(int w) {
    std::vector<float> t((size_t)w * w);
    for (int d2 = 0; d2 < w * w; d2++) t[d2] = (float)(0.5 * (1.0 + std::cos(kPi * std::sqrt((double)d2) / w)));
    return t;
}

// H(|k|) / n^3 by the integer |k|^2, up to the first radius at which the filter is zero for good
std::vector<float> mask_lowpass_table(int n, double r_c, double e) {
    const double r_end = r_c + 0.5 * e, r_one = r_c - 0.5 * e;
    const long k2_box = 3L * (n / 2) * (n / 2);
    const long nh = std::min(k2_box, (long)std::floor(r_end * r_end) + 1) + 1;
    const double inv = 1.0 / ((double)n * n * n);
    std::vector<float> t((size_t)nh);
    for (long k2 = 0; k2 < nh; k2++) {
        const double r = std::sqrt((double)k2);
        double h;
        if (r <= r_one) h = 1.0;
        else if (r >= r_end) h = 0.0;
        else h = 0.5 * (1.0 + std::cos(kPi * (r - r_one) / e));
        t[k2] = (float)(h * inv);
    }
    return t;
}

}  // namespace

extern "C" int ppm_mask_volume(const void *map, const void *mask, int on_device, int n, const ppm_mask_cfg *cfg, void *out) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!map || !mask || !cfg || !out) return fail(-22, "null argument");
    if (n < 8 || n > 512) return fail(-22, "mask_volume: box must be 8..512, got " + std::to_string(n));
    if (!(cfg->pixel_size > 0)) return fail(-22, "mask_volume: the pixel size must be positive");
    if (cfg->edge_width < 0 || cfg->edge_width > kMaskMaxW) return fail(-22, "mask_volume: the width of the cosine edge must be 0..64 pixels, got " + std::to_string(cfg->edge_width));
    if (cfg->filter != 0 && cfg->filter != 2) return fail(-22, "mask_volume: outside filter " + std::to_string(cfg->filter) + " is not supported by this build (0 = none, 2 = cosine edge)");
    if (cfg->filter == 2) {
        if (!box_ok(n)) return fail(-22, "mask_volume: the outside filter needs an even box, 32..512, with prime factors 2, 3, 5, 7");
        if (!(cfg->filter_radius_A > 0)) return fail(-22, "mask_volume: the filter radius must be positive");
        if (!(cfg->filter_edge_px >= 0)) return fail(-22, "mask_volume: the width of the filter edge must not be negative");
    }
    HIPCHK(hipSetDevice(g.device));
    const int w = cfg->edge_width;
    const size_t n3 = (size_t)n * n * n;
    const float weight = (float)cfg->outside_weight;
    // with weight 0 the outside density drops out of the blend: no transforms (what PYP sends by default: filter 2, weight 0.0)
    const bool filtered = cfg->filter == 2 && weight != 0.f;
    hipStream_t st = cur_stream();

    DevTmp<float> t_map, t_mask, t_edge, t_h;
    DevTmp<unsigned short> t_d1, t_d2;
    DevTmp<float2> t_f;
    const float *d_map = (const float *)map, *d_mask = (const float *)mask;
    float *d_out = (float *)out;
    if (!on_device) {
        HIPCHK(t_map.alloc(n3));
        HIPCHK(t_mask.alloc(n3));
        HIPCHK(hipMemcpyAsync(t_map.p, map, n3 * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t_mask.p, mask, n3 * sizeof(float), hipMemcpyHostToDevice, st));
        d_map = t_map.p; d_mask = t_mask.p; d_out = t_map.p;        // every voxel of the blend reads and writes its own index only
    }
    // temporaries and tables first, so that the launches below follow each other without a host allocation in between
    std::vector<float> edge, h;                                      // outlive the asynchronous uploads
    if (w > 0) {
        edge = mask_edge_table(w);
        HIPCHK(t_edge.alloc(edge.size()));
        HIPCHK(t_d1.alloc(n3));
        HIPCHK(t_d2.alloc(n3));
    }
    if (filtered) {
        h = mask_lowpass_table(n, n * cfg->pixel_size / cfg->filter_radius_A, cfg->filter_edge_px);
        HIPCHK(t_h.alloc(h.size()));
        HIPCHK(t_f.alloc(n3));
    }
    // PPM_TRACE: device time of the call between the uploads and the download, by two events on the call's stream
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (getenv("PPM_TRACE")) { ev0 = ev_get(); ev1 = ev_get(); (void)hipEventRecord(ev0, st); }
    const unsigned nt = (unsigned)((n + kMaskTX - 1) / kMaskTX), na = (unsigned)((n + kMaskTL - 1) / kMaskTL);
    MaskBlendP B; B.map = nullptr; B.mask = nullptr; B.outside = nullptr; B.edge = nullptr; B.out = nullptr; B.weight = 0.f;
    if (w > 0) {
        HIPCHK(hipMemcpyAsync(t_edge.p, edge.data(), edge.size() * sizeof(float), hipMemcpyHostToDevice, st));
        const long nlines = (long)n * n;
        hipLaunchKernelGGL(k_mask_dx, dim3((unsigned)((nlines + kMaskLines - 1) / kMaskLines)), dim3(256), (size_t)kMaskLines * n, st,
                           d_mask, t_d1.p, n, nlines, w);
        hipLaunchKernelGGL(k_mask_dline<false>, dim3(nt, na, (unsigned)n), dim3(256), 0, st, t_d1.p, t_d2.p, n, w, (size_t)n, (size_t)n * n, B);
        HIPCHK(hipGetLastError());
    }
    if (filtered) {
        HIPCHK(hipMemcpyAsync(t_h.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mask_r2c, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, d_map, t_f.p, n3);
        HIPCHK(hipGetLastError());
        if (int rc = fft3d(t_f.p, n, false)) return rc;
        hipLaunchKernelGGL(k_mask_lowpass, dim3((unsigned)((n + 63) / 64), (unsigned)n, (unsigned)n), dim3(64), 0, st, t_f.p, t_h.p, (int)h.size(), n);
        HIPCHK(hipGetLastError());
        if (int rc = fft3d(t_f.p, n, true)) return rc;
    }
    B.map = d_map; B.mask = d_mask; B.outside = filtered ? t_f.p : nullptr; B.edge = t_edge.p; B.out = d_out; B.weight = weight;
    hipLaunchKernelGGL(k_mask_dline<true>, dim3(nt, na, (unsigned)n), dim3(256), 0, st, w > 0 ? t_d2.p : nullptr, (unsigned short *)nullptr, n, w,
                       (size_t)n * n, (size_t)n, B);
    HIPCHK(hipGetLastError());
    if (ev1) (void)hipEventRecord(ev1, st);
    if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, n3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ev1) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        fprintf(stderr, "ppm_mask_volume: box %d, edge %d, filter %s: %.3f ms on the device\n", n, w, filtered ? "2" : "none", ms);
        std::lock_guard<std::mutex> lk(g_mu);
        g.pool.push_back(ev0); g.pool.push_back(ev1);
    }
    return 0;
}
