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

    StagedMap s_map, s_mask;
    DevTmp<float> t_edge;
    DevTmp<unsigned short> t_d1, t_d2;
    DevTmp<float2> t_f;
    if (int rc = s_map.in(map, n3, on_device)) return rc;
    if (int rc = s_mask.in(mask, n3, on_device)) return rc;
    const float *d_map = s_map.p, *d_mask = s_mask.p;
    float *d_out = on_device ? (float *)out : s_map.copy.p;          // every voxel of the blend reads and writes its own index only
    // temporaries and tables first, so that the launches below follow each other without a host allocation in between
    std::vector<float> edge;                                         // outlives the asynchronous upload
    LowPass lowpass;
    if (w > 0) {
        edge = mask_edge_table(w);
        HIPCHK(t_edge.alloc(edge.size()));
        HIPCHK(t_d1.alloc(n3));
        HIPCHK(t_d2.alloc(n3));
    }
    if (filtered) {
        if (int rc = lowpass.init(n, n * cfg->pixel_size / cfg->filter_radius_A, cfg->filter_edge_px)) return rc;
        HIPCHK(t_f.alloc(n3));
    }
    StageTimer timer;
    timer.begin("on the device");
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
        if (int rc = real_to_complex(d_map, t_f.p, n3)) return rc;
        if (int rc = lowpass.apply(t_f.p)) return rc;
    }
    B.map = d_map; B.mask = d_mask; B.outside = filtered ? t_f.p : nullptr; B.edge = t_edge.p; B.out = d_out; B.weight = weight;
    hipLaunchKernelGGL(k_mask_dline<true>, dim3(nt, na, (unsigned)n), dim3(256), 0, st, w > 0 ? t_d2.p : nullptr, (unsigned short *)nullptr, n, w,
                       (size_t)n * n, (size_t)n, B);
    HIPCHK(hipGetLastError());
    timer.end();
    if (int rc = copy_out(out, d_out, n3, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    char header[96];
    snprintf(header, sizeof(header), "box %d, edge %d, filter %s", n, w, filtered ? "2" : "none");
    timer.report("ppm_mask_volume", header);
    return 0;
}
