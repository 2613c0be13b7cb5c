// host_locres.h — ppm_local_resolution: local resolution of two half maps (the work of ResMap --noguiSplit in PYP's Post-processing
// block).  Included by ppm_lib.hip only, after host_post.h.
#pragma once

namespace {

constexpr double kLrMinStep = 0.25;             // Angstrom
constexpr double kLrMinLevelPx = 2.5;           // lambda_min >= 2.5 pixels: band centre plus two widths inside Nyquist
constexpr double kLrTableCut = 104.0;           // exp(-x) / n^3 is below half the smallest float32 from here on: the entry is 0

// the level grid of DESIGN.md §2e in float64, ascending; what was adjusted goes into notes
int locres_levels(const ppm_locres_cfg *cfg, int n, std::vector<double> &lv, std::string &notes) {
    const double a = cfg->pixel_size;
    if (!(a > 0) || !std::isfinite(a)) return fail(-22, "local_resolution: the pixel size must be positive");
    if (!(cfg->p_value > 0 && cfg->p_value < 1)) return fail(-22, "local_resolution: the p-value must lie strictly between 0 and 1");
    if (!(cfg->step >= kLrMinStep) || !std::isfinite(cfg->step)) return fail(-22, "local_resolution: the resolution step must be at least 0.25 A");
    if (!(cfg->min_res >= 0) || !std::isfinite(cfg->min_res) || !(cfg->max_res >= 0) || !std::isfinite(cfg->max_res))
        return fail(-22, "local_resolution: the minimum and maximum resolution must not be negative (0 = the default)");
    char buf[160];
    double lo = cfg->min_res, hi = cfg->max_res;
    if (lo < kLrMinLevelPx * a) {
        snprintf(buf, sizeof(buf), "minimum resolution %g A raised to %g A (2.5 pixels); ", lo, kLrMinLevelPx * a);
        notes += buf;
        lo = kLrMinLevelPx * a;
    }
    if (hi == 0) {
        hi = n * a / 6.0;
        snprintf(buf, sizeof(buf), "maximum resolution set to %g A (box / 6); ", hi);
        notes += buf;
    } else if (hi > n * a / 4.0) {
        snprintf(buf, sizeof(buf), "local_resolution: the maximum resolution %g A is above a quarter of the box (%g A)", hi, n * a / 4.0);
        return fail(-22, buf);
    }
    lv.clear();
    for (int i = 0; ; i++) {
        const double l = lo + i * cfg->step;
        if (!(l <= hi)) break;
        if (i >= PPM_LOCRES_MAX_LEVELS) return fail(-22, "local_resolution: more than 64 resolution levels; raise the step or narrow the range");
        lv.push_back(l);
    }
    if (lv.empty()) {
        snprintf(buf, sizeof(buf), "local_resolution: no resolution level between %g A and %g A", lo, hi);
        return fail(-22, buf);
    }
    return 0;
}

// band and window of one level over the integer |k|^2, 1 / n^3 folded in, float64 rounded once to float32
void locres_tables(int n, double a, double lambda, float *band, float *window) {
    const long top = 3L * (n / 2) * (n / 2);
    const double inv = 1.0 / ((double)n * n * n);
    const double s = n * a / lambda, l = lambda / a;
    const double sb = std::max(s / 8.0, 1.5), sw = std::max(l, 2.0) / 2.0;
    const double cw = 2.0 * kPi * kPi * sw * sw / ((double)n * n);
    for (long k2 = 0; k2 <= top; k2++) {
        const double d = std::sqrt((double)k2) - s, xb = (d * d) / (2.0 * sb * sb), xw = cw * (double)k2;
        band[k2] = xb > kLrTableCut ? 0.f : (float)(std::exp(-xb) * inv);
        window[k2] = xw > kLrTableCut ? 0.f : (float)(std::exp(-xw) * inv);
    }
    band[0] = 0.f;
}

}  // namespace

extern "C" int ppm_local_resolution(const ppm_locres_cfg *cfg, const void *half1, const void *half2, const void *mask, int on_device, int n,
                                    void *out_res, void *level_maps, ppm_locres_info *info) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!cfg || !half1 || !half2 || !out_res) return fail(-22, "null argument");
    if (!box_ok(n)) return fail(-22, "local_resolution: the box must be even, 32..512, with prime factors 2, 3, 5, 7, got " + std::to_string(n));
    std::vector<double> lv;
    std::string notes;
    if (int rc = locres_levels(cfg, n, lv, notes)) return rc;
    const int L = (int)lv.size();
    if (cfg->keep_levels < 0 || (cfg->keep_levels > 0 && (!level_maps || cfg->keep_levels < L)))
        return fail(-22, "local_resolution: keep_levels must be 0 or at least the number of levels (" + std::to_string(L) + "), with room for them in level_maps");
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const size_t n3 = (size_t)n * n * n, quads = n3 / 4, pairs = n3 / 2;
    const size_t tab = (size_t)3 * (n / 2) * (n / 2) + 1;

    // working memory, owned by the call: two complex arrays, the map, the byte map, the tables, the histogram and the counters
    StagedMap s_h1, s_h2, s_mask;
    DevTmp<float> t_res, t_tab;
    DevTmp<float2> t_z, t_w;
    DevTmp<unsigned char> t_state;
    DevTmp<unsigned long long> t_count;
    RankPasses rank_passes;
    // the kernels read 16 bytes at a time: host arrays, and device arrays that do not start on such a boundary, go through a copy
    if (int rc = s_h1.in(half1, n3, on_device, true)) return rc;
    if (int rc = s_h2.in(half2, n3, on_device, true)) return rc;
    if (int rc = s_mask.in(mask, n3, on_device, true)) return rc;
    const float *d_h1 = s_h1.p, *d_h2 = s_h2.p, *d_mask = s_mask.p;
    HIPCHK(t_z.alloc(n3)); HIPCHK(t_w.alloc(n3)); HIPCHK(t_res.alloc(n3)); HIPCHK(t_state.alloc(n3));
    HIPCHK(t_tab.alloc((size_t)2 * L * tab));
    if (int rc = rank_passes.alloc()) return rc;
    HIPCHK(t_count.alloc((size_t)L + 1));
    if (int rc = raise_lds_limit((const void *)k_lr_key_hist0, kLrHist0Bins * (int)sizeof(unsigned))) return rc;

    StageTimer timer;
    const auto wall0 = std::chrono::steady_clock::now();

    const dim3 b256(256), g_quads((unsigned)((quads + 255) / 256)), g_pairs((unsigned)((pairs + 255) / 256));
    const dim3 g_loop((unsigned)std::min<size_t>(kLrBlocks, (quads + 255) / 256)), g_hist0((unsigned)std::min<size_t>(kLrHist0Blocks, (quads + 1023) / 1024));
    // k_lr_band, k_lr_window: a thread per pair of x, a block per (ky, kz) with both <= N/2
    const int half = n / 2, row_threads = half <= 64 ? 64 : half <= 128 ? 128 : 256;
    const dim3 b_rows((unsigned)row_threads), g_rows((unsigned)((half + row_threads - 1) / row_threads), (unsigned)(half + 1), (unsigned)(half + 1));
    int transforms = 0;
    auto transform = [&](float2 *zb, bool inverse) -> int { transforms++; return fft3d(zb, n, inverse); };

    timer.begin("init + pack");
    HIPCHK(hipMemsetAsync(t_count.p, 0, ((size_t)L + 1) * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_lr_init, g_loop, b256, 0, st, d_mask, t_state.p, t_res.p, n, PPM_LOCRES_UNASSIGNED, t_count.p);
    hipLaunchKernelGGL(k_lr_pack, g_quads, b256, 0, st, d_h1, d_h2, t_z.p, quads);
    HIPCHK(hipGetLastError());
    timer.end();
    timer.begin("forward transform");
    if (int rc = transform(t_z.p, false)) return rc;
    timer.end();
    // the tables of every level, made while the device transforms
    std::vector<float> tables((size_t)2 * L * tab);
    for (int i = 0; i < L; i++) locres_tables(n, cfg->pixel_size, lv[i], &tables[(size_t)2 * i * tab], &tables[(size_t)(2 * i + 1) * tab]);
    HIPCHK(hipMemcpyAsync(t_tab.p, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice, st));
    unsigned long long n_inside = 0;
    HIPCHK(hipMemcpyAsync(&n_inside, t_count.p, sizeof(n_inside), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_inside == 0) return fail(-22, "local_resolution: no voxel is inside the mask (values above 0.5)");
    const long rank = locres_rank(cfg->p_value, (long)n_inside);

    std::vector<float> tau(L);
    for (int i = L - 1; i >= 0; i--) {                      // from the coarsest level to the finest
        const float *d_band = t_tab.p + (size_t)2 * i * tab, *d_win = d_band + tab;
        timer.begin("band");
        hipLaunchKernelGGL(k_lr_band, g_rows, b_rows, 0, st, t_z.p, t_w.p, d_band, n);
        HIPCHK(hipGetLastError());
        timer.end();
        timer.begin("band back");
        if (int rc = transform(t_w.p, true)) return rc;
        timer.end();
        timer.begin("square");
        hipLaunchKernelGGL(k_lr_square, g_pairs, b256, 0, st, t_w.p, pairs);
        HIPCHK(hipGetLastError());
        timer.end();
        timer.begin("squares forward");
        if (int rc = transform(t_w.p, false)) return rc;
        timer.end();
        timer.begin("window");
        hipLaunchKernelGGL(k_lr_window, g_rows, b_rows, 0, st, t_w.p, d_win, n);
        HIPCHK(hipGetLastError());
        timer.end();
        timer.begin("window back");
        if (int rc = transform(t_w.p, true)) return rc;
        timer.end();
        if (cfg->keep_levels)
            if (int rc = copy_out((float2 *)level_maps + (size_t)i * n3, t_w.p, 2 * n3, on_device)) return rc;
        // tau: the rank-th smallest E_D over the inside voxels, 16 bits of its integer image at a time
        timer.begin("threshold (2 histogram passes)");
        unsigned key = 0;
        const int found = rank_passes.run(kLrHist0Bins, false, [&](const unsigned *, int) { return (long long)rank; },
                                          [&](int pass, unsigned prefix, unsigned *d_hist) {
                                              if (pass == 0) hipLaunchKernelGGL(k_lr_key_hist0, g_hist0, dim3(1024), kLrHist0Bins * sizeof(unsigned), st, t_w.p, t_state.p, quads, d_hist);
                                              else hipLaunchKernelGGL(k_lr_key_hist1, g_loop, b256, 0, st, t_w.p, t_state.p, quads, prefix, d_hist);
                                          }, &key);
        if (found < 0) return found;
        if (found != 0) return fail(-5, "local_resolution: the histogram holds fewer voxels than the mask (a value that is not a number?)");
        timer.end();
        memcpy(&tau[i], &key, sizeof(float));
        timer.begin("assign");
        hipLaunchKernelGGL(k_lr_assign, g_loop, b256, 0, st, t_w.p, t_state.p, t_res.p, quads, tau[i], (float)lv[i], t_count.p + 1 + i);
        HIPCHK(hipGetLastError());
        timer.end();
    }
    std::vector<unsigned long long> alive((size_t)L + 1);
    HIPCHK(hipMemcpyAsync(alive.data(), t_count.p, alive.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (int rc = copy_out(out_res, t_res.p, n3, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_levels = L; info->transforms = transforms; info->n_inside = (long)n_inside;
        info->unassigned = (long)(n_inside - alive[L]);                  // alive[1 + i]: still alive after level i; the coarsest is level L - 1
        long seen = 0;
        const long mid = ((long)n_inside + 1) / 2;
        info->median = PPM_LOCRES_UNASSIGNED;
        for (int i = 0; i < L; i++) {
            info->levels[i] = (float)lv[i]; info->tau[i] = tau[i];
            info->counts[i] = (long)(alive[1 + i] - (i > 0 ? alive[i] : 0ULL));
            if (seen < mid && seen + info->counts[i] >= mid) info->median = info->levels[i];
            seen += info->counts[i];
        }
        snprintf(info->notes, sizeof(info->notes), "%s", notes.c_str());
    }
    if (timer.on) {
        char header[160];
        snprintf(header, sizeof(header), "box %d, %d levels, %d transforms, %.3f ms wall; on the device, summed over the levels", n, L, transforms,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
        timer.report("ppm_local_resolution", header);
    }
    return 0;
}
