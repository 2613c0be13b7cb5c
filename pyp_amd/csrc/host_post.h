// host_post.h — ppm_postprocess: corrected FSC, resolution, B-factor and the sharpened map of two half maps (the work of PYP's
// external/postprocessing/postprocessing.py).  Included by ppm_lib.hip only, after host_volume.h, host_mask.h and host_label.h.
#pragma once

namespace {

constexpr int kPostMaskEdge = 6;                // cosine edge of the automatic mask (voxels)
constexpr double kPostAutomaskEdgePx = 4.0;     // low-pass edge of the automatic mask's body: prompts.CREATE_MASK_EDGE_PX
constexpr double kPostRebin = 0.5;              // its re-bin value
constexpr double kPostFscCut = 0.143;

// shell(k) = floor(|k| + 1/2) by the integer |k|^2: s^2 - s < k2 <= s^2 + s; kPostNoShell beyond shell n/2
std::vector<unsigned short> post_shell_table(int n) {
    const long top = 3L * (n / 2) * (n / 2);
    std::vector<unsigned short> t((size_t)top + 1);
    long s = 0;
    for (long k2 = 0; k2 <= top; k2++) {
        while (k2 > s * s + s) s++;
        t[k2] = s <= n / 2 ? (unsigned short)s : kPostNoShell;
    }
    return t;
}

double post_fsc(const double *q) { const double d = q[1] * q[2]; return d > 0 ? q[0] / std::sqrt(d) : 0.0; }

struct PostCurves { int s_res = 0; double f_res = 0, resolution = 0, bfactor = 0; int fit_shells = 0; std::vector<float> wtab; };

// everything the host decides from the three sets of shell sums, in float64 (DESIGN.md §2d "Curves" and "Filter")
int post_curves(const ppm_post_cfg *cfg, int n, int s_r, const double *su, const double *sm, const double *sr, double *curves, PostCurves &R) {
    const int ns = n / 2 + 1;
    const double df = 1.0 / (n * cfg->pixel_size);
    double *U = curves, *Mk = curves + ns, *Rd = curves + 2 * ns, *Cc = curves + 3 * ns;
    for (int s = 0; s < ns; s++) {
        U[s] = post_fsc(su + 4 * s); Mk[s] = post_fsc(sm + 4 * s); Rd[s] = post_fsc(sr + 4 * s);
        if (s < s_r + 2) Cc[s] = Mk[s];
        else { const double d = 1.0 - Rd[s]; Cc[s] = d < 1e-6 ? 0.0 : (Mk[s] - Rd[s]) / d; }
    }
    R.s_res = 0; R.f_res = (n / 2) * df;
    for (int s = 1; s < ns; s++) {
        if (Cc[s] < kPostFscCut) {
            R.s_res = s;
            const double up = Cc[s - 1] - Cc[s];
            R.f_res = up > 0 && Cc[s - 1] >= kPostFscCut ? ((s - 1) + (Cc[s - 1] - kPostFscCut) / up) * df : s * df;
            break;
        }
    }
    R.resolution = 1.0 / R.f_res;
    std::vector<double> w(ns);
    for (int s = 0; s < ns; s++) {
        const double c = Cc[s];
        if (cfg->skip_fsc_weighting) w[s] = 1.0;
        else if (cfg->apply_fsc2) w[s] = c > 0 ? c * c : 0.0;
        else w[s] = c > 0 ? std::sqrt(2.0 * c / (1.0 + c)) : 0.0;
    }
    double B = 0.0;
    R.fit_shells = 0;
    if (cfg->bfactor_method == 1) B = cfg->adhoc_bfac;
    else if (cfg->bfactor_method == 2) {
        const double f_lo = 1.0 / cfg->fit_low, f_hi = cfg->fit_high > 0 ? 1.0 / cfg->fit_high : R.f_res;
        std::vector<double> x, y;
        for (int s = 1; s < ns; s++) {
            const double f = s * df, P = sm[4 * s + 3] > 0 ? 0.25 * (sm[4 * s + 1] + sm[4 * s + 2] + 2.0 * sm[4 * s]) / sm[4 * s + 3] : 0.0;
            if (f < f_lo || f > f_hi || !(w[s] > 0) || !(P > 0)) continue;
            x.push_back(f * f); y.push_back(std::log(std::sqrt(P) * w[s]));
        }
        R.fit_shells = (int)x.size();
        if (x.size() < 3) return fail(-22, "postprocess: the automatic B-factor needs at least three shells with a positive FSC weight between its limits, got " + std::to_string(x.size()));
        double xm = 0, ym = 0, sxy = 0, sxx = 0;
        for (size_t i = 0; i < x.size(); i++) { xm += x[i]; ym += y[i]; }
        xm /= x.size(); ym /= x.size();
        for (size_t i = 0; i < x.size(); i++) { sxy += (x[i] - xm) * (y[i] - ym); sxx += (x[i] - xm) * (x[i] - xm); }
        B = 4.0 * sxy / sxx;
    }
    R.bfactor = B;
    const double lp_A = cfg->lowpass_auto ? R.resolution : cfg->lowpass, hp_A = cfg->highpass;
    const double s_lp = lp_A > 0 ? n * cfg->pixel_size / lp_A : 0.0, s_hp = hp_A > 0 ? n * cfg->pixel_size / hp_A : 0.0;
    const double inv = 1.0 / ((double)n * n * n);
    R.wtab.assign(ns, 0.f);
    for (int s = 0; s < ns; s++) {
        const double f = s * df;
        double L = 1.0;
        if (lp_A > 0) {
            if (cfg->gaussian) L *= std::exp(-std::log(2.0) * (s / s_lp) * (s / s_lp));
            else L *= s <= s_lp - 1 ? 1.0 : s >= s_lp + 1 ? 0.0 : 0.5 * (1.0 + std::cos(kPi * (s - (s_lp - 1)) / 2.0));
        }
        if (hp_A > 0) {
            if (cfg->gaussian) L *= 1.0 - std::exp(-std::log(2.0) * (s / s_hp) * (s / s_hp));
            else L *= s <= s_hp - 1 ? 0.0 : s >= s_hp + 1 ? 1.0 : 0.5 * (1.0 - std::cos(kPi * (s - (s_hp - 1)) / 2.0));
        }
        R.wtab[s] = (float)(w[s] * std::exp(-B * f * f / 4.0) * L * inv);
    }
    return 0;
}

}  // namespace

extern "C" int ppm_postprocess(const void *half1, const void *half2, const void *mask, int on_device, int n, const ppm_post_cfg *cfg,
                               void *unmasked_out, void *masked_out, void *mask_out, double *curves, long *shell_count, ppm_post_info *info) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!half1 || !half2 || !cfg || !unmasked_out || !masked_out || !curves) return fail(-22, "null argument");
    if (!box_ok(n)) return fail(-22, "postprocess: the box must be even, 32..512, with prime factors 2, 3, 5, 7, got " + std::to_string(n));
    if (!(cfg->pixel_size > 0)) return fail(-22, "postprocess: the pixel size must be positive");
    if (cfg->skip_fsc_weighting && cfg->apply_fsc2) return fail(-22, "postprocess: skip_fsc_weighting and apply_fsc2 exclude each other");
    if (cfg->mask_mode < 0 || cfg->mask_mode > 2) return fail(-22, "postprocess: mask mode must be 0 (none), 1 (external) or 2 (automatic)");
    if (cfg->mask_mode == 1 && !mask) return fail(-22, "postprocess: the external mask is missing");
    if (cfg->mask_mode != 1 && mask) return fail(-22, "postprocess: a mask was given, but the mask mode is not 1 (external)");
    if (cfg->mask_mode == 2) {
        if (cfg->threshold_method < 0 || cfg->threshold_method > 2) return fail(-22, "postprocess: threshold method must be 0 (intensity), 1 (sigma) or 2 (volume)");
        if (!(cfg->automask_lp >= 0)) return fail(-22, "postprocess: the low-pass of the automatic mask must not be negative (0 = none)");
        if (!std::isfinite(cfg->threshold_value)) return fail(-22, "postprocess: the threshold value must be a finite number");
        if (cfg->threshold_method == 2 && !(cfg->threshold_value > 0 && cfg->threshold_value <= 1)) return fail(-22, "postprocess: the volume fraction must lie in (0, 1]");
    }
    if (cfg->randomize_method < 0 || cfg->randomize_method > 1) return fail(-22, "postprocess: randomise method must be 0 (resolution) or 1 (fsc)");
    if (cfg->randomize_method == 0 && !(cfg->randomize_value > 0)) return fail(-22, "postprocess: the resolution beyond which phases are randomised must be positive");
    if (!std::isfinite(cfg->randomize_value)) return fail(-22, "postprocess: the randomise value must be a finite number");
    if (cfg->bfactor_method < 0 || cfg->bfactor_method > 2) return fail(-22, "postprocess: B-factor method must be 0 (none), 1 (ad hoc) or 2 (automatic)");
    if (cfg->bfactor_method == 1 && !std::isfinite(cfg->adhoc_bfac)) return fail(-22, "postprocess: the ad-hoc B-factor must be a finite number");
    if (cfg->bfactor_method == 2 && (!(cfg->fit_low > 0) || !(cfg->fit_high >= 0) || (cfg->fit_high > 0 && cfg->fit_high > cfg->fit_low)))
        return fail(-22, "postprocess: the limits of the B-factor fit must be low > 0 and 0 <= high <= low (in Angstrom; high 0 = the resolution)");
    if (!cfg->lowpass_auto && !(cfg->lowpass >= 0)) return fail(-22, "postprocess: the low-pass resolution must not be negative (0 = none)");
    if (!std::isfinite(cfg->highpass)) return fail(-22, "postprocess: the high-pass resolution must be a finite number");
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const int ns = n / 2 + 1;
    const size_t n3 = (size_t)n * n * n;
    const int nblocks = n * kPostYSplit;
    const double px = cfg->pixel_size;

    StagedMap s_h1, s_h2, s_mask;
    DevTmp<float> t_mask, t_un, t_ma, t_w, t_a;
    DevTmp<float2> t_zu, t_zr;
    DevTmp<unsigned short> t_shell;
    DevTmp<double> t_partial, t_sums, t_sph;
    DevTmp<unsigned long long> t_count;
    if (int rc = s_h1.in(half1, n3, on_device)) return rc;
    if (int rc = s_h2.in(half2, n3, on_device)) return rc;
    if (int rc = s_mask.in(mask, n3, on_device)) return rc;
    const float *d_h1 = s_h1.p, *d_h2 = s_h2.p, *d_mask = s_mask.p;
    float *d_un = (float *)unmasked_out, *d_ma = (float *)masked_out;
    if (!on_device) {
        HIPCHK(t_un.alloc(n3)); HIPCHK(t_ma.alloc(n3));
        d_un = t_un.p; d_ma = t_ma.p;
    }
    const std::vector<unsigned short> shells = post_shell_table(n);          // outlives the asynchronous upload
    HIPCHK(t_shell.alloc(shells.size()));
    HIPCHK(hipMemcpyAsync(t_shell.p, shells.data(), shells.size() * sizeof(unsigned short), hipMemcpyHostToDevice, st));
    HIPCHK(t_zu.alloc(n3)); HIPCHK(t_zr.alloc(n3));
    HIPCHK(t_partial.alloc((size_t)nblocks * ns * 4)); HIPCHK(t_sums.alloc((size_t)3 * ns * 4)); HIPCHK(t_w.alloc(ns));
    HIPCHK(t_count.alloc(1));

    StageTimer timer;
    const dim3 b256(256), g_vox((unsigned)((n3 + 255) / 256)), g_rows((unsigned)((n + 63) / 64), (unsigned)n, (unsigned)n);
    const size_t shells_lds = (size_t)4 * (ns + 1) * 4 * sizeof(double);
    int transforms = 0;
    auto transform = [&](float2 *zb, bool inverse) -> int { transforms++; return fft3d(zb, n, inverse); };
    auto shell_sums = [&](const float2 *zb, int which) -> int {
        hipLaunchKernelGGL(k_post_shells, dim3((unsigned)n, kPostYSplit), b256, shells_lds, st, zb, t_shell.p, n, ns, t_partial.p);
        hipLaunchKernelGGL(k_post_shell_sum, dim3((unsigned)((ns * 4 + 255) / 256)), b256, 0, st, t_partial.p, nblocks, ns * 4, t_sums.p + (size_t)which * ns * 4);
        HIPCHK(hipGetLastError());
        return 0;
    };

    // ---- the mask
    timer.begin("mask");
    double threshold_used = 0.0;
    long mask_voxels = (long)n3;
    LowPass lowpass;
    RankPasses rank;
    if (cfg->mask_mode == 2) {
        HIPCHK(t_mask.alloc(n3));
        HIPCHK(t_a.alloc(n3));
        hipLaunchKernelGGL(k_post_mean, g_vox, b256, 0, st, d_h1, d_h2, t_a.p, n3);
        HIPCHK(hipGetLastError());
        const bool lp = cfg->automask_lp > 0;
        const double r_c = lp ? n * px / cfg->automask_lp : 0.0, edge = lp ? std::min(kPostAutomaskEdgePx, 2.0 * r_c) : 0.0;
        const double orad = 0.5 * n * px, rr = (orad / px) * (orad / px);      // the sphere of ppm_create_mask, by its own expression
        const long long r2 = (long long)std::floor(rr);
        double t = cfg->threshold_value;
        if (cfg->threshold_method != 0) {
            // the low-passed map as ppm_create_mask will see it: the same LowPass of the same (n, r_c, edge)
            if (int rc = real_to_complex(t_a.p, t_zr.p, n3)) return rc;
            if (lp) {
                if (int rc = lowpass.init(n, r_c, edge)) return rc;
                if (int rc = lowpass.apply(t_zr.p)) return rc;
                transforms += 2;
            }
            if (cfg->threshold_method == 1) {
                HIPCHK(t_sph.alloc((size_t)kPostSumBlocks * 3 + 3));
                hipLaunchKernelGGL(k_post_sphere_sums, dim3(kPostSumBlocks), b256, 0, st, t_zr.p, n, r2, t_sph.p);
                hipLaunchKernelGGL(k_post_sphere_total, dim3(1), dim3(64), 0, st, t_sph.p, kPostSumBlocks, t_sph.p + (size_t)kPostSumBlocks * 3);
                HIPCHK(hipGetLastError());
                double tot[3];
                HIPCHK(hipMemcpyAsync(tot, t_sph.p + (size_t)kPostSumBlocks * 3, sizeof(tot), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                const double mean = tot[0] / tot[2], var = std::max(0.0, tot[1] / tot[2] - mean * mean);
                t = mean + cfg->threshold_value * std::sqrt(var);
            } else {
                // the ceil(f n_sphere)-th largest value, 16 bits of its integer image at a time
                unsigned key = 0;
                if (int rc = rank.alloc()) return rc;
                const int rc = rank.run(65536, true, [&](const unsigned *h, int bins) { return rank_of_fraction(cfg->threshold_value, rank_total(h, bins)); },
                                        [&](int pass, unsigned prefix, unsigned *d_hist) {
                                            hipLaunchKernelGGL(k_post_key_hist, g_vox, b256, 0, st, t_zr.p, n, r2, pass, prefix, d_hist);
                                        }, &key);
                if (rc < 0) return rc;                  // the count is a share of the very histogram walked: it is always found
                t = rank_signed_key_value(key);
            }
        }
        threshold_used = t;
        ppm_create_mask_cfg cm = {px, orad, t, lp ? cfg->automask_lp : 0.0, edge, kPostRebin};
        ppm_create_mask_info ci;
        transforms += lp ? 4 : 0;
        if (int rc = ppm_create_mask(t_a.p, 1, n, &cm, t_a.p, &ci)) return rc;
        mask_voxels = ci.mask_voxels;
        // the soft edge: §2b step 1 on a map of ones
        hipLaunchKernelGGL(k_post_fill, g_vox, b256, 0, st, t_mask.p, 1.f, n3);
        HIPCHK(hipGetLastError());
        ppm_mask_cfg mc = {px, kPostMaskEdge, 0.0, 0, 0.0, 0.0};
        if (int rc = ppm_mask_volume(t_mask.p, t_a.p, 1, n, &mc, t_mask.p)) return rc;
        d_mask = t_mask.p;
    } else if (d_mask) {
        HIPCHK(hipMemsetAsync(t_count.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_post_count, dim3(kPostSumBlocks), b256, 0, st, d_mask, n3, t_count.p);
        HIPCHK(hipGetLastError());
        unsigned long long c = 0;
        HIPCHK(hipMemcpyAsync(&c, t_count.p, sizeof(c), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        mask_voxels = (long)c;
    }
    timer.end();
    // ---- transform 1: the unmasked pair; its shell sums decide s_r
    timer.begin("unmasked sums");
    hipLaunchKernelGGL(k_post_pack, g_vox, b256, 0, st, d_h1, d_h2, (const float *)nullptr, t_zu.p, n3);
    HIPCHK(hipGetLastError());
    if (int rc = transform(t_zu.p, false)) return rc;
    if (int rc = shell_sums(t_zu.p, 0)) return rc;
    std::vector<double> sums((size_t)3 * ns * 4);
    HIPCHK(hipMemcpyAsync(sums.data(), t_sums.p, (size_t)ns * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int s_r = ns - 1;
    if (cfg->randomize_method == 0) {
        const double v = std::floor(n * px / cfg->randomize_value + 0.5);
        s_r = v > ns - 1 ? ns - 1 : (int)v;
    } else {
        for (int s = 1; s < ns; s++) if (post_fsc(&sums[4 * s]) < cfg->randomize_value) { s_r = s; break; }
    }
    s_r = std::max(1, std::min(s_r, ns - 1));
    timer.end();
    // ---- transforms 2 and 3: randomised phases, back, mask, forward
    timer.begin("randomised sums");
    hipLaunchKernelGGL(k_post_randomise, g_rows, dim3(64), 0, st, t_zu.p, t_zr.p, t_shell.p, n, s_r, (unsigned)cfg->seed * 0x9E3779B9u);
    HIPCHK(hipGetLastError());
    if (int rc = transform(t_zr.p, true)) return rc;
    hipLaunchKernelGGL(k_post_scale_mask, g_vox, b256, 0, st, t_zr.p, d_mask, (float)(1.0 / ((double)n * n * n)), n3);
    HIPCHK(hipGetLastError());
    if (int rc = transform(t_zr.p, false)) return rc;
    if (int rc = shell_sums(t_zr.p, 2)) return rc;
    timer.end();
    // ---- transform 4: the masked pair
    timer.begin("masked sums");
    hipLaunchKernelGGL(k_post_pack, g_vox, b256, 0, st, d_h1, d_h2, d_mask, t_zr.p, n3);
    HIPCHK(hipGetLastError());
    if (int rc = transform(t_zr.p, false)) return rc;
    if (int rc = shell_sums(t_zr.p, 1)) return rc;
    HIPCHK(hipMemcpyAsync(sums.data(), t_sums.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    timer.end();
    // ---- curves, resolution, B and the filter table on the host
    timer.begin("filter");
    PostCurves R;
    if (int rc = post_curves(cfg, n, s_r, &sums[0], &sums[(size_t)ns * 4], &sums[(size_t)2 * ns * 4], curves, R)) return rc;
    if (shell_count) for (int s = 0; s < ns; s++) shell_count[s] = (long)sums[4 * s + 3];
    // ---- transform 5: the filtered pair back; outputs
    HIPCHK(hipMemcpyAsync(t_w.p, R.wtab.data(), ns * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_post_weight, g_rows, dim3(64), 0, st, t_zu.p, t_shell.p, t_w.p, n);
    HIPCHK(hipGetLastError());
    if (int rc = transform(t_zu.p, true)) return rc;
    timer.end();
    timer.begin("outputs");
    hipLaunchKernelGGL(k_post_out, g_rows, dim3(64), 0, st, t_zu.p, d_mask, d_un, d_ma, n, cfg->flip_x ? 1 : 0, cfg->flip_y ? 1 : 0, cfg->flip_z ? 1 : 0);
    HIPCHK(hipGetLastError());
    timer.end();
    if (int rc = copy_out(unmasked_out, d_un, n3, on_device)) return rc;
    if (int rc = copy_out(masked_out, d_ma, n3, on_device)) return rc;
    if (mask_out) {
        if (d_mask) { if (int rc = copy_out(mask_out, d_mask, n3, on_device)) return rc; }
        else if (on_device) { hipLaunchKernelGGL(k_post_fill, g_vox, b256, 0, st, (float *)mask_out, 1.f, n3); HIPCHK(hipGetLastError()); }
        else std::fill((float *)mask_out, (float *)mask_out + n3, 1.f);
    }
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
        info->s_r = s_r; info->res_shell = R.s_res; info->fit_shells = R.fit_shells; info->transforms = transforms;
        info->resolution = R.resolution; info->bfactor = R.bfactor; info->threshold = threshold_used; info->mask_voxels = mask_voxels;
    }
    timer.report("ppm_postprocess", "box " + std::to_string(n) + ", " + std::to_string(transforms) + " transforms");
    return 0;
}
