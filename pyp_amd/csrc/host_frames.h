// host_frames.h — movie-frame refinement (ppm_frame_refine): per-frame particle shifts from pooled score maps.
#pragma once

namespace {
// the frame list of a call: the usable rows (OCCUPANCY > 0) of the groups in first..last, group by group, ascending FIND inside a group
struct FrameList {
    std::vector<int> goff, frow, fproc, fnew, ffind;     // fproc / fnew: the scoring order inside a group, frames of one model side by side
    std::vector<unsigned char> grefine;             // [group] inside tind_min..tind_max: shifts are written back
    std::vector<float> fm6, fsh;
    long models = 0;
};

// bit-identical pose and CTF parameters: the two frames share one gathered slice, wherever they stand in the group
inline bool frame_same_model(const double *a, const double *b) {
    static const int cols[7] = { PPM_PSI, PPM_THETA, PPM_PHI, PPM_DF1, PPM_DF2, PPM_ANGAST, PPM_PSHIFT };
    for (int c : cols) if (std::memcmp(&a[c], &b[c], sizeof(double)) != 0) return false;
    return true;
}

constexpr int kColFind = 29, kColFshiftX = 30, kColFshiftY = 31;     // FIND, FSHIFT_X, FSHIFT_Y (cistem_star_file.py:596-628)

// rows -> groups.  Refuses a FIND that occurs twice in a group (whatever the rows' occupancy).
static int frame_build_list(const double *rows, int n_rows, const ppm_frame_cfg *fc, double pixel, FrameList &L) {
    std::vector<int> order(n_rows);
    for (int i = 0; i < n_rows; i++) order[i] = i;
    auto key = [&](int i, int c) { return (long)rows[(size_t)i * PPM_NCOL + c]; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (key(x, PPM_PIND) != key(y, PPM_PIND)) return key(x, PPM_PIND) < key(y, PPM_PIND);
        if (key(x, PPM_TIND) != key(y, PPM_TIND)) return key(x, PPM_TIND) < key(y, PPM_TIND);
        return key(x, kColFind) < key(y, kColFind);
    });
    L.goff.assign(1, 0);
    for (int lo = 0; lo < n_rows;) {
        int hi = lo + 1;
        while (hi < n_rows && key(order[hi], PPM_PIND) == key(order[lo], PPM_PIND) && key(order[hi], PPM_TIND) == key(order[lo], PPM_TIND)) hi++;
        for (int q = lo + 1; q < hi; q++)
            if (key(order[q], kColFind) == key(order[q - 1], kColFind))
                return fail(-22, "frame refinement: FIND " + std::to_string(key(order[q], kColFind)) + " occurs twice for particle " + std::to_string(key(order[lo], PPM_PIND)) +
                                 " in tilt " + std::to_string(key(order[lo], PPM_TIND)));
        const long tind = key(order[lo], PPM_TIND);
        if (tind >= fc->first && (fc->last < 0 || tind <= fc->last)) {
            const int g0 = L.goff.back();
            std::vector<int> model;                                     // per frame of the group: the first frame with the same parameters
            for (int q = lo; q < hi; q++) {
                const int j = order[q];
                const double *row = rows + (size_t)j * PPM_NCOL;
                if (!(row[PPM_OCC] > 0)) continue;
                const int f = (int)L.frow.size();
                int m = f;
                for (int e = g0; e < f; e++) if (model[e - g0] == e && frame_same_model(rows + (size_t)L.frow[e] * PPM_NCOL, row)) { m = e; break; }
                model.push_back(m);
                double M[9]; euler_matrix(row[PPM_PSI], row[PPM_THETA], row[PPM_PHI], M);
                L.frow.push_back(j); L.ffind.push_back((int)key(j, kColFind));
                for (int k : { 0, 1, 3, 4, 6, 7 }) L.fm6.push_back((float)M[k]);
                L.fsh.push_back((float)(row[PPM_XSHIFT] / pixel)); L.fsh.push_back((float)(row[PPM_YSHIFT] / pixel));
            }
            const int g1 = (int)L.frow.size();
            for (int e = g0; e < g1; e++) {
                if (model[e - g0] != e) continue;
                L.models++;
                for (int f = e; f < g1; f++) if (model[f - g0] == e) { L.fproc.push_back(f); L.fnew.push_back(f == e); }
            }
            if (g1 > g0) {
                L.goff.push_back((int)L.frow.size());
                L.grefine.push_back(tind >= fc->tind_min && (fc->tind_max < 0 || tind <= fc->tind_max));
            }
        }
        lo = hi;
    }
    return 0;
}
}  // namespace

extern "C" int ppm_frame_plan(const ppm_frame_cfg *fc, float *step_px, int *n_steps, int *clipped) {
    if (!fc) return fail(-22, "null argument");
    if (!(fc->step_px >= 0)) return fail(-22, "frame refinement: step_px must not be negative (0 = half a pixel)");
    if (!(fc->range_px > 0)) return fail(-22, "frame refinement: range_px must be positive");
    if (fc->half_width < 0) return fail(-22, "frame refinement: half_width must not be negative");
    const float h = ppm::frame_step(fc->step_px);
    int clip = 0;
    const int W = ppm::frame_steps(fc->range_px, h, PPM_FRAME_MAX_STEPS, &clip);
    if (step_px) *step_px = h;
    if (n_steps) *n_steps = W;
    if (clipped) *clipped = clip;
    return 0;
}

extern "C" int ppm_frame_refine(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const ppm_frame_cfg *fc, const void *images, int images_on_device,
                                const double *rows, int n_rows, double *rows_out, float *own_maps, float *pooled_maps, ppm_frame_info *info) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!ref || !cfg || !fc || !images || !rows || !rows_out) return fail(-22, "null argument");
    StreamScope ss_(ref->stream, ref->copy);
    float h = 0; int W = 0, clipped = 0;
    if (int rc = ppm_frame_plan(fc, &h, &W, &clipped)) return rc;
    const int side = 2 * W + 1, npts = side * side;
    ppm_frame_info fi; std::memset(&fi, 0, sizeof(fi));
    fi.n_steps = W; fi.step_px = h; fi.range_px = (float)W * h; fi.clipped = clipped;
    ref->note.clear();
    if (clipped) {
        char b[200];
        std::snprintf(b, sizeof(b), "frame refinement: a shift range of %g pixels needs more than %d steps of %g either side; the grid covers +-%g pixels",
                      (double)fc->range_px, PPM_FRAME_MAX_STEPS, (double)h, (double)fi.range_px);
        ref->note = b;
    }
    if (info) *info = fi;
    if (n_rows <= 0) return 0;
    CspRun c; c.ref = ref; c.cfg = cfg; c.n_proj = n_rows;
    const Geom &gm = c.gm;
    ppm_refine_cfg c2 = *cfg; c2.global_search = 0; c2.res_signed_cc = 0;       // all rings signed
    std::string err;
    if (!geom_init(c.gm, c2, err)) return fail(-22, err);
    if (gm.N != ref->N) return fail(-22, "particle box differs from the reference box");
    if (gm.B > (ref->B + 1) / ref->pad - 1) return fail(-22, "high-resolution limit exceeds the band the reference was prepared for");
    FrameList L;
    if (int rc = frame_build_list(rows, n_rows, fc, gm.a, L)) return rc;
    std::memcpy(rows_out, rows, (size_t)n_rows * PPM_NCOL * sizeof(double));
    if (own_maps) std::memset(own_maps, 0, (size_t)n_rows * npts * sizeof(float));
    if (pooled_maps) std::memset(pooled_maps, 0, (size_t)n_rows * npts * sizeof(float));
    const int nf = (int)L.frow.size(), ng = (int)L.goff.size() - 1;
    fi.groups = ng; fi.models = L.models; fi.rows_skipped = n_rows - nf;
    if (info) *info = fi;
    if (nf == 0) return 0;
    const Trace trace_("ppm_frame_refine");
    c.rm_px = cfg->mask_radius / gm.a;
    build_samples(gm, c.sl);
    c.S_pad = (int)c.sl.packed.size(); c.nrings = gm.B + 2;
    // host tables and results: declared ahead of the guard, so that they outlive the drain of an error return
    std::vector<int> ti; std::vector<float> tf, h_own, h_pool, h_score; std::vector<double> gw, h_delta;
    DrainOnError drain;
    drain.armed = true;
    if (int rc = csp_prepare_spectra(c, images, images_on_device, rows, false)) return rc;
    trace_.mark("spectra prepared");
    const int S_used = c.prefix_of(gm.r_hi);
    if (S_used <= 0 || (S_used & 15)) return fail(-22, "frame refinement: the band holds no samples");
    // tables: ints [goff | frow | fproc | fnew | ffind], floats [fm6 | fsh], the pooling weights.  The ensures below are the call's only
    // ones on the frame workspace and come before MP and PP are filled; the spectra were ensured by csp_prepare_spectra.
    const int hw = fc->half_width;
    int span = 0;
    for (int gi = 0; gi < ng; gi++) span = std::max(span, L.ffind[L.goff[gi + 1] - 1] - L.ffind[L.goff[gi]]);
    const int n_gw = std::min(hw, span) + 1;
    gw.assign(n_gw, 1.0);
    for (int d = 1; d < n_gw; d++) gw[d] = std::exp(-((double)d * d) / (2.0 * (0.5 * hw) * (0.5 * hw)));
    ti.reserve(ng + 1 + 4 * (size_t)nf);
    ti.insert(ti.end(), L.goff.begin(), L.goff.end()); ti.insert(ti.end(), L.frow.begin(), L.frow.end());
    ti.insert(ti.end(), L.fproc.begin(), L.fproc.end()); ti.insert(ti.end(), L.fnew.begin(), L.fnew.end()); ti.insert(ti.end(), L.ffind.begin(), L.ffind.end());
    tf.reserve(8 * (size_t)nf);
    tf.insert(tf.end(), L.fm6.begin(), L.fm6.end()); tf.insert(tf.end(), L.fsh.begin(), L.fsh.end());
    const bool in_lds = frame_store_in_lds(S_used);
    if (int rc = ref->frames.ints.ensure(ti.size() + (size_t)nf)) return rc;            // + amax
    if (int rc = ref->frames.flts.ensure(tf.size() + 2 * (size_t)nf)) return rc;        // + score
    if (int rc = ref->frames.dbls.ensure((size_t)n_gw + 2 * (size_t)nf)) return rc;     // + delta
    if (int rc = ref->frames.own.ensure((size_t)nf * npts)) return rc;
    if (int rc = ref->frames.pool.ensure((size_t)nf * npts)) return rc;
    if (!in_lds) if (int rc = ref->frames.store.ensure((size_t)ng * S_used)) return rc;
    HIPCHK(hipMemcpyAsync(ref->frames.ints.p, ti.data(), ti.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->frames.flts.p, tf.data(), tf.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->frames.dbls.p, gw.data(), gw.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    FrameMapP MP;
    MP.cv = cube_view(ref); MP.samples = ref->samples.p; MP.Il = ref->spectra.Il.p; MP.cw = ref->spectra.cw.p; MP.S_pad = c.S_pad; MP.N = gm.N; MP.S_used = S_used;
    MP.rlo2 = (float)(gm.r_lo * gm.r_lo); MP.rmax2 = (float)(gm.r_hi * gm.r_hi); MP.W = W; MP.h = h;
    MP.goff = ref->frames.ints.p; MP.frow = MP.goff + (ng + 1); MP.fproc = MP.frow + nf; MP.fnew = MP.fproc + nf;
    const int *d_ffind = MP.fnew + nf; int *d_amax = ref->frames.ints.p + ti.size();
    MP.fm6 = ref->frames.flts.p; MP.fsh = MP.fm6 + 6 * (size_t)nf;
    float *d_score = ref->frames.flts.p + tf.size();
    MP.scratch = in_lds ? nullptr : ref->frames.store.p; MP.own = ref->frames.own.p;
    FramePeakP PP;
    PP.W = W; PP.h = h; PP.half_width = hw; PP.goff = MP.goff; PP.ffind = d_ffind; PP.gw = ref->frames.dbls.p; PP.n_gw = n_gw;
    PP.own = ref->frames.own.p; PP.pooled = ref->frames.pool.p; PP.amax = d_amax; PP.delta = ref->frames.dbls.p + n_gw; PP.score = d_score;
    {
        ProfScope ps(PPM_K_LOCAL);
        hipLaunchKernelGGL(k_frame_maps, dim3((unsigned)ng), dim3(kFrameThreads), frame_lds_bytes(S_used), cur_stream(), MP);
        hipLaunchKernelGGL(k_frame_peak, dim3((unsigned)ng), dim3(64), (size_t)npts * sizeof(double), cur_stream(), PP);
    }
    HIPCHK(hipGetLastError());
    h_score.resize(2 * (size_t)nf); h_delta.resize(2 * (size_t)nf);
    if (own_maps) { h_own.resize((size_t)nf * npts); HIPCHK(hipMemcpyAsync(h_own.data(), ref->frames.own.p, h_own.size() * sizeof(float), hipMemcpyDeviceToHost, cur_stream())); }
    if (pooled_maps) { h_pool.resize((size_t)nf * npts); HIPCHK(hipMemcpyAsync(h_pool.data(), ref->frames.pool.p, h_pool.size() * sizeof(float), hipMemcpyDeviceToHost, cur_stream())); }
    HIPCHK(hipMemcpyAsync(h_score.data(), d_score, h_score.size() * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(h_delta.data(), PP.delta, h_delta.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    trace_.mark("maps and peaks");
    for (int gi = 0; gi < ng; gi++)
        for (int f = L.goff[gi]; f < L.goff[gi + 1]; f++) {
            const int j = L.frow[f];
            double *row = rows_out + (size_t)j * PPM_NCOL;
            if (own_maps) std::memcpy(own_maps + (size_t)j * npts, &h_own[(size_t)f * npts], (size_t)npts * sizeof(float));
            if (pooled_maps) std::memcpy(pooled_maps + (size_t)j * npts, &h_pool[(size_t)f * npts], (size_t)npts * sizeof(float));
            if (L.grefine[gi]) {
                const double dx = h_delta[2 * (size_t)f] * gm.a, dy = h_delta[2 * (size_t)f + 1] * gm.a;
                row[PPM_XSHIFT] += dx; row[PPM_YSHIFT] += dy; row[kColFshiftX] += dx; row[kColFshiftY] += dy;
                row[PPM_SCORE] = 100.0 * (double)h_score[2 * (size_t)f];
                fi.rows_refined++;
            } else {
                row[PPM_SCORE] = 100.0 * (double)h_score[2 * (size_t)f + 1];
                fi.rows_scored++;
            }
        }
    if (info) *info = fi;
    ref->last_counts[0] = npts; ref->last_counts[1] = 1; ref->last_counts[2] = (long)std::floor(kPi * gm.r_hi * gm.r_hi / 2);
    ref->last_counts[3] = (long)((double)L.models * S_used / std::max(n_rows, 1));
    return drain.ok();
}
