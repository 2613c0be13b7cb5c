// host_ctf.h — the ppm_ctf handle, ppm_ctf_spectrum_plan / ppm_ctf_spectrum (the averaged periodogram of a micrograph or a movie, pinned
// to the reference's own periodogram_averaging) and ppm_ctf_fit_plan / ppm_ctf_fit / ppm_ctf_estimate (defocus and astigmatism from
// spectra): the work of cistem2's ctffind, DESIGN.md §2g.  Included by ppm_lib.hip only.

// Workspaces of both stages, owned by the handle and sized by the plans (ppm_ctf_plan.h) before the first launch.
struct ppm_ctf {
    hipStream_t stream = nullptr, copy = nullptr;
    DevBuf<float> img, part, power;      // a host image staged, the chunks' partial sums, the result of the last call
    DevBuf<float2> half;                 // row-transformed tiles of one trip
    // the fit: host spectra staged; the sample list (geometry; positions, rings, window steps, grid winners); conditioned samples, their sums
    // of squares and the winners' scores; windows and refined parameters; the grid's scores
    DevBuf<float> spectra, v, scores, diag; DevBuf<float4> geo; DevBuf<int> pos; DevBuf<double> lo, prof;     // prof, diag: k_ctf_profile's outputs
};

namespace {

void ctf_plan_info(const CtfSpectrumPlan &p, ppm_ctf_spectrum_info *o) {
    o->tile = p.tile; o->half_w = p.half_w; o->tiles_x = p.tiles_x; o->tiles_y = p.tiles_y; o->groups = p.groups; o->vec = p.vec;
    o->tiles = p.tiles; o->chunks = p.chunks; o->pass_tiles = p.pass_tiles;
    o->half_bytes = p.half_floats2 * 8; o->part_bytes = p.part_floats * 4; o->out_floats = p.out_floats;
}

}  // namespace

extern "C" ppm_ctf_t *ppm_ctf_create(void) {
    if (!g.inited) { fail(-1, "ppm_init has not been called"); return nullptr; }
    struct Undo { ppm_ctf *p; ~Undo() { ppm_ctf_destroy(p); } } guard{ new ppm_ctf() };
    HIPCHKP(hipSetDevice(g.device));
    HIPCHKP(hipStreamCreateWithFlags(&guard.p->stream, hipStreamNonBlocking));
    HIPCHKP(hipStreamCreateWithFlags(&guard.p->copy, hipStreamNonBlocking));
    ppm_ctf *h = guard.p;
    guard.p = nullptr;
    return h;
}

extern "C" void ppm_ctf_destroy(ppm_ctf_t *h) {
    if (!h) return;
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->copy) (void)hipStreamDestroy(h->copy);
    delete h;
}

// host only: no device is touched (and none is needed)
extern "C" int ppm_ctf_spectrum_plan(int nx, int ny, int nframes, int group, int tile, ppm_ctf_spectrum_info *out) {
    if (!out) return fail(-22, "null argument");
    std::memset(out, 0, sizeof(*out));
    const CtfSpectrumPlan p = ctf_spectrum_plan(nx, ny, nframes, group, tile);
    if (!p.ok) {
        std::string msg = std::string("ctf spectrum: ") + p.why + " (image " + std::to_string(nx) + " x " + std::to_string(ny) + ", " + std::to_string(nframes) +
                          " frame(s) averaged by " + std::to_string(group) + ", tile " + std::to_string(tile) + ")";
        if (!ctf_tile_ok(tile)) msg += ": " + resample_sizes_hint(tile);
        return fail(-22, msg);
    }
    ctf_plan_info(p, out);
    return 0;
}

extern "C" int ppm_ctf_spectrum(ppm_ctf_t *h, const void *img, int on_device, int nx, int ny, int nframes, int group, int tile, int normalise,
                                void *out_power, int out_on_device) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!h || !img) return fail(-22, "null argument");
    ppm_ctf_spectrum_info info;
    if (int rc = ppm_ctf_spectrum_plan(nx, ny, nframes, group, tile, &info)) return rc;
    const CtfSpectrumPlan p = ctf_spectrum_plan(nx, ny, nframes, group, tile);
    StreamScope ss_(h->stream, h->copy);
    hipStream_t st = cur_stream();
    // every workspace before the first launch; a buffer that cannot be had refuses the call, nothing is shrunk to fit
    const size_t npix = (size_t)nx * ny * nframes;
    if (!on_device) if (int rc = h->img.ensure(npix)) return rc;
    if (int rc = h->half.ensure((size_t)p.half_floats2)) return rc;
    if (int rc = h->part.ensure((size_t)p.part_floats)) return rc;
    if (int rc = h->power.ensure((size_t)p.out_floats)) return rc;
    if (int rc = ensure_plan(tile)) return rc;
    const float *d_img = (const float *)img;
    if (!on_device) { HIPCHK(hipMemcpyAsync(h->img.p, img, npix * sizeof(float), hipMemcpyHostToDevice, st)); d_img = h->img.p; }

    CtfTilesP P;
    P.img = d_img; P.half = h->half.p; P.part = h->part.p; P.plan = g.plans[tile].plan; P.T = tile; P.W = p.half_w;
    P.nx = nx; P.ny = ny; P.nframes = nframes; P.group = group; P.tiles_x = p.tiles_x; P.tiles_y = p.tiles_y;
    P.vec = p.vec && aligned16(d_img);
    const unsigned row_blocks = (unsigned)((tile + kCtfRowsPerBlock - 1) / kCtfRowsPerBlock);
    const int C = ctf_cols_per_block(tile);
    const unsigned col_blocks = (unsigned)((p.half_w + C - 1) / C);
    for (long t0 = 0; t0 < p.tiles; t0 += p.pass_tiles) {
        P.tile0 = t0; P.ntiles = std::min(p.pass_tiles, p.tiles - t0);
        const unsigned nchunk = (unsigned)((P.ntiles + kCtfChunkTiles - 1) / kCtfChunkTiles);
        hipLaunchKernelGGL(k_ctf_tile_rows, dim3(row_blocks, (unsigned)P.ntiles), dim3(256), (size_t)ctf_rows_lds(tile), st, P);
        hipLaunchKernelGGL(k_ctf_tile_cols, dim3(col_blocks, nchunk), dim3(256), (size_t)ctf_cols_lds(tile), st, P, (int)(t0 / kCtfChunkTiles));
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ctf_fold, dim3((unsigned)((p.out_floats + 255) / 256)), dim3(256), 0, st, h->part.p, h->power.p, p.out_floats, p.chunks, (float)p.tiles);
    if (normalise) hipLaunchKernelGGL(k_ctf_normalise, dim3(1), dim3(1024), 0, st, h->power.p, p.out_floats);
    HIPCHK(hipGetLastError());
    if (out_power) HIPCHK(hipMemcpyAsync(out_power, h->power.p, (size_t)p.out_floats * sizeof(float), out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" const void *ppm_ctf_last_power(ppm_ctf_t *h) { return h ? h->power.p : nullptr; }

// host only: no device is touched (and none is needed)
extern "C" int ppm_ctf_fit_plan(int tile, const ppm_ctf_cfg *cfg, ppm_ctf_fit_info *out) {
    if (!cfg || !out) return fail(-22, "null argument");
    std::memset(out, 0, sizeof(*out));
    const CtfFitPlan p = ctf_fit_plan(tile, cfg->pixel, cfg->min_res, cfg->max_res, cfg->step, cfg->tol);
    if (!p.ok) return fail(-22, std::string("ctf fit: ") + p.why);
    if (!(cfg->kv > 0) || !(cfg->cs >= 0) || !(cfg->wgh >= 0) || !(cfg->wgh < 1)) return fail(-22, "ctf fit: voltage, spherical aberration and amplitude contrast (0 .. 1) are out of range");
    const long ni = ctf_window_steps(cfg->min_def, cfg->max_def, cfg->step);
    if (!ni) return fail(-22, "ctf fit: the defocus range must be positive, minimum <= maximum, at most 100000 steps");
    out->tile = tile; out->B = p.B; out->a = p.a; out->k2lo = p.k2lo; out->k2hi = p.k2hi; out->bg_w = p.bg_w; out->nj = p.nj; out->nc = p.nc;
    out->ni = ni; out->candidates = ni * p.nc;
    // the fitted samples, counted as they will be listed
    long ns = 0;
    for (int ky = -p.B / 2; ky < p.B / 2; ky++)
        for (int kx = 0; kx <= p.B / 2; kx++) { const int k2 = kx * kx + ky * ky; if (k2 >= p.k2lo && k2 <= p.k2hi && !(kx == 0 && ky < 0)) ns++; }
    out->samples = ns;
    return 0;
}

extern "C" int ppm_ctf_fit(ppm_ctf_t *h, const void *spectra, int on_device, int n, int tile, const ppm_ctf_cfg *cfg, const double *def_lo,
                           const double *def_hi, double *out_rows, float *grid_scores, long grid_ld, double *avrot, float *diag) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!h || !spectra || !cfg || !out_rows) return fail(-22, "null argument");
    if (n < 1 || n > 65535) return fail(-22, "ctf fit: 1 .. 65535 spectra per call, got " + std::to_string(n));
    if ((def_lo == nullptr) != (def_hi == nullptr)) return fail(-22, "ctf fit: per-spectrum windows need both ends");
    ppm_ctf_fit_info info;
    if (int rc = ppm_ctf_fit_plan(tile, cfg, &info)) return rc;
    const CtfFitPlan p = ctf_fit_plan(tile, cfg->pixel, cfg->min_res, cfg->max_res, cfg->step, cfg->tol);
    // ---- the windows: shared when all are the same
    std::vector<double> lo((size_t)n, cfg->min_def); std::vector<int> ni((size_t)n, (int)info.ni);
    bool shared = true; long ni_max = info.ni;
    if (def_lo) {
        ni_max = 0;
        for (int s = 0; s < n; s++) {
            const long k = ctf_window_steps(def_lo[s], def_hi[s], cfg->step);
            if (!k) return fail(-22, "ctf fit: the defocus window of spectrum " + std::to_string(s) + " must be positive, minimum <= maximum, at most 100000 steps");
            lo[s] = def_lo[s]; ni[s] = (int)k; ni_max = std::max(ni_max, k);
            shared = shared && def_lo[s] == def_lo[0] && k == ni[0];
        }
    }
    const long ncand_max = ni_max * p.nc;
    if (grid_scores && grid_ld < ncand_max) return fail(-22, "ctf fit: the grid scores need " + std::to_string(ncand_max) + " floats per spectrum");
    // ---- the sample list, scan order (ky = -B/2 .. B/2 - 1, kx = 0 .. B/2)
    const int B = p.B, W = tile / 2 + 1, ns = (int)info.samples;
    if (ns < 2) return fail(-22, "ctf fit: fewer than two samples lie between the two resolutions");
    std::vector<float4> geo; std::vector<int> pos, ring;
    geo.reserve(ns); pos.reserve(ns); ring.reserve(ns);
    for (int ky = -B / 2; ky < B / 2; ky++)
        for (int kx = 0; kx <= B / 2; kx++) {
            const int k2 = kx * kx + ky * ky;
            if (k2 < p.k2lo || k2 > p.k2hi || (kx == 0 && ky < 0)) continue;
            const double d = (double)B * p.a;
            geo.push_back(make_float4((float)(k2 / (d * d)), (float)((double)(kx * kx - ky * ky) / k2), (float)(2.0 * kx * ky / k2), 0.f));
            pos.push_back((ky < 0 ? ky + tile : ky) * W + kx);
            ring.push_back((int)std::floor(std::sqrt((double)k2) + 0.5));
        }
    StreamScope ss_(h->stream, h->copy);
    hipStream_t st = cur_stream();
    // ---- every workspace before the first launch
    const size_t per = (size_t)tile * W;
    if (!on_device) if (int rc = h->spectra.ensure((size_t)n * per)) return rc;
    if (int rc = h->geo.ensure((size_t)ns)) return rc;
    if (int rc = h->pos.ensure((size_t)2 * ns + 2 * (size_t)n)) return rc;
    if (int rc = h->v.ensure((size_t)n * ns + 2 * (size_t)n)) return rc;
    if (int rc = h->lo.ensure((size_t)n * 5)) return rc;
    if (int rc = h->scores.ensure((size_t)n * ncand_max)) return rc;
    const size_t NR = (size_t)B / 2 + 1, prof_per = 6 * NR + 1;
    if (int rc = h->prof.ensure((size_t)n * prof_per)) return rc;
    if (diag) if (int rc = h->diag.ensure((size_t)n * B * B)) return rc;
    const float *d_sp = (const float *)spectra;
    if (!on_device) { HIPCHK(hipMemcpyAsync(h->spectra.p, spectra, (size_t)n * per * sizeof(float), hipMemcpyHostToDevice, st)); d_sp = h->spectra.p; }
    HIPCHK(hipMemcpyAsync(h->geo.p, geo.data(), (size_t)ns * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->pos.p, pos.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->pos.p + ns, ring.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->pos.p + 2 * (size_t)ns, ni.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->lo.p, lo.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));

    CtfFitP P;
    P.spectra = d_sp; P.geo = h->geo.p; P.pos = h->pos.p; P.ring = h->pos.p + ns; P.ni = h->pos.p + 2 * (size_t)ns; P.best = h->pos.p + 2 * (size_t)ns + n;
    P.v = h->v.p; P.V = h->v.p + (size_t)n * ns; P.best_score = P.V + n; P.lo = h->lo.p; P.refined = h->lo.p + n;
    P.scores = h->scores.p; P.scores_ld = ncand_max;
    P.n = n; P.T = tile; P.W = W; P.B = B; P.R = B / 2; P.ns = ns; P.bg_w = p.bg_w; P.nc = p.nc; P.nj = p.nj; P.group = shared ? kCtfGridSpectra : 1;
    P.step = cfg->step; P.tol = cfg->tol;
    const double v_ = cfg->kv * 1000.0, lam = 12.2639 / std::sqrt(v_ + 0.97845e-6 * v_ * v_);
    P.k1 = (float)(kPi * lam); P.k2 = (float)(0.5 * cfg->cs * 1e7 * lam * lam); P.extra = (float)std::atan(cfg->wgh / std::sqrt(1.0 - cfg->wgh * cfg->wgh));
    for (int k = 0; k < kCtfThetas; k++) { const double t2 = 2.0 * kPi * k / kCtfThetas; P.c2a[k] = (float)std::cos(t2); P.s2a[k] = (float)std::sin(t2); }
    hipLaunchKernelGGL(k_ctf_condition, dim3((unsigned)n), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_ctf_grid, dim3((unsigned)((ncand_max + 255) / 256), (unsigned)((n + P.group - 1) / P.group)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_ctf_argmax, dim3((unsigned)n), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_ctf_refine, dim3((unsigned)n), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_ctf_profile, dim3((unsigned)n), dim3(256), 0, st, P, h->prof.p, diag ? h->diag.p : (float *)nullptr, p.a, cfg->min_res);
    HIPCHK(hipGetLastError());
    std::vector<double> prof((size_t)n * prof_per);
    HIPCHK(hipMemcpyAsync(prof.data(), h->prof.p, prof.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (diag) HIPCHK(hipMemcpyAsync(diag, h->diag.p, (size_t)n * B * B * sizeof(float), hipMemcpyDeviceToHost, st));
    std::vector<double> refined((size_t)n * 4); std::vector<int> best((size_t)n); std::vector<float> gsc((size_t)n);
    HIPCHK(hipMemcpyAsync(refined.data(), P.refined, refined.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(best.data(), P.best, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (grid_scores) HIPCHK(hipMemcpy2DAsync(grid_scores, (size_t)grid_ld * sizeof(float), h->scores.p, (size_t)ncand_max * sizeof(float), (size_t)ncand_max * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(gsc.data(), P.best_score, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < n; s++) {
        const double *r = &refined[(size_t)s * 4];
        double ang = std::fmod(r[2], 180.0);
        if (ang > 90.0) ang -= 180.0;
        if (ang <= -90.0) ang += 180.0;
        double *o = out_rows + (size_t)s * 8;
        o[0] = r[0] + 0.5 * r[1]; o[1] = r[0] - 0.5 * r[1]; o[2] = ang; o[3] = r[3]; o[4] = (double)best[s]; o[5] = (double)gsc[s]; o[6] = (double)ns; o[7] = prof[(size_t)s * prof_per + 6 * NR];
        if (avrot) std::memcpy(avrot + (size_t)s * 6 * NR, &prof[(size_t)s * prof_per], 6 * NR * sizeof(double));
    }
    return 0;
}

extern "C" int ppm_ctf_estimate(ppm_ctf_t *h, const void *img, int on_device, int nx, int ny, int nframes, int group, int tile,
                                const ppm_ctf_cfg *cfg, double *out_row, double *avrot, float *diag) {
    if (!cfg || !out_row) return fail(-22, "null argument");
    ppm_ctf_fit_info info;
    if (int rc = ppm_ctf_fit_plan(tile, cfg, &info)) return rc;          // a fit that would be refused costs no spectrum
    if (int rc = ppm_ctf_spectrum(h, img, on_device, nx, ny, nframes, group, tile, 0, nullptr, 0)) return rc;
    return ppm_ctf_fit(h, h->power.p, 1, 1, tile, cfg, nullptr, nullptr, out_row, nullptr, 0, avrot, diag);
}
