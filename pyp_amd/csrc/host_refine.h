// host_refine.h — references, matching projections and ppm_refine_batch: pre-processing, grid search and local refinement launches.
#pragma once

// ------------------------------------------------------------------------------ pre-processing launch
static int launch_prep(DevBuf<float2> &spill /* the calling handle's scratch */, const float *d_images, const double *d_rows, int n_img, const Geom &gm, double Rm_px, float fall_px,
                       int normalize, int invert, int do_mask, int whiten, float2 *band, float *wring,
                       const uint32_t *samples, int S_pad, float2 *Il, float *cw, float2 *Wp, float *C2, float *nI,
                       unsigned *band_max = nullptr /* insertion: receives the chunk's largest |band| component */,
                       const float *focus_px = nullptr /* focus mask: sphere centre and radius in pixels, or null */) {
    if (int rc = ensure_plan(gm.N)) return rc;
    PrepP P;
    P.images = d_images; P.rows = d_rows; P.plan = g.plans[gm.N].plan;
    P.N = gm.N; P.B = gm.B; P.W = gm.W; P.H = gm.H;
    P.r_hi2 = (float)(gm.r_hi * gm.r_hi); P.Rm = (float)Rm_px; P.wfall = fall_px; P.a = (float)gm.a;
    // background pixels: r^2 > Rm^2 taken in double (an integer r^2 exceeds the double Rm^2 exactly when it exceeds its floor); a
    // float Rm^2 rounds radii like 0.4 N px / px onto the integer r^2 of a pixel ring and drops that ring from the statistics
    P.Rm2_bg = (float)std::min(std::floor(Rm_px * Rm_px), 16777216.0);
    P.normalize = normalize; P.invert = invert; P.do_mask = do_mask; P.whiten = whiten;
    for (int k = 0; k < 4; k++) P.focus[k] = focus_px ? focus_px[k] : 0.f;
    P.band_max = band_max;
    P.band = band; P.wring = wring; P.samples = samples; P.S_pad = S_pad; P.Il = Il; P.cw = cw;
    P.Wp = Wp; P.C2 = C2; P.nI = nI; P.Bs = gm.Bs; P.Hs = gm.Hs;
    P.r_s2 = (float)(gm.r_s * gm.r_s); P.r_lo2 = (float)(gm.r_lo * gm.r_lo);
    // Two block shapes, one per path of k_prep (ppm_kernels.h); prep_plan (ppm_geom.h) chooses and sizes them.  The FFT stages are
    // barrier-bound: several small independent blocks overlap each other's barrier waits.  A/B on one box, 100 k x 256^2 insertion
    // workload, us per particle (CHANGELOG.md, Round 2): 512 threads / 80 KB (233 VGPRs: ONE block per CU resident) 0.456; 512 threads
    // held to 128 VGPRs for two blocks 0.646 (spills); 1024 threads / 160 KB 0.69; 256 threads / 52 KB at 233 VGPRs (two blocks) 0.399;
    // 256 threads / 40 KB held to 168 VGPRs (three blocks, 252 B of scratch) 0.376 <- every box but 256.
    // Box 256 is scratch-free: one 512-thread block per CU keeps the half spectrum in registers between the row and the column phase
    // (same workload: reconstruction 0.38 -> 0.29 us per particle, refinement 0.44 -> 0.37)
    const PrepPlan pl = prep_plan(gm.N, gm.B, gm.W);
    if (pl.err) return fail(-12, pl.err);
    P.L = pl.L; P.nc = pl.nc; P.nchunks = pl.nchunks; P.TS = pl.TS; P.WS = pl.WS;
    P.spill = nullptr;
    if (!pl.scratch_free) {     // the whole half spectrum goes through a global scratch between the two phases
        if (int rc = spill.ensure((size_t)n_img * gm.N * gm.W)) return rc;
        P.spill = spill.p;
    }
    if (int rc = pl.scratch_free ? raise_lds_limit((const void *)k_prep<512, 2>, 160 * 1024) : raise_lds_limit((const void *)k_prep<256, 3>, 80 * 1024)) return rc;
    ProfScope ps(PPM_K_PREP);
    if (pl.scratch_free) hipLaunchKernelGGL((k_prep<512, 2>), dim3(n_img), dim3(512), pl.lds.total, cur_stream(), P);
    else hipLaunchKernelGGL((k_prep<256, 3>), dim3(n_img), dim3(256), pl.lds.total, cur_stream(), P);
    HIPCHK(hipGetLastError());
    return 0;
}

// The k_global instantiation for a shift window of R steps either side (1 .. 6; anything else takes 6: wider windows go to k_gfft, or to
// tiles of this one), one or both halves of psi, and a search band of Bs: launch_global runs this pointer and ppm_overlap.h reads
// its registers and LDS
template <int... I>
static const void *global_kernel_at(int i, std::integer_sequence<int, I...>) {
    static const void *const fn[] = { (const void *)k_global<I / 4 + 1, (I & 2) != 0, (I & 1) != 0>... };
    return fn[i];
}
static const void *global_kernel(int R, bool half, int Bs) {
    const bool two = Bs <= 31;          // search bands of at most 32 pixels: two slices per wave (k_global<.., TWO>)
    return global_kernel_at(((R >= 1 && R <= 5 ? R : 6) - 1) * 4 + (half ? 2 : 0) + (two ? 1 : 0), std::make_integer_sequence<int, 24>());
}
// dynamic LDS of a k_global launch: the W tables of a block's particles, or the top-K pass's copy of a particle's scores when that is larger
static size_t global_lds_bytes(int HsP, int n_orient, int R, int *topk_lds) {
    size_t lds = (size_t)HsP * 64 * sizeof(float2) * global_particles(R);
    if (lds < 1024) lds = 1024;
    // the top-K pass re-uses the block's LDS for a copy of the particle's scores of this launch (one section of the grid) when they
    // fit (160 KB = 40 928 orientations, e.g. 8 deg at C1 in one section); larger sections select on the global scratch instead
    const size_t lds_topk = (size_t)(32 + n_orient) * sizeof(float);
    const int fits = lds_topk <= (size_t)160 * 1024 ? 1 : 0;
    if (topk_lds) *topk_lds = fits;
    if (fits && lds_topk > lds) lds = lds_topk;
    return lds;
}
static int launch_global(GlobP &P, int n_img, bool half, int R) {
    P.n = n_img;
    const size_t lds = global_lds_bytes(P.HsP, P.n_orient, R, &P.topk_lds);
    const void *fn = global_kernel(R, half, P.Bs);
    if (int rc = raise_lds_limit(fn, 160 * 1024)) return rc;
    ProfScope ps(PPM_K_GLOBAL);
    // resident grid: every block takes most of a CU's LDS, so a CU holds one; the blocks walk the particle groups in strides of the grid
    const int ngroups = (n_img + global_particles(R) - 1) / global_particles(R);
    void *args[] = { &P };
    HIPCHK(hipLaunchKernel(fn, dim3(std::min(ngroups, g.cu_count)), dim3(global_threads(R)), args, lds, cur_stream()));
    return 0;
}

// Full-window correlation (ppm_gfft.h): LDS plan and launch.  Returns -1 when the search grid is outside what the kernel is built
// for (Ns = 16 .. 128), in which case the caller keeps the tiled k_global.
struct GfftPlan { int LN = 0, L = 0, RC = 0, nchunk = 1; size_t fixed = 0, t_bytes = 0, lds = 0; int topk_lds = 0; };
static bool gfft_plan(const Geom &gm, GfftPlan &pl) {
    int LN = 0; while ((1 << LN) < gm.Ns) LN++;
    if ((1 << LN) != gm.Ns || LN < 4 || LN > 7) return false;
    pl.LN = LN; pl.L = gm.Ns / 2;
    const int L = pl.L, G = gfft_slices_per_pass(L), NR = 2 * gm.RSy + 1;
    const size_t row = (size_t)G * 2 * gfft_row_stride(L) * sizeof(float2), fixed = (size_t)L * L * sizeof(float4) + gfft_small_bytes(L);
    const size_t room = (size_t)160 * 1024 - fixed;
    int RC = NR;
    if (const char *e = getenv("PPM_GFFT_ROWS")) { const int v = atoi(e); if (v > 0 && v < RC) RC = v; }       // tests: force several row chunks
    if ((size_t)RC * row > room) RC = (int)(room / row);
    if (RC > 2 * L) RC = 2 * L;
    pl.RC = RC; pl.nchunk = (NR + RC - 1) / RC;
    pl.RC = (NR + pl.nchunk - 1) / pl.nchunk;        // even chunks
    pl.t_bytes = std::max((size_t)pl.RC * row, (size_t)G * L * L * sizeof(float4));        // T doubles as the staging area of the bank slice(s) of a pass
    pl.fixed = fixed;
    return true;
}
// ... and where the top-K step keeps its scores: in T when the orientations of one launch (the largest section of the grid) fit
static void gfft_plan_topk(GfftPlan &pl, int n_orient) {
    const size_t topk = (size_t)n_orient * sizeof(float);
    pl.topk_lds = 0;
    if (topk <= pl.t_bytes) pl.topk_lds = 1;
    else if (pl.fixed + topk <= (size_t)160 * 1024) { pl.topk_lds = 1; pl.t_bytes = (topk + 15) & ~(size_t)15; }
    pl.lds = pl.fixed + pl.t_bytes;
}
// the k_gfft instantiation for a search grid of 2^LN points (4 .. 7, gfft_plan), its shift rows in one piece or in chunks
static const void *gfft_kernel(int LN, bool chunked) {
    static const void *const fn[] = { (const void *)k_gfft<4, false>, (const void *)k_gfft<4, true>, (const void *)k_gfft<5, false>, (const void *)k_gfft<5, true>,
                                      (const void *)k_gfft<6, false>, (const void *)k_gfft<6, true>, (const void *)k_gfft<7, false>, (const void *)k_gfft<7, true> };
    return fn[((LN >= 4 && LN <= 6 ? LN : 7) - 4) * 2 + (chunked ? 1 : 0)];
}
static int launch_gfft(GfftP &P, int n_img, const GfftPlan &pl) {
    P.n = n_img; P.RC = pl.RC; P.nchunk = pl.nchunk; P.t_bytes = (int)pl.t_bytes; P.topk_lds = pl.topk_lds;
    const void *fn = gfft_kernel(pl.LN, pl.nchunk > 1);
    if (int rc = raise_lds_limit(fn, 160 * 1024)) return rc;
    ProfScope ps(PPM_K_GLOBAL);
    void *args[] = { &P };
    HIPCHK(hipLaunchKernel(fn, dim3(n_img), dim3(256), args, pl.lds, cur_stream()));
#ifdef PPM_GFFT_STAMPS
    {   // diagnostic build: cycles per phase and wave of blocks 0 .. 3 (ppm_gfft.h)
        float st[4 * 4 * 12];
        HIPCHK(hipStreamSynchronize(cur_stream()));
        HIPCHK(hipMemcpy(st, P.cc, sizeof(st), hipMemcpyDeviceToHost));
        const char *names[12] = { "products", "fft", "stores", "barrier A", "row tail", "barrier B", "twiddles", "loop", "row reads + pairs", "row fft", "row max", "-" };
        const int nsl = P.n_dir * P.npsi_store;
        for (int b = 0; b < 4 && b < n_img; b++) for (int w = 0; w < 4; w++) {
            fprintf(stderr, "k_gfft stamps block %d wave %d (cycles per slice):", b, w);
            for (int i = 0; i < 11; i++) fprintf(stderr, " | %s %.0f", names[i], st[(b * 4 + w) * 12 + i] / nsl);
            fprintf(stderr, "\n");
        }
    }
#endif
    return 0;
}

// ------------------------------------------------------------------------------ refine
// k_defocus: the offsets -nt .. +nt (steps of `step` Angstrom) about every row's defocus, scored at the pose in `states`.  With `ddef`
// the kernel chooses per particle (rcls2 > 0: the choice is scored once more over the classification band); with `all_scores` every
// offset's score is written out and nothing is chosen (constrained search, mode 4).
static void launch_defocus(const CubeView &cv, const Geom &gm, const uint32_t *samples, int S_pad, const float2 *Il, const float *wring, const double *rows,
                           LState *states, int n, int nt, float step, float *ddef, double *all_scores, float rcls2) {
    const int nrings = gm.B + 2;
    DefocusP DP;
    DP.cv = cv; DP.samples = samples; DP.Il = Il; DP.wring = wring; DP.S_pad = S_pad; DP.nrings = nrings; DP.N = gm.N; DP.B = gm.B;
    DP.rlo2 = (float)(gm.r_lo * gm.r_lo); DP.rmax2 = (float)(gm.r_hi * gm.r_hi); DP.ring_signed = (float)std::min(gm.ring_signed, 1e30); DP.a = (float)gm.a;
    DP.rows = rows; DP.states = states; DP.ddef = ddef; DP.nt = nt; DP.step = step; DP.all_scores = all_scores; DP.rcls2 = rcls2;
    long knob = 0;
    if (const char *e = std::getenv("PPM_DEFOCUS_CHUNK")) knob = std::atol(e);                  // tests: several passes at a small box
    DP.tchunk = ppm::defocus_chunk(nt, nrings, knob);                                           // per-wave ring tables of one pass stay below 64 KB
    ProfScope ps(PPM_K_LOCAL);
    hipLaunchKernelGGL(k_defocus, dim3(n), dim3(256), ring_lds_bytes(4, DP.tchunk, nrings), cur_stream(), DP);
}

namespace {
// One k_local launch of a call, the same for every chunk: LocalP but for the chunk's pointers (Il, cw, states: launch_local takes them from
// the chunk's Lane), the threads of a block, the poses per particle (blocks = particles x per_particle) and the in-band samples summed
// over the launch's score evaluations of one particle
// near: the launch runs k_local's tap-reusing instance (the full-band launch; P.near_it says in which iterations it reuses)
struct LocalLaunch { LocalP P = {}; int threads = 0, per_particle = 1; double evals = 0; bool near = false; };
// what a ppm_refine_batch call works out before its chunk loop; the loop's stages read it and write none of it
struct RefineRun {
    ppm_ref *ref = nullptr; const ppm_refine_cfg *cfg = nullptr;
    Geom gm; SampleList sl; CubeView cv;
    int S_pad = 0, nrings = 0, CH = 0;
    int K = 0, Tb = 0, Tc = 0;          // top hits kept; compass iterations of every hit (Tb) and of the best one at the full band (Tc)
    double Rm_px = 0; float fall_px = 0;
    bool focus_on = false, sep_search = false; float focus_px[4] = { 0, 0, 0, 0 };
    // grid search: the window's path and, for k_global, its tiles
    GfftPlan gpl; bool use_fft = false;
    RowPlan rows = {};                                              // row order of k_global's bank (ppm_rows.h); HsP = rows.HsP
    int Rtx = 0, Rty = 0, Rwin = 0, HsP = 0, nslices = 0; std::vector<int> cxs, cys;
    // ... and the sections of the grid (ppm_sections.h) with the offsets of their hit lists: section s keeps kpre[s + 1] - kpre[s] hits
    std::vector<GridSection> secs; std::vector<int> kpre; int sec_dirs = 0;     // sec_dirs: directions of the largest section
    // local refinement
    LocalP base = {}; bool local_tab = false;   // base: what the call's k_local launches share (local_setup)
    double bf = 3.0; bool any_ang = false, any_sh = false;
    double ha0 = 0, hs0 = 0;            // no grid search: the first compass steps about the rows' own poses
    int ndef = 0;                       // defocus offsets tried on either side of the row's values
    int per_iter = 0; bool cls_on = false;
    LocalLaunch hit, fin;               // every hit refined over the search band; one pose per particle (the best hit, or the row's) at the full band
    double sample_evals = 0;            // in-band samples summed over all k_local score evaluations of one particle
    // the local stage of chunk i on a second stream beside the search of chunk i + 1 (ppm_overlap.h)
    bool overlap = false; int tenants = 0;
    unsigned long long *reuse = nullptr;    // PPM_LOCAL_REUSE_COUNT=1: the handle's two tap-reuse counters (device), zeroed for this call

    int ntiles() const { return (int)(cxs.size() * cys.size()); }
    int nsec() const { return (int)secs.size(); }
    size_t bank_slice() const { return (size_t)HsP * 64; }                                  // float2 per stored slice of k_global's bank
    size_t bank4_slice() const { return use_fft ? (size_t)gpl.L * gpl.L : 0; }              // float4 per stored slice of k_gfft's
    size_t HS() const { return (size_t)gm.Hs * 64; }
    int prefix_of(double rband) const { int rg = (int)std::ceil(rband); if (rg > gm.B + 1) rg = gm.B + 1; return sl.ring_off[rg]; }
    // the highest ring a list prefix of S samples holds (a prefix ends with a whole band of rings, build_samples): its samples lie at |k| < ring + 1
    int reach_of(int S) const { int b = gm.B + 2; while (b > 1 && sl.ring_off[b] > S) b--; return std::min(gm.B, b - 1); }
};
constexpr int kTileR = 6;               // k_global keeps its shift window in registers: up to kTileR steps either side without scratch
constexpr int kFinalThreads = 256;      // block of the final (one pose per particle) k_local launch
}  // namespace

static void refine_notes(ppm_ref *ref, const ppm_refine_cfg *cfg, const Geom &gm) {
    ref->note.clear();
    if (gm.r_s_asked > gm.r_s) {
        char b[256];
        std::snprintf(b, sizeof(b), "NOTE: global search band lowered from %.1f to %.1f Fourier pixels (%.2f A instead of %.2f A): the grid-search "
                      "kernel covers 64 pixels; the top hits are refined up to the high-resolution limit as asked", gm.r_s_asked, gm.r_s,
                      gm.N * gm.a / gm.r_s, gm.N * gm.a / gm.r_s_asked);
        ref->note = b;
    }
    if (cfg->global_search && gm.range_capped) {
        char b[320];
        std::snprintf(b, sizeof(b), "%sNOTE: shift window of the grid search: +-%.0f x +-%.0f pixels (%d x %d search-grid steps of %.1f pixels, the most the "
                      "search grid of %d points holds; asked: %.0f pixels); the refinement of the hits is not limited to it", ref->note.empty() ? "" : "\n",
                      gm.RSx * gm.step, gm.RSy * gm.step, gm.RSx, gm.RSy, gm.step, gm.Ns, gm.range_asked_px);
        ref->note += b;
    }
}

// Device memory the slice banks of one section may take, and what the per-chunk workspaces may: a quarter of the device's TOTAL memory
// each — never of what happens to be free (a budget read from the free memory made the chunks of two processes on one device depend on
// which of them asked first).  PPM_BANK_BYTES lowers the banks' share (tests: force several sections).
static size_t workspace_budget() { return g.total_mem / 4; }
static size_t bank_budget() {
    size_t b = g.total_mem / 4;
    if (const char *e = std::getenv("PPM_BANK_BYTES")) { const long long v = std::atoll(e); if (v > 0 && (size_t)v < b) b = (size_t)v; }
    return b;
}

// sections of the grid (ppm_sections.h), the lengths of their hit lists, the top-K plan of k_gfft for the largest of them, the note
static int plan_grid_sections(RefineRun &r) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    std::string err;
    const size_t budget = bank_budget();
    if (!plan_sections(gm.n_dir, gm.npsi_store, r.bank_slice() * sizeof(float2), r.bank4_slice() * sizeof(float4), budget, r.secs, err)) return fail(-22, err);
    if (r.nsec() > 1 && !r.use_fft && r.ntiles() > 1) {
        // the tiled k_global (PPM_GLOBAL_PATH=tiles, the A/B path of wide windows) searches the whole grid from one bank
        char b[320];
        std::snprintf(b, sizeof(b), "PPM_GLOBAL_PATH=tiles keeps the slice bank of the whole grid (%.2f GB at an angular step of %.3g degrees), the bank may take "
                      "%.2f GB; use a coarser angular step or the default path, which searches the grid in sections", (double)r.nslices * r.bank_slice() * sizeof(float2) / 1073741824.0,
                      gm.dstep, budget / 1073741824.0);
        return fail(-22, b);
    }
    r.kpre.assign(1, 0); r.sec_dirs = 0;
    for (const GridSection &sc : r.secs) {
        r.kpre.push_back(r.kpre.back() + std::min(r.K, sc.nd * gm.n_psi));
        r.sec_dirs = std::max(r.sec_dirs, sc.nd);
    }
    if (r.use_fft) gfft_plan_topk(r.gpl, r.sec_dirs * gm.n_psi);
    ref->last_sections = r.nsec();
    if (r.nsec() > 1) {
        char b[200];
        std::snprintf(b, sizeof(b), "%sNOTE: grid search in %d sections of the orientation grid (%d directions, angular step %.3g degrees: the slice banks are "
                      "built and searched one section at a time)", ref->note.empty() ? "" : "\n", r.nsec(), gm.n_dir, gm.dstep);
        ref->note += b;
    }
    return 0;
}

// iteration counts, masks, the sample list (uploaded), the grid search's window path and tiles, its sections, the chunk size
static int refine_plan(RefineRun &r, int n_img) {
    ppm_ref *ref = r.ref; const ppm_refine_cfg *cfg = r.cfg; const Geom &gm = r.gm;
    r.K = cfg->top_hits > 0 ? cfg->top_hits : 20;
    if (r.K > PPM_MAX_TOP_HITS) r.K = PPM_MAX_TOP_HITS;
    if (r.K > gm.n_orient) r.K = gm.n_orient;
    // answers 36 / 37 (ppm.h): a global search always refines its top hits (Tb iterations each); answer 37 decides whether the
    // best hit continues at the full band (Tc iterations).  iters_hit < 0: hits stay at their grid points (test hook).
    r.Tb = cfg->iters_hit > 0 ? cfg->iters_hit : (cfg->iters_hit < 0 ? 0 : 2); r.Tc = cfg->iters_final > 0 ? cfg->iters_final : 7;
    const double fall = cfg->mask_falloff > 0 ? cfg->mask_falloff : 20.0;
    r.fall_px = (float)(fall / gm.a);
    r.Rm_px = cfg->mask_radius / gm.a;
    r.focus_on = cfg->focus[3] > 0.f;     // a focus mask replaces the centred masks of both stages
    for (int k = 0; k < 4; k++) r.focus_px[k] = (float)(cfg->focus[k] / gm.a);
    r.sep_search = !r.focus_on && cfg->global_search && cfg->search_mask_radius > 0 && cfg->search_mask_radius != cfg->mask_radius;

    build_samples(gm, r.sl);
    r.S_pad = (int)r.sl.packed.size();
    r.nrings = gm.B + 2;
    if (int rc = ref->samples.ensure(r.S_pad)) return rc;
    HIPCHK(hipMemcpyAsync(ref->samples.p, r.sl.packed.data(), r.S_pad * sizeof(uint32_t), hipMemcpyHostToDevice, cur_stream()));

    // shift window: the kernel searches +-PPM_MAX_SHIFT_STEPS steps; a wider window is covered by overlapping tiles of that
    // half-width whose union is exactly [-RS, RS] (centres cxs / cys, in steps)
    // k_global keeps its shift window in registers: up to kTileR steps either side without scratch.  Anything wider — PYP's default
    // "search range 0 = mask radius" is +-41 steps at a 256 box and 4 A — goes to the full-window transform (k_gfft, ppm_gfft.h);
    // PPM_GLOBAL_PATH=tiles keeps the tiled k_global (A/B runs and the tests that hold one path against the other), =fft forces
    // the transform for narrow windows too.
    r.use_fft = false;
    if (cfg->global_search && gfft_plan(gm, r.gpl)) {
        const char *gp = getenv("PPM_GLOBAL_PATH");
        const bool force_fft = gp && !strcmp(gp, "fft"), force_tiles = gp && !strcmp(gp, "tiles");
        r.use_fft = force_fft || (!force_tiles && std::max(gm.RSx, gm.RSy) > kTileR);
    }
    r.Rtx = std::min(gm.RSx, kTileR); r.Rty = std::min(gm.RSy, kTileR);
    auto tile_centres = [](int RS, int Rt) {
        const int T = (2 * RS + 1 + 2 * Rt) / (2 * Rt + 1);
        std::vector<int> c(T, 0);
        for (int i = 0; i < T && T > 1; i++) c[i] = -RS + Rt + (int)(((long)i * 2 * (RS - Rt)) / (T - 1));
        return c;
    };
    r.cxs = tile_centres(gm.RSx, r.Rtx); r.cys = tile_centres(gm.RSy, r.Rty);
    r.Rwin = std::max(r.Rtx, r.Rty);
    // bank rows per slice in the order k_global consumes them (ppm_rows.h): steps of four rows, two steps per trip
    static_assert(global_unroll(1) == 4 && global_unroll(PPM_MAX_SHIFT_STEPS) == 4, "row_plan lays the bank out in steps of U = 4 rows");
    r.rows = row_plan(gm.Ns, gm.Bs, global_fold(gm.Bs));
    r.HsP = r.rows.HsP;
    r.nslices = gm.n_dir * gm.npsi_store;
    if (cfg->global_search) if (int rc = plan_grid_sections(r)) return rc;
    // chunk so that the scratch stays well inside HBM
    const size_t NN = (size_t)gm.N * gm.N, HW = (size_t)gm.H * gm.W;
    size_t per = NN * 4 + HW * 8 + (size_t)r.S_pad * 12 + 2 * PPM_NCOL * 8 + (gm.B + 2) * 4;
    if (cfg->global_search) per += r.HS() * 12 + (size_t)r.nslices * 4 + (size_t)gm.n_orient * 8 + (size_t)r.K * (sizeof(Hit) + sizeof(LState)) + sizeof(LState);
    size_t fit = ((size_t)4 << 30) / per;
    if (fit < 64) {
        // Fine angular steps: the per-orientation tables of a particle (norms, scores, shifts, window maxima) stay whole over the
        // sections and outgrow 4 GB per 64 particles (about 1.4 degrees in C1).  The chunk keeps its 64 particles while they fit the
        // workspace share of the device, shrinks below that, and a step whose tables do not fit for one particle is refused here.
        const size_t ws = workspace_budget(), per_all = per + (r.use_fft ? (size_t)gm.n_orient * 8 : 0);
        fit = std::min<size_t>(64, ws / per_all);
        if (fit < 1) {
            char b[320];
            std::snprintf(b, sizeof(b), "angular step of %.3g degrees: the grid search keeps %.1f GB of tables per particle for its %d orientations, "
                          "the workspace holds %.1f GB; use a coarser angular step", gm.dstep, per_all / 1073741824.0, gm.n_orient, ws / 1073741824.0);
            return fail(-22, b);
        }
    }
    int CH = (int)std::min<size_t>((size_t)n_img, fit);
    CH = std::min(CH, 8192);
    if (CH >= 2048) CH &= ~1023;        // whole rounds of blocks: 256 CUs x 1 (k_global) and x 4 (k_local, one block per particle)
    if (const char *e = std::getenv("PPM_CHUNK")) { int v = std::atoi(e); if (v > 0) CH = std::min(CH, v); }   // tests: force several chunks
    r.CH = CH;
    return 0;
}

// per-chunk workspaces of every call that no local stage reads: one set serves both lanes
static int ensure_chunk_buffers(RefineRun &r, bool images_on_device) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    if (!images_on_device) if (int rc = ref->images.ensure((size_t)2 * r.CH * gm.N * gm.N)) return rc;     // double-buffered staging
    return ref->band.ensure((size_t)r.CH * gm.H * gm.W);
}
// ... and one set of those the local stage reads (after local_setup: ndef)
static int ensure_lane(const RefineRun &r, int i) {
    Lane &L = r.ref->lane[i]; const size_t CH = r.CH;
    if (int rc = L.rows_in.ensure(CH * PPM_NCOL)) return rc;
    if (int rc = L.rows_out.ensure(CH * PPM_NCOL)) return rc;
    if (int rc = L.wring.ensure(CH * (r.gm.B + 2))) return rc;
    if (int rc = L.Il.ensure(CH * r.S_pad)) return rc;
    if (int rc = L.cw.ensure(CH * r.S_pad)) return rc;
    if (int rc = L.states2.ensure(CH)) return rc;
    if (r.cfg->global_search) {
        if (int rc = L.hits.ensure(CH * r.K)) return rc;
        if (int rc = L.states.ensure(CH * r.K)) return rc;
    }
    if (r.ndef > 0) if (int rc = L.ddef.ensure(CH)) return rc;
    return 0;
}

// k_global's bank of one section of the grid (rebuilt only when the grid, the band or the section changes: a call of one section finds
// the bank of the call before; with several, every chunk rebuilds every section, and the key keeps the first section of a chunk from
// taking the last section of the chunk before for its own)
static int ensure_bank(const RefineRun &r, const GridSection &sec) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    const std::string key = ref->grid_key + "/d" + std::to_string(sec.d0) + "+" + std::to_string(sec.nd);
    if (ref->bank_key == key) return 0;
    const int nsl = sec.nd * gm.npsi_store;
    BankP BP; BP.cv = r.cv; BP.mats = ref->mats.p + (size_t)sec.d0 * gm.npsi_store * 6; BP.bank = ref->bank.p; BP.nslices = nsl; BP.Bs = gm.Bs; BP.Hs = r.HsP; BP.rows = r.rows;
    BP.r_s2 = (float)(gm.r_s * gm.r_s);
    {
        ProfScope ps(PPM_K_BANK);
        size_t tot = (size_t)nsl * r.bank_slice();
        hipLaunchKernelGGL(k_bank, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), BP);
    }
    HIPCHK(hipGetLastError());
    ref->bank_key = key;
    return 0;
}

// ... and k_gfft's, in the column pass's layout
static int ensure_bank4(const RefineRun &r, const GridSection &sec) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm; const int L = r.gpl.L;
    const std::string key = ref->grid_key + "/d" + std::to_string(sec.d0) + "+" + std::to_string(sec.nd) + "/L" + std::to_string(L);
    if (ref->bank4_key == key) return 0;
    const int nsl = sec.nd * gm.npsi_store;
    Bank4P BP; BP.cv = r.cv; BP.mats = ref->mats.p + (size_t)sec.d0 * gm.npsi_store * 6; BP.bank4 = ref->bank4.p; BP.nslices = nsl; BP.Bs = gm.Bs; BP.L = L; BP.r_s2 = (float)(gm.r_s * gm.r_s);
    ProfScope ps(PPM_K_BANK);
    const size_t tot = (size_t)nsl * r.bank4_slice();
    hipLaunchKernelGGL(k_bank4, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), BP);
    HIPCHK(hipGetLastError());
    ref->bank4_key = key;
    return 0;
}

// grid search: per-chunk workspaces but the lanes' own; twiddles, direction tables and rotation matrices of the whole grid (rebuilt only when the grid /
// band changes); the banks' storage, sized for the largest section
static int ensure_search_tables(RefineRun &r) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm; const int CH = r.CH, nslices = r.nslices, HsP = r.HsP;
    const size_t HS = r.HS(), HSP = (size_t)HsP * 64;
    if (int rc = ref->Wp.ensure((size_t)CH * HS)) return rc;
    if (int rc = ref->C2.ensure((size_t)CH * HS)) return rc;
    if (int rc = ref->nP.ensure((size_t)CH * nslices)) return rc;
    if (int rc = ref->nI.ensure(CH)) return rc;
    if (int rc = ref->cc.ensure((size_t)CH * gm.n_orient)) return rc;
    if (int rc = ref->sh.ensure((size_t)CH * gm.n_orient)) return rc;
    {   // a bank that had to grow is empty again
        const size_t cap = ref->bank.cap;
        if (int rc = ref->bank.ensure((size_t)r.sec_dirs * gm.npsi_store * HSP)) return rc;
        if (ref->bank.cap != cap) ref->bank_key.clear();
    }
    if (r.nsec() > 1) {
        if (int rc = ref->hits_s.ensure((size_t)CH * r.kpre.back())) return rc;
        if (int rc = ref->sec_k.ensure(r.kpre.size())) return rc;
        HIPCHK(hipMemcpyAsync(ref->sec_k.p, r.kpre.data(), r.kpre.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    }
    char key[160];
    std::snprintf(key, sizeof(key), "%d/%.6f/%.6f/%d/%d/%d/%.3f/%.3f", gm.N, gm.r_s, gm.dstep, gm.Ns, gm.npsi_store, HsP, gm.phi_max, gm.theta_max);
    if (ref->grid_key == key) return 0;
    ref->bank_key.clear(); ref->bank4_key.clear();      // the banks were sampled with the old grid's matrices
    std::vector<float> mats((size_t)nslices * 6);
    std::vector<double> dth(gm.n_dir), dph(gm.n_dir);
    for (int d = 0; d < gm.n_dir; d++) {
        grid_direction(gm, d, dth[d], dph[d]);
        for (int k = 0; k < gm.npsi_store; k++) {
            double M[9]; euler_matrix(k * gm.dpsi, dth[d], dph[d], M);
            float *m = &mats[((size_t)d * gm.npsi_store + k) * 6];
            m[0] = (float)M[0]; m[1] = (float)M[1]; m[2] = (float)M[3]; m[3] = (float)M[4]; m[4] = (float)M[6]; m[5] = (float)M[7];
        }
    }
    std::vector<float2> tw(gm.Ns);
    for (int t = 0; t < gm.Ns; t++) tw[t] = make_float2((float)std::cos(2.0 * kPi * t / gm.Ns), (float)std::sin(2.0 * kPi * t / gm.Ns));
    if (int rc = ref->mats.ensure(mats.size())) return rc;
    if (int rc = ref->dir_theta.ensure(gm.n_dir)) return rc;
    if (int rc = ref->dir_phi.ensure(gm.n_dir)) return rc;
    if (int rc = ref->twN.ensure(gm.Ns)) return rc;
    HIPCHK(hipMemcpyAsync(ref->mats.p, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->dir_theta.p, dth.data(), dth.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->dir_phi.p, dph.data(), dph.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->twN.p, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, cur_stream()));
    // row twiddles of the shift window (scalar loads in k_global)
    {
        std::vector<float4> rt((size_t)kRowTwRows * PPM_MAX_SHIFT_STEPS, make_float4(1.f, 1.f, 0.f, 0.f));
        // one entry per pair slot (stored row / 2) of the bank's row order; a quad's step reads its first slot
        for (int tp = 0; 2 * tp < HsP && tp < kRowTwRows; tp++) for (int j = 1; j <= PPM_MAX_SHIFT_STEPS; j++) {
            int t = ((row_slot_t(r.rows, tp) * j) % gm.Ns + gm.Ns) % gm.Ns;
            const float c = (float)std::cos(2.0 * kPi * t / gm.Ns), sn = (float)std::sin(2.0 * kPi * t / gm.Ns);
            rt[(size_t)tp * PPM_MAX_SHIFT_STEPS + j - 1] = make_float4(c, c, sn, sn);
        }
        if (int rc = ref->rowtw.ensure(rt.size())) return rc;
        HIPCHK(hipMemcpyAsync(ref->rowtw.p, rt.data(), rt.size() * sizeof(float4), hipMemcpyHostToDevice, cur_stream()));
    }
    HIPCHK(hipStreamSynchronize(cur_stream()));   // host vectors go out of scope
    ref->grid_key = key;
    return 0;
}

// full-window correlation (k_gfft): the storage of its bank (the largest section: below 4 GB, ppm_sections.h), the twiddle tables of the
// search grid and the column penalties
static int ensure_gfft_tables(RefineRun &r) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    const int L = r.gpl.L;
    if (int rc = ref->part.ensure((size_t)r.CH * gm.n_orient * 2)) return rc;
    {
        const size_t cap = ref->bank4.cap;
        if (int rc = ref->bank4.ensure((size_t)r.sec_dirs * gm.npsi_store * r.bank4_slice())) return rc;
        if (ref->bank4.cap != cap) ref->bank4_key.clear();
    }
    if (ref->gtw_ns != gm.Ns || ref->gtw_rsx != gm.RSx) {
        // twiddle tables of the in-register transforms (ppm_fft_reg.h), (cos, sin) pairs: the butterfly table of the L-point transform
        // (8 floats per entry: w^k, w^2k, w^3k, padding), then the line table w^0 .. w^(L-1) of the Ns-point grid
        const int nb = fr::bfly_entries(L);
        std::vector<float> tw((size_t)fr::tw_table_floats(L) + gm.Ns, 0.f);
        auto put = [&](float *d, double ang) { d[0] = (float)std::cos(ang); d[1] = (float)std::sin(ang); };
        for (int M = L; M >= 8; M /= 4)
            for (int k = 1; k < M / 4; k++)
                for (int j = 1; j <= 3; j++) put(&tw[(size_t)fr::bfly_entry(L, M, k) * 8 + (j - 1) * 2], 2.0 * kPi * j * k / M);
        for (int t = 0; t < L; t++) put(&tw[(size_t)nb * 8 + (size_t)t * 2], 2.0 * kPi * t / gm.Ns);
        // column penalties of the row pass, in the order the L-point transform leaves its outputs: position p holds the columns
        // j = 2 f, 2 f + 1 (f = freq_at(L, p)), column j is the shift sx = j (j < L) or j - Ns
        for (int pp = 0; pp < L; pp++)
            for (int h = 0; h < 2; h++) {
                const int j = 2 * fr::freq_at(L, pp) + h, sx = j < L ? j : j - gm.Ns;
                tw[(size_t)fr::tw_table_floats(L) + 2 * pp + h] = std::abs(sx) <= gm.RSx ? 0.f : -3.0e38f;
            }
        if (int rc = ref->gtw.ensure(tw.size())) return rc;
        HIPCHK(hipMemcpyAsync(ref->gtw.p, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
        HIPCHK(hipStreamSynchronize(cur_stream()));       // the host vector goes out of scope
        ref->gtw_ns = gm.Ns; ref->gtw_rsx = gm.RSx;
    }
    return 0;
}

// r.base, LocalP but for its per-launch fields (T, nr, schedule) and the chunk's pointers: band constants, free parameters, priors, the
// classification band
static int local_setup(RefineRun &r) {
    ppm_ref *ref = r.ref; const ppm_refine_cfg *cfg = r.cfg; const Geom &gm = r.gm; LocalP &LP = r.base;
    r.bf = cfg->band_factor == 0 ? 3.0 : cfg->band_factor;
    r.any_ang = cfg->refine_psi || cfg->refine_theta || cfg->refine_phi; r.any_sh = cfg->refine_x || cfg->refine_y;
    r.ha0 = cfg->local_angle_step > 0 ? cfg->local_angle_step : 2.5; r.hs0 = cfg->local_shift_step > 0 ? cfg->local_shift_step : 2.0;
    r.ndef = cfg->refine_defocus ? ppm::defocus_steps(cfg->defocus_range, cfg->defocus_step, PPM_MAX_DEFOCUS_STEPS) : 0;
    LP.cv = r.cv; LP.samples = ref->samples.p; LP.S_pad = r.S_pad; LP.nrings = r.nrings; LP.N = gm.N;
    LP.tabR = cube_tab_radius(gm.B, r.cv.scale);        // of the full band: decides between tables and arithmetic; a launch sizes its own (local_shape)
    r.local_tab = local_tables_wanted(LP.tabR);
    LP.rlo2 = (float)(gm.r_lo * gm.r_lo); LP.ring_signed = (float)std::min(gm.ring_signed, 1e30);
    LP.en[0] = cfg->refine_psi; LP.en[1] = cfg->refine_theta; LP.en[2] = cfg->refine_phi; LP.en[3] = cfg->refine_x; LP.en[4] = cfg->refine_y;
    LP.use_priors = 0;
    for (int i = 0; i < 5; i++) { LP.pmean[i] = 0; LP.pw[i] = 0; }
    if (cfg->use_priors) {          // Gaussian restraint on the refined parameters (include/ppm.h; same numbers as the oracle's prior_init)
        const double ns = kPi * (gm.r_hi * gm.r_hi - gm.r_lo * gm.r_lo);
        for (int i = 0; i < 5; i++) {
            double var = cfg->prior_var[i], mean = cfg->prior_mean[i];
            if (i >= 3) { mean /= gm.a; var /= gm.a * gm.a; }
            LP.pmean[i] = mean;
            if (LP.en[i] && var > 0 && ns > 0) { LP.pw[i] = 1.0 / (2.0 * var * ns); LP.use_priors = 1; }
        }
    }
    const int nfree = (cfg->refine_psi != 0) + (cfg->refine_theta != 0) + (cfg->refine_phi != 0) + (cfg->refine_x != 0) + (cfg->refine_y != 0);
    r.per_iter = nfree ? 2 * nfree + 2 : 0;     // centre + 2 per free parameter + trial
    if (r.Tb + r.Tc > kMaxIters) return fail(-22, "too many compass iterations requested");
    LP.rmax2_final = (float)(gm.r_hi * gm.r_hi); LP.S_final = r.S_pad;
    // answer 22: LOGP / SIGMA over r_lo .. r_cls; without a defocus refinement the final k_local launch scores it, with one k_defocus does
    r.cls_on = gm.r_cls < gm.r_hi;
    LP.rmax2_class = (float)(gm.r_cls * gm.r_cls); LP.S_class = (r.cls_on && r.ndef == 0) ? r.prefix_of(gm.r_cls) : 0;
    return 0;
}

// `L` with the bands and sample-list prefixes of its L.P.T compass iterations from the steps (ha, hs), halved after each, and the
// in-band samples of their evaluations
static LocalLaunch with_schedule(const RefineRun &r, LocalLaunch L, double ha, double hs, double rcap) {
    for (int t = 0; t < L.P.T; t++) {
        double rb = march_band(r.bf, r.gm.N, r.Rm_px, ha, hs, r.any_ang, r.any_sh, rcap);
        L.P.rmax2_it[t] = (float)(rb * rb); L.P.S_it[t] = r.prefix_of(rb);
        L.evals += (double)L.per_particle * r.per_iter * std::floor(kPi * rb * rb / 2);
        if (L.near && near_reuse_pays(r.any_ang, ha, r.cv.scale, rb)) L.P.near_it |= 1u << t;
        ha *= 0.5; hs *= 0.5;
    }
    return L;
}
// Every hit refined over the search band.  One wave per block up to 1 024 samples per sweep (no cross-wave steps, 64-sample granularity:
// k_local 83.9 -> 80.9 ms per 28 672 particles against two waves, 93.2 with four; CHANGELOG.md, Round 5, "one-wave blocks for the hit
// stage"), two waves above
static LocalLaunch hit_launch(const RefineRun &r) {
    const Geom &gm = r.gm;
    LocalLaunch L; L.P = r.base; L.per_particle = r.K;
    L.P.T = r.Tb; L.P.final_rescore = 0; L.P.nr = std::min(r.nrings, (int)std::ceil(gm.r_s) + 1);
    L = with_schedule(r, L, 0.5 * gm.dstep, gm.step, gm.r_s);
    L.threads = r.Tb > 0 && L.P.S_it[0] > 1024 ? 128 : 64;
    return L;
}
// one pose per particle for T iterations from the steps (ha, hs), then scored at the full band
static LocalLaunch full_band_launch(const RefineRun &r, int T, double ha, double hs) {
    LocalLaunch L; L.P = r.base; L.threads = kFinalThreads; L.near = local_reuse_wanted();
    L.P.T = r.cfg->local_refine ? T : 0; L.P.final_rescore = 1; L.P.nr = r.nrings;
    L = with_schedule(r, L, ha, hs, r.gm.r_hi);
    L.evals += std::floor(kPi * r.gm.r_hi * r.gm.r_hi / 2);
    return L;
}
// ... the best hit, from the steps the hit stage ended with
static LocalLaunch final_launch(const RefineRun &r) { return full_band_launch(r, r.Tc, 0.5 * r.gm.dstep / (double)(1 << r.Tb), r.gm.step / (double)(1 << r.Tb)); }
// ... the row's own pose (no grid search)
static LocalLaunch rows_launch(const RefineRun &r) { return full_band_launch(r, r.Tb + r.Tc, r.ha0, r.hs0); }

// Dynamic LDS of a k_local launch, whether it takes its tap addresses from LDS tables, and the radius of those.  The choice between tables
// and arithmetic is that of the full band (the two round differently, so a stage must not change sides with its band); the tables
// themselves cover the largest marching band of THIS launch — the coordinates its sample-list prefixes reach — so that the one-wave
// blocks of the hit stage stay small (ppm_overlap.h).  Same entries, fewer of them.
struct LocalShape { size_t lds; bool tab; int tabR; };
// the instance of k_local a launch runs: plan_overlap asks the runtime about the one the hit stage really launches
typedef void (*LocalKernel)(LocalP);
static LocalKernel local_kernel(bool tab, bool near) {
    if (near) return tab ? k_local<true, true> : k_local<false, true>;
    return tab ? k_local<true, false> : k_local<false, false>;
}
static LocalShape local_shape(const RefineRun &r, const LocalLaunch &L) {
    const LocalP &LP = L.P;
    const size_t ring = ring_lds_bytes8(L.threads / 64, kMaxCand, LP.nr);
    LocalShape s;
    s.tab = r.local_tab && tables_fit_lds(ring, LP.tabR);
    int S = 0;
    for (int t = 0; t < LP.T; t++) S = std::max(S, LP.S_it[t]);
    if (LP.final_rescore) S = std::max(S, std::max(LP.S_final, LP.S_class));
    s.tabR = std::min(LP.tabR, cube_tab_radius(r.reach_of(S), r.cv.scale));
    s.lds = ring + (s.tab ? cube_tab_bytes(s.tabR) : 0);
    return s;
}
// `L` for the nb particles of the chunk in `ln`, their poses in `states`
static void launch_local(const RefineRun &r, const LocalLaunch &L, const Lane &ln, LState *states, int nb) {
    LocalP LP = L.P;
    LP.Il = ln.Il.p; LP.cw = ln.cw.p; LP.states = states; LP.reuse = L.near ? r.reuse : nullptr;
    const LocalShape s = local_shape(r, L);
    LP.tabR = s.tabR;
    const dim3 grid((unsigned)(nb * L.per_particle)), block(L.threads);
    ProfScope ps(PPM_K_LOCAL);
    hipLaunchKernelGGL(local_kernel(s.tab, L.near), grid, block, s.lds, cur_stream(), LP);
}

// one section of the grid for one chunk: the section's banks (built unless they are the ones in place), slice norms -> k_gfft | one
// k_global tile | tiles + merge -> the section's K best in `hits`.  The per-orientation tables (nP, cc, sh, part) are those of the
// whole grid: the kernels get pointers to the section's first column and the tables' row lengths, and name the grid's orientations
// in their hits.  `ev_pre`, when set, is recorded ahead of k_global: the other stream's hit stage starts with it, not before it.
static int search_section(const RefineRun &r, int nb, const GridSection &sec, Hit *hits, int K, hipEvent_t ev_pre) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    const int HsP = r.HsP, ntiles = r.ntiles(), nsl = sec.nd * gm.npsi_store, sl0 = sec.d0 * gm.npsi_store, o0 = sec.d0 * gm.n_psi;
    if (int rc = ensure_bank(r, sec)) return rc;
    if (r.use_fft) if (int rc = ensure_bank4(r, sec)) return rc;
    GlobP GP;
    GP.bank = ref->bank.p; GP.Wp = ref->Wp.p; GP.nP = ref->nP.p + sl0; GP.nI = ref->nI.p; GP.twN = ref->twN.p; GP.rowtw = ref->rowtw.p;
    GP.cc = ref->cc.p + o0; GP.sh = ref->sh.p + o0; GP.hits = hits;
    GP.Bs = gm.Bs; GP.Hs = gm.Hs; GP.HsP = HsP; GP.rows = r.rows; GP.Ns = gm.Ns; GP.RSx = r.Rtx; GP.RSy = r.Rty;
    GP.n_dir = sec.nd; GP.n_psi = gm.n_psi; GP.npsi_store = gm.npsi_store; GP.n_orient = sec.nd * gm.n_psi; GP.K = K;
    GP.nP_ld = r.nslices; GP.o_ld = gm.n_orient; GP.o_base = o0;
    {
        ProfScope ps(PPM_K_NORMS);
        NormP NP; NP.C2 = ref->C2.p; NP.bank = ref->bank.p; NP.nP = ref->nP.p + sl0; NP.n = nb; NP.nslices = nsl; NP.ldn = r.nslices; NP.Bs = gm.Bs; NP.Hs = gm.Hs; NP.HsP = HsP; NP.rows = r.rows;
        hipLaunchKernelGGL(k_slice_norms, dim3((nb + 127) / 128, (nsl + 127) / 128), dim3(256), 0, cur_stream(), NP);
    }
    if (r.use_fft) {
        GfftP FP;
        FP.bank4 = ref->bank4.p; FP.bank4_bytes = (unsigned)((size_t)nsl * r.bank4_slice() * sizeof(float4)); FP.Wp = ref->Wp.p; FP.nP = ref->nP.p + sl0; FP.nI = ref->nI.p; FP.tw = ref->gtw.p;
        FP.part = ref->part.p + (size_t)o0 * (r.gpl.L == 64 ? 2 : 1); FP.cc = ref->cc.p + o0; FP.hits = hits;
        FP.Bs = gm.Bs; FP.Hs = gm.Hs; FP.RSx = gm.RSx; FP.RSy = gm.RSy;
        FP.n_dir = sec.nd; FP.n_psi = gm.n_psi; FP.npsi_store = gm.npsi_store; FP.n_orient = sec.nd * gm.n_psi; FP.K = K;
        FP.nP_ld = r.nslices; FP.o_ld = gm.n_orient; FP.o_base = o0;
        if (int rc = launch_gfft(FP, nb, r.gpl)) return rc;
    } else if (ntiles == 1) {
        if (ev_pre) HIPCHK(hipEventRecord(ev_pre, cur_stream()));
        if (int rc = launch_global(GP, nb, gm.half != 0, r.Rwin)) return rc;
    } else {
        // tiles of the shift window (one section: plan_grid_sections): ramp the search tables to the tile's centre, search, keep the
        // tile's top-K; then merge
        if (int rc = ref->hits_t.ensure((size_t)ntiles * nb * K)) return rc;
        if (int rc = ref->tile_c.ensure((size_t)2 * ntiles)) return rc;
        std::vector<int> tc(2 * ntiles);
        for (int ty = 0, t = 0; ty < (int)r.cys.size(); ty++) for (int tx = 0; tx < (int)r.cxs.size(); tx++, t++) { tc[t] = r.cxs[tx]; tc[ntiles + t] = r.cys[ty]; }
        HIPCHK(hipMemcpyAsync(ref->tile_c.p, tc.data(), tc.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
        int px = 0, py = 0;
        const size_t tot = (size_t)nb * r.HS();
        for (int t = 0; t < ntiles; t++) {
            const int dcx = tc[t] - px, dcy = tc[ntiles + t] - py;
            if (dcx || dcy) hipLaunchKernelGGL(k_wp_ramp, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), ref->Wp.p, tot, gm.Bs, gm.Ns, dcx, dcy, ref->twN.p);
            px = tc[t]; py = tc[ntiles + t];
            GP.hits = ref->hits_t.p + (size_t)t * nb * K;
            if (int rc = launch_global(GP, nb, gm.half != 0, r.Rwin)) return rc;
        }
        hipLaunchKernelGGL(k_merge_hits, dim3((nb + 127) / 128), dim3(128), 0, cur_stream(), ref->hits_t.p, hits, nb, K, ntiles, ref->tile_c.p, ref->tile_c.p + ntiles);
        HIPCHK(hipStreamSynchronize(cur_stream()));      // the host vector of the centres goes out of scope
    }
    return 0;
}

// grid search of one chunk: the sections of the grid one after another (one section: straight into the chunk's hits; several: every
// section's K best into its list, then the K best of the lists) -> states from the hits.  `L`: the chunk's set of the workspaces the
// local stage reads (hits_local_stage, which may run on another stream beside the next chunk's search_stage)
static int search_stage(const RefineRun &r, int nb, const Lane &L, hipEvent_t ev_pre) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    const int K = r.K;
    if (r.nsec() == 1) {
        if (int rc = search_section(r, nb, r.secs[0], L.hits.p, K, ev_pre)) return rc;
    } else {
        for (int s = 0; s < r.nsec(); s++)
            if (int rc = search_section(r, nb, r.secs[s], ref->hits_s.p + (size_t)r.kpre[s] * nb, r.kpre[s + 1] - r.kpre[s], ev_pre)) return rc;
        ProfScope ps(PPM_K_TOPK);
        hipLaunchKernelGGL(k_merge_sections, dim3(nb), dim3(64), 0, cur_stream(), ref->hits_s.p, L.hits.p, nb, K, r.nsec(), ref->sec_k.p);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(PPM_K_TOPK);
        hipLaunchKernelGGL(k_states_from_hits, dim3((nb * K + 255) / 256), dim3(256), 0, cur_stream(), L.hits.p, L.states.p, nb, K,
                           ref->dir_theta.p, ref->dir_phi.p, gm.n_psi, gm.dpsi, gm.step, 0.5 * gm.dstep, gm.step);
    }
    return 0;
}

// the states of one chunk's hits -> refinement of every hit over the search band -> the best hit, refined at the full band into states2
static void hits_local_stage(const RefineRun &r, int nb, const Lane &L) {
    if (r.Tb > 0) launch_local(r, r.hit, L, L.states.p, nb);
    {
        ProfScope ps(PPM_K_TOPK);
        hipLaunchKernelGGL(k_select_best, dim3((nb + 255) / 256), dim3(256), 0, cur_stream(), L.states.p, L.states2.p, nb, r.K);
    }
    launch_local(r, r.fin, L, L.states2.p, nb);
}

// no grid search: the rows' own poses, refined at the full band into states2
static void rows_stage(const RefineRun &r, int nb, const Lane &L) {
    hipLaunchKernelGGL(k_states_from_rows, dim3((nb + 255) / 256), dim3(256), 0, cur_stream(), L.rows_in.p, L.states2.p, nb, r.gm.a, r.ha0, r.hs0);
    launch_local(r, r.fin, L, L.states2.p, nb);
}

// defocus offsets at the final pose (states2), then the output rows
static int finish_chunk(const RefineRun &r, int nb, const Lane &L) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    const float *d_ddef = nullptr;
    if (r.ndef > 0) {
        launch_defocus(r.cv, gm, ref->samples.p, r.S_pad, L.Il.p, L.wring.p, L.rows_in.p, L.states2.p, nb, r.ndef, r.cfg->defocus_step,
                       L.ddef.p, nullptr, r.cls_on ? (float)(gm.r_cls * gm.r_cls) : 0.f);
        d_ddef = L.ddef.p;
    }
    hipLaunchKernelGGL(k_rows_out, dim3((nb + 255) / 256), dim3(256), 0, cur_stream(), L.states2.p, L.rows_in.p, L.rows_out.p, nb, gm.a, gm.r_cls, gm.r_lo, d_ddef);
    HIPCHK(hipGetLastError());
    return 0;
}

// Whether this call runs the back of chunk i beside the front of chunk i + 1, by the one rule of ppm_overlap.h: the registers and LDS of
// the two kernels as the runtime reports them for THIS build, plus the dynamic LDS of their launches, against a CU's.
// PPM_REFINE_OVERLAP=0 keeps the serial order (A/B runs, tests).
static int plan_overlap(RefineRun &r, int n_img) {
    ppm_ref *ref = r.ref; const Geom &gm = r.gm;
    r.overlap = false; r.tenants = 0;
    OverlapCall c;
    c.global_search = r.cfg->global_search != 0; c.use_fft = r.use_fft; c.ntiles = r.ntiles(); c.nsections = r.nsec();
    c.nchunks = (n_img + r.CH - 1) / r.CH; c.hit_stage = r.Tb > 0;
    const char *e = std::getenv("PPM_REFINE_OVERLAP");
    c.forced_off = e && std::atoi(e) == 0;
    if (!overlap_on(1, c)) return 0;            // not a call the rule overlaps, whatever fits on a CU
    const LocalShape ls = local_shape(r, r.hit);
    hipFuncAttributes ga, la;
    HIPCHK(hipFuncGetAttributes(&ga, global_kernel(r.Rwin, gm.half != 0, gm.Bs)));
    HIPCHK(hipFuncGetAttributes(&la, (const void *)local_kernel(ls.tab, r.hit.near)));
    const OverlapKernel host = { ga.numRegs, global_threads(r.Rwin), (long)ga.sharedSizeBytes + (long)global_lds_bytes(r.HsP, r.secs[0].nd * gm.n_psi, r.Rwin, nullptr) };
    const OverlapKernel tenant = { la.numRegs, r.hit.threads, (long)la.sharedSizeBytes + (long)ls.lds };
    // gfx950 (the only device ppm_init accepts): 512 registers per lane and SIMD handed out in eights, four SIMDs, LDS in blocks of 1 280 bytes
    const OverlapDevice dev = { 512, 4, (long)g.lds_per_cu, 8, 1280 };
    r.tenants = overlap_tenants(host, tenant, dev);
    r.overlap = overlap_on(r.tenants, c);
    if (std::getenv("PPM_TRACE"))
        fprintf(stderr, "ppm_refine_batch: k_global %d VGPRs / %ld B LDS, hit stage %d threads, %d VGPRs / %ld B LDS: %d blocks per CU beside the search, overlap %s\n",
                host.vgprs, host.lds_bytes, tenant.threads, tenant.vgprs, tenant.lds_bytes, r.tenants, r.overlap ? "on" : "off");
    if (!r.overlap) return 0;
    if (int rc = ensure_lane(r, 1)) return rc;
    if (!ref->local) {      // the tenants' stream yields to the search's where the dispatcher has a choice
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&ref->local, hipStreamNonBlocking, lo));
    }
    return 0;
}

// the events of the two-stream chunk loop (one per workspace set); both streams are drained before the loop's frame goes away,
// on the error returns too
struct OverlapStreams {
    ppm_ref *ref = nullptr; hipEvent_t ready[2] = { nullptr, nullptr }, pre[2] = { nullptr, nullptr }, done[2] = { nullptr, nullptr };
    int open(ppm_ref *ref_) {
        ref = ref_;
        for (int i = 0; i < 2; i++) { ready[i] = ev_get(); pre[i] = ev_get(); done[i] = ev_get(); if (!ready[i] || !pre[i] || !done[i]) return fail(-12, "out of events"); }
        return 0;
    }
    int drain() {
        HIPCHK(hipStreamSynchronize(ref->local));
        HIPCHK(hipStreamSynchronize(ref->stream));
        return 0;
    }
    ~OverlapStreams() {
        if (!ref) return;
        (void)hipStreamSynchronize(ref->local); (void)hipStreamSynchronize(ref->stream);
        std::lock_guard<std::mutex> lk(g_mu);
        for (int i = 0; i < 2; i++) for (hipEvent_t e : { ready[i], pre[i], done[i] }) if (e) g.pool.push_back(e);
    }
};

// evaluation counts per particle, for the roofline's algorithmic bytes (ppm_refine_last_counts)
static void refine_counts(const RefineRun &r) {
    const ppm_refine_cfg *cfg = r.cfg; const Geom &gm = r.gm;
    long nl;
    if (cfg->global_search) nl = (long)r.K * r.Tb * r.per_iter + (cfg->local_refine ? (long)r.Tc * r.per_iter : 0) + 1;
    else nl = 1 + (cfg->local_refine ? (long)(r.Tb + r.Tc) * r.per_iter : 0);
    nl += 2L * r.ndef + (r.cls_on ? 1 : 0);
    double evals = r.sample_evals + 2.0 * r.ndef * std::floor(kPi * gm.r_hi * gm.r_hi / 2);
    if (r.cls_on) evals += std::floor(kPi * gm.r_cls * gm.r_cls / 2);
    long *c = r.ref->last_counts;
    c[0] = cfg->global_search ? gm.n_orient : 0;
    c[1] = nl;
    c[2] = (long)std::floor(kPi * gm.r_s * gm.r_s / 2);
    c[3] = (long)evals;         // sum over the local evaluations of their in-band sample counts
}

// the call's tap-reuse counts, once its streams are drained (ppm_refine_last_reuse)
static int read_reuse(const RefineRun &r) {
    if (!r.reuse) return 0;
    unsigned long long h[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(h, r.reuse, sizeof(h), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    r.ref->last_reuse[0] = (long)h[0]; r.ref->last_reuse[1] = (long)h[1];
    if (std::getenv("PPM_TRACE"))
        fprintf(stderr, "ppm_refine_batch: tap reuse in the full-band stage: %llu of %llu neighbour lane-gathers (iterations 0x%x)\n", h[1], h[0], r.fin.P.near_it);
    return 0;
}

extern "C" {

// ------------------------------------------------------------------------------ reference
ppm_ref_t *ppm_reference_create_weighted(const float *vol, int n, float max_band_px, int pad, const float *ring_weight, int n_weight) {
    if (!g.inited) { fail(-1, "ppm_init has not been called"); return nullptr; }
    if (!vol || !box_ok(n) || !(max_band_px > 0)) { fail(-22, "reference box must be even, 32..512, with prime factors 2, 3, 5, 7, and the band positive"); return nullptr; }
    if ((pad != 1 && pad != 2 && pad != 4) || n * pad > 512) { fail(-22, "padding factor must be 1, 2 or 4 with padded box <= 512"); return nullptr; }
    if (max_band_px > n / 2) max_band_px = (float)(n / 2);
    const int np = n * pad;
    int B = (int)std::ceil((double)max_band_px * pad) - 1;
    if (B > np / 2 - 1) B = np / 2 - 1;
    size_t n3 = (size_t)n * n * n, np3 = (size_t)np * np * np;
    struct Undo { ppm_ref *p; ~Undo() { ppm_reference_destroy(p); } } guard{ new ppm_ref() };        // freed on every error return
    ppm_ref *r = guard.p;
    HIPCHKP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    HIPCHKP(hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking));
    StreamScope ss_(r->stream, r->copy);          // the preparation runs on the new handle's own stream: references may be made concurrently
    DevTmp<float> t_vol, t_w; DevTmp<float2> t_f;
    HIPCHKP(t_vol.alloc(n3));
    HIPCHKP(t_f.alloc(np3));
    float *d_vol = t_vol.p; float2 *d_f = t_f.p;
    HIPCHKP(hipMemcpy(d_vol, vol, n3 * sizeof(float), hipMemcpyHostToDevice));
    if (pad > 1) HIPCHKP(hipMemsetAsync(d_f, 0, np3 * sizeof(float2), cur_stream()));
    float *d_w = nullptr;
    if (ring_weight && n_weight > 0) {
        HIPCHKP(t_w.alloc((size_t)n_weight));
        d_w = t_w.p;
        HIPCHKP(hipMemcpyAsync(d_w, ring_weight, (size_t)n_weight * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
    }
    r->N = n; r->pad = pad; r->B = B; r->CX = B + 2; r->CY = 2 * B + 3;
    size_t cube_n = (size_t)r->CX * r->CY * r->CY;
    r->NBX = (r->CX + 3) / 4; r->NBY = (r->CY + 1) / 2;
    const size_t copy_n = (size_t)r->NBX * r->NBY * r->NBY * 16;         // blocked layout, two copies (ppm_dev.h)
    if (2 * copy_n * sizeof(float2) >= ((size_t)1 << 32)) {        // byte offsets of the buffer loads are 32-bit
    fail(-22, "reference cube too large"); return nullptr; }
    r->LB = (unsigned)copy_n;
    if (hipMalloc(&r->cube, 2 * copy_n * sizeof(float2)) != hipSuccess) { r->cube = nullptr; fail(-12, "out of device memory for the reference cube"); return nullptr; }
    HIPCHKP(hipMemsetAsync(r->cube, 0, 2 * copy_n * sizeof(float2), cur_stream()));
    {
        ProfScope ps(PPM_K_BANK);
        hipLaunchKernelGGL(k_ref_load, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, cur_stream(), d_vol, d_f, n, np);
        if (fft3d(d_f, np, false)) return nullptr;
        hipLaunchKernelGGL(k_ref_crop, dim3((unsigned)((cube_n + 255) / 256)), dim3(256), 0, cur_stream(), d_f, r->cube, np, n, B, r->CX, r->CY, r->NBX, r->NBY, r->LB, d_w, n_weight);
    }
    if (hipStreamSynchronize(cur_stream()) != hipSuccess || hipGetLastError() != hipSuccess) { fail(-5, "reference preparation failed on the device"); return nullptr; }
    return std::exchange(guard.p, nullptr);
}

ppm_ref_t *ppm_reference_create_padded(const float *vol, int n, float max_band_px, int pad) { return ppm_reference_create_weighted(vol, n, max_band_px, pad, nullptr, 0); }
ppm_ref_t *ppm_reference_create(const float *vol, int n, float max_band_px) { return ppm_reference_create_weighted(vol, n, max_band_px, 1, nullptr, 0); }

// The cube is freed by hand; every workspace is a DevBuf and goes with `delete`, AFTER the streams are destroyed (the frees used to come
// first).  That order is safe: every entry point drains the handle's streams before it returns, so they are idle here; and were work
// still queued, hipStreamDestroy returns at once and lets it complete, while each hipFree waits for the device before it releases memory.
void ppm_reference_destroy(ppm_ref_t *r) {
    if (!r) return;
    if (r->cube) (void)hipFree(r->cube);
    if (r->local) (void)hipStreamDestroy(r->local);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    if (r->copy) (void)hipStreamDestroy(r->copy);
    delete r;
}

// ------------------------------------------------------------------------------ matching projections
int ppm_match_projections(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const double *rows, int n_rows, float *out) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!ref || !cfg || !rows || !out) return fail(-22, "null argument");
    StreamScope ss_(ref->stream, ref->copy);
    if (n_rows <= 0) return 0;
    ppm_refine_cfg c2 = *cfg; c2.global_search = 0;          // only box, pixel size and the high-resolution limit matter here
    Geom gm; std::string err;
    if (!geom_init(gm, c2, err)) return fail(-22, err);
    if (gm.N != ref->N) return fail(-22, "particle box differs from the reference box");
    if (gm.B > (ref->B + 1) / ref->pad - 1) return fail(-22, "high-resolution limit exceeds the band the reference was prepared for");
    const size_t NN = (size_t)gm.N * gm.N;
    const int CH = (int)std::min<size_t>((size_t)n_rows, std::max<size_t>(1, ((size_t)1 << 30) / (NN * 12)));
    DevTmp<float2> d_f; DevTmp<float> d_o; DevTmp<MatchRow> d_rows;
    HIPCHK(d_f.alloc(NN * CH)); HIPCHK(d_o.alloc(NN * CH)); HIPCHK(d_rows.alloc(CH));
    MatchP MP;
    MP.cv = cube_view(ref);
    MP.rows = d_rows.p; MP.f = d_f.p; MP.N = gm.N; MP.B = gm.B; MP.r_hi2 = (float)(gm.r_hi * gm.r_hi);
    std::vector<MatchRow> hr(CH);
    const float scale = (cfg->invert ? -1.f : 1.f) / (float)gm.N;     // cube = FFT / N: the unnormalised inverse transform needs 1 / N more
    for (int c0 = 0; c0 < n_rows; c0 += CH) {
        const int nb = std::min(CH, n_rows - c0);
        for (int i = 0; i < nb; i++) {
            const double *row = rows + (size_t)(c0 + i) * PPM_NCOL;
            double M[9]; euler_matrix(row[PPM_PSI], row[PPM_THETA], row[PPM_PHI], M);
            MatchRow &q = hr[i];
            q.m[0] = (float)M[0]; q.m[1] = (float)M[1]; q.m[2] = (float)M[3]; q.m[3] = (float)M[4]; q.m[4] = (float)M[6]; q.m[5] = (float)M[7];
            q.sx = (float)(row[PPM_XSHIFT] / gm.a); q.sy = (float)(row[PPM_YSHIFT] / gm.a);
            q.ctf = ctf_from_row(row, gm.N, gm.a);
        }
        HIPCHK(hipMemcpyAsync(d_rows.p, hr.data(), (size_t)nb * sizeof(MatchRow), hipMemcpyHostToDevice, cur_stream()));
        MP.n = nb;
        hipLaunchKernelGGL(k_match_fill, dim3((unsigned)((NN * nb + 255) / 256)), dim3(256), 0, cur_stream(), MP);
        if (int rc = fft2d_batch(d_f.p, gm.N, nb, true)) return rc;
        hipLaunchKernelGGL(k_match_real, dim3((unsigned)((NN * nb + 255) / 256)), dim3(256), 0, cur_stream(), d_f.p, d_o.p, NN * nb, scale);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + (size_t)c0 * NN, d_o.p, NN * nb * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
        HIPCHK(hipStreamSynchronize(cur_stream()));            // `hr` is reused by the next chunk
    }
    return 0;
}

// ------------------------------------------------------------------------------ refine
int ppm_refine_batch(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const void *images, int images_on_device,
                     int n_img, const double *rows_in, double *rows_out) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!ref || !cfg || !images || !rows_in || !rows_out) return fail(-22, "null argument");
    StreamScope ss_(ref->stream, ref->copy);
    if (n_img <= 0) return 0;
    ref->last_sections = 0;
    RefineRun r; r.ref = ref; r.cfg = cfg;
    const Geom &gm = r.gm; std::string err;
    if (!geom_init(r.gm, *cfg, err)) return fail(-22, err);
    if (gm.N != ref->N) return fail(-22, "particle box differs from the reference box");
    refine_notes(ref, cfg, gm);
    if (gm.B > (ref->B + 1) / ref->pad - 1) return fail(-22, "high-resolution limit exceeds the band the reference was prepared for");
    if (cfg->global_search && gm.Bs + 1 > 64)
        return fail(-22, "global search band wider than 64 Fourier pixels is not supported; lower the 'resolution limit for search'");
    if (int rc = refine_plan(r, n_img)) return rc;
    if (int rc = ensure_chunk_buffers(r, images_on_device != 0)) return rc;
    r.cv = cube_view(ref);
    if (cfg->global_search) {       // the tables of the grid and the banks of its first section (the only one of most calls: kept across calls)
        if (int rc = ensure_search_tables(r)) return rc;
        if (int rc = ensure_bank(r, r.secs[0])) return rc;
        if (r.use_fft) { if (int rc = ensure_gfft_tables(r)) return rc; if (int rc = ensure_bank4(r, r.secs[0])) return rc; }
    }
    HIPCHK(hipStreamSynchronize(cur_stream()));
    if (int rc = local_setup(r)) return rc;
    ref->last_reuse[0] = ref->last_reuse[1] = 0;
    if (const char *e = std::getenv("PPM_LOCAL_REUSE_COUNT")) if (std::atoi(e) != 0) {
        if (int rc = ref->reuse.ensure(2)) return rc;
        HIPCHK(hipMemsetAsync(ref->reuse.p, 0, 2 * sizeof(unsigned long long), cur_stream()));
        HIPCHK(hipStreamSynchronize(cur_stream()));         // the second stream's launches add to it as well
        r.reuse = ref->reuse.p;
    }
    if (cfg->global_search) { r.hit = hit_launch(r); r.fin = final_launch(r); }
    else r.fin = rows_launch(r);
    r.sample_evals = r.hit.evals + r.fin.evals;
    if (int rc = ensure_lane(r, 0)) return rc;
    if (int rc = plan_overlap(r, n_img)) return rc;
    ref->last_overlap = r.overlap ? r.tenants : 0;

    const int CH = r.CH;
    const size_t NN = (size_t)gm.N * gm.N;
    const ChunkStager stage{ (const float *)images, ref->images.p, images_on_device != 0, n_img, CH, NN };
    if (int rc = stage.prime()) return rc;
    // front of a chunk: rows upload, refinement spectra (+ search tables when the same mask serves both), grid search -> the states of the hits
    auto front = [&](int c0, int ci, int nb, const Lane &L, hipEvent_t ev_pre) -> int {
        HIPCHK(hipMemcpyAsync(L.rows_in.p, rows_in + (size_t)c0 * PPM_NCOL, (size_t)nb * PPM_NCOL * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
        const float *d_img = stage.chunk_ptr(c0, ci);
        if (int rc = launch_prep(ref->spill, d_img, L.rows_in.p, nb, gm, r.Rm_px, r.fall_px, cfg->normalize, cfg->invert, 1, 1, ref->band.p, L.wring.p,
                                 ref->samples.p, r.S_pad, L.Il.p, L.cw.p,
                                 (cfg->global_search && !r.sep_search) ? ref->Wp.p : nullptr, ref->C2.p, ref->nI.p, nullptr, r.focus_on ? r.focus_px : nullptr)) return rc;
        if (r.sep_search)
            if (int rc = launch_prep(ref->spill, d_img, L.rows_in.p, nb, gm, cfg->search_mask_radius / gm.a, r.fall_px, cfg->normalize, cfg->invert, 1, 1,
                                     ref->band.p, nullptr, nullptr, 0, nullptr, nullptr, ref->Wp.p, ref->C2.p, ref->nI.p)) return rc;
        if (cfg->global_search) if (int rc = search_stage(r, nb, L, ev_pre)) return rc;
        return 0;
    };
    // back of a chunk: local refinement (of the hits, or of the rows' own poses), defocus, output rows
    auto back = [&](int nb, const Lane &L) -> int {
        if (cfg->global_search) hits_local_stage(r, nb, L);
        else rows_stage(r, nb, L);
        return finish_chunk(r, nb, L);
    };
    auto download = [&](int c0, int nb, const Lane &L) -> int {
        HIPCHK(hipMemcpyAsync(rows_out + (size_t)c0 * PPM_NCOL, L.rows_out.p, (size_t)nb * PPM_NCOL * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
        return 0;
    };
    if (!r.overlap) {
        const Lane &L = ref->lane[0];
        for (int c0 = 0, ci = 0; c0 < n_img; c0 += CH, ci++) {
            const int nb = std::min(CH, n_img - c0);
            if (int rc = front(c0, ci, nb, L, nullptr)) return rc;
            if (int rc = back(nb, L)) return rc;
            if (int rc = stage.prefetch_next(c0, ci)) return rc;     // next chunk's images travel while this chunk computes
            if (int rc = download(c0, nb, L)) return rc;
            if (int rc = stage.sync()) return rc;
        }
        refine_counts(r);
        return read_reuse(r);
    }
    // Software pipeline over two streams and the handle's two lanes (chunk parity).  This handle's stream (A)
    // runs the front of chunk i + 1 while the second stream (B) runs the back of chunk i: the hit stage's one-wave blocks move in beside
    // the resident blocks of k_global (ppm_overlap.h), the final stage follows when those have left.  Ordering is by events alone:
    //   A -> B  `ready`: the states of a chunk's hits are written;  `pre`: the next chunk's k_global is next in A's queue (B's hit stage
    //           waits for it too, so that its blocks do not fill the CUs ahead of the search's)
    //   B -> A  `done`: the back of the chunk that used a workspace set has finished, the set may be written again
    // The host drains A and the copy stream at the end of every chunk as before (the image stager's double buffer) and B at the end.
    OverlapStreams os;
    if (int rc = os.open(ref)) return rc;
    int prev_c0 = 0, prev_nb = 0;
    for (int c0 = 0, ci = 0; ; c0 += CH, ci++) {
        const bool more = c0 < n_img;
        const int lane = ci & 1, nb = more ? std::min(CH, n_img - c0) : 0;
        if (more) {
            if (ci >= 2) HIPCHK(hipStreamWaitEvent(cur_stream(), os.done[lane], 0));
            if (int rc = front(c0, ci, nb, ref->lane[lane], os.pre[lane])) return rc;
            HIPCHK(hipEventRecord(os.ready[lane], cur_stream()));
        }
        if (ci >= 1) {
            StreamScope sb(ref->local, ref->copy);
            HIPCHK(hipStreamWaitEvent(cur_stream(), os.ready[lane ^ 1], 0));
            if (more) HIPCHK(hipStreamWaitEvent(cur_stream(), os.pre[lane], 0));
            if (int rc = back(prev_nb, ref->lane[lane ^ 1])) return rc;
            if (int rc = download(prev_c0, prev_nb, ref->lane[lane ^ 1])) return rc;
            HIPCHK(hipEventRecord(os.done[lane ^ 1], cur_stream()));
        }
        if (!more) break;
        if (int rc = stage.prefetch_next(c0, ci)) return rc;
        if (int rc = stage.sync()) return rc;
        prev_c0 = c0; prev_nb = nb;
    }
    if (int rc = os.drain()) return rc;
    refine_counts(r);
    return read_reuse(r);
}


const char *ppm_refine_note(ppm_ref_t *ref) { return ref ? ref->note.c_str() : ""; }

int ppm_refine_last_sections(ppm_ref_t *ref) { return ref ? ref->last_sections : 0; }
int ppm_refine_last_overlap(ppm_ref_t *ref) { return ref ? ref->last_overlap : 0; }
int ppm_refine_last_reuse(ppm_ref_t *ref, long *gathers, long *reused) {
    if (!ref) return fail(-22, "null reference");
    if (gathers) *gathers = ref->last_reuse[0];
    if (reused) *reused = ref->last_reuse[1];
    return 0;
}

int ppm_refine_last_counts(ppm_ref_t *ref, long *n_global, long *n_local, long *samples_global, long *samples_local) {
    if (!ref) return fail(-22, "null reference");
    if (n_global) *n_global = ref->last_counts[0];
    if (n_local) *n_local = ref->last_counts[1];
    if (samples_global) *samples_global = ref->last_counts[2];
    if (samples_local) *samples_local = ref->last_counts[3];
    return 0;
}

}  // extern "C"
