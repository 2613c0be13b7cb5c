// host_sva.h — sub-tomogram alignment and averaging (ppm_sva_align, ppm_sva_align_average, ppm_sva_insert).
#pragma once

// ------------------------------------------------------------------------------ sub-tomogram alignment (3DAVG)
namespace {
double sva_band_weight(const ppm_sva_cfg &c, double s) {
    double w = 1.0;
    if (c.highpass_cutoff > 0 && s < c.highpass_cutoff) { const double d = c.highpass_cutoff - s; w *= c.highpass_decay > 0 ? std::exp(-d * d / (2.0 * c.highpass_decay * c.highpass_decay)) : 0.0; }
    if (c.lowpass_cutoff > 0 && s > c.lowpass_cutoff) { const double d = s - c.lowpass_cutoff; w *= c.lowpass_decay > 0 ? std::exp(-d * d / (2.0 * c.lowpass_decay * c.lowpass_decay)) : 0.0; }
    return w;
}
double sva_band_radius(const ppm_sva_cfg &c) {
    const int N = c.box;
    double s = c.lowpass_cutoff > 0 ? c.lowpass_cutoff + (c.lowpass_decay > 0 ? 3.7169 * c.lowpass_decay : 0.0) : 0.5;
    if (s > 0.5) s = 0.5;
    double r = s * N; if (r > N / 2 - 1) r = N / 2 - 1;
    return r;
}
}  // namespace

// missing-wedge limits of `n` sub-volumes from `first` on -> device ((-90, 90): no wedge); `hw` is the caller's staging vector
static int stage_wedges(std::vector<float> &hw, const float *wedges, size_t first, int n, float *d_wedges) {
    for (int v = 0; v < n; v++) { hw[2 * v] = wedges ? wedges[2 * (first + v)] : -90.f; hw[2 * v + 1] = wedges ? wedges[2 * (first + v) + 1] : 90.f; }
    HIPCHK(hipMemcpyAsync(d_wedges, hw.data(), (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
    return 0;
}

namespace {
// Work arrays and pruning of the 3-D transforms of sub-volumes (sva_transform).  Only kx < KX and |ky|, |kz| <= R are computed
// (KY = lines kept along y); the average takes the full transform (KX = N / 2 + 1, KY = N, R = N / 2).
struct SvaXform {
    int N = 0, R = 0, KX = 0, KY = 0;
    bool fast16 = false;            // box sizes that are multiples of 16 take the two-step transforms (k_sva_x16 / k_sva_yz16); PPM_SVA_GENERIC_FFT: never
    bool fold = false;              // the two-step z pass emits the band's samples itself; false (PPM_SVA_FOLD=0): it writes B back and k_sva_gather16 picks them (A/B, tests)
    SvaWin W;
    float2 *A = nullptr, *B = nullptr;      // work arrays [vol][z][y][KX] and, two-step only, [vol][kx][kyi][z]
    double *spart = nullptr;                // per-block partial sums of the two-step x pass
    int S = 0; const uint32_t *samples = nullptr; const unsigned *pos = nullptr;     // the band's sample list and its `pos` table (alignment; S = 0: none)
};
}  // namespace

// the transform of box N pruned to the band radius R (R = N / 2: the full one), windowed as `window` says (null: the whole sub-volumes, no window)
static SvaXform sva_xform(int N, int R, const ppm_sva_cfg *window) {
    SvaXform T;
    T.N = N; T.R = R; T.KX = sva_kx(N, R); T.KY = sva_ky(N, R);
    T.fast16 = N % 16 == 0 && getenv("PPM_SVA_GENERIC_FFT") == nullptr;
    T.fold = !(getenv("PPM_SVA_FOLD") && atoi(getenv("PPM_SVA_FOLD")) == 0);
    for (int k = 0; k < 3; k++) T.W.w[k] = window ? window->window[k] : 0.f;
    T.W.sigma = window ? window->window_sigma : 0.f;
    return T;
}
// its work arrays for `NB` sub-volumes per launch: grows w.f (and w.g, two-step only), allocates the x pass's partial sums, and only then
// reads the pointers into T
static int sva_bind_work(SvaXform &T, SvaWork &w, int NB, DevTmp<double> &spart) {
    if (int rc = w.f.ensure((size_t)NB * T.N * T.N * T.KX)) return rc;
    if (T.fast16) {
        if (int rc = w.g.ensure((size_t)NB * T.KX * T.KY * T.N)) return rc;
        HIPCHK(spart.alloc(sva_xpass_partials(T.N, NB)));
    }
    T.A = w.f.p; T.B = w.g.p; T.spart = spart.p;
    return 0;
}

// Transforms of `mv` sub-volumes at `vols`.  mode 1: the sub-volumes, normalised by their statistics and windowed; mode 2 (two-step
// only): the window's own transform.  Statistics: the two-step x pass gathers them into stats[mv][2]; the generic path (k_sva_xpass +
// k_fft_lines) reads them there (k_sva_stats, the caller's).  Sink: with `F` the band's samples go to F[mv][S] (through `pos` in the
// z pass, or k_sva_gather16 / k_sva_gather; Fw: the window's transform at the samples, for the normalisation's mean term); without,
// the transform stays in the work array for k_sva_insert (B two-step, A generic).
static int sva_transform(const SvaXform &T, int mode, const float *vols, int mv, double *stats, float2 *F, const float2 *Fw) {
    const int N = T.N, KX = T.KX, KY = T.KY, R = T.R;
    const long NN2 = (long)N * N;
    if (int rc = ensure_plan(N)) return rc;
    if (T.fast16) {
        const int L16 = sva_lines_per_block(N);
        const size_t lds = (size_t)L16 * (N + 1) * sizeof(float2);
        SvaX16P X; X.vol = vols; X.stats = mode == 1 ? T.spart : nullptr; X.A = T.A; X.tw = g.plans[N].plan.tw; X.n = N; X.L = L16; X.KX = KX; X.mode = mode;
        X.nlines = (long)mv * NN2; X.W = T.W;
        hipLaunchKernelGGL(k_sva_x16, dim3((unsigned)(X.nlines / L16)), dim3(256), lds, cur_stream(), X);
        if (mode == 1) hipLaunchKernelGGL(k_sva_stats_sum, dim3(mv), dim3(64), 0, cur_stream(), T.spart, (int)(NN2 / L16), stats);
        SvaYZ16P Y; Y.A = T.A; Y.B = T.B; Y.tw = X.tw; Y.n = N; Y.L = L16; Y.KX = KX; Y.KY = KY; Y.R = R; Y.in_place = 0; Y.nlines = 0;
        Y.pos = nullptr; Y.F = nullptr; Y.S = T.S; Y.stats = nullptr; Y.Fw = nullptr;
        hipLaunchKernelGGL(k_sva_yz16, dim3((unsigned)((long)mv * KX * (N / L16))), dim3(256), lds, cur_stream(), Y);
        Y.in_place = 1; Y.nlines = (long)mv * KX * KY;
        if (F && T.fold) { Y.pos = T.pos; Y.F = F; Y.stats = stats; Y.Fw = Fw; }
        hipLaunchKernelGGL(k_sva_yz16, dim3((unsigned)((Y.nlines + L16 - 1) / L16)), dim3(256), lds, cur_stream(), Y);
        if (F && !T.fold) hipLaunchKernelGGL(k_sva_gather16, dim3((unsigned)((T.S + 255) / 256), mv), dim3(256), 0, cur_stream(), T.B, T.samples, T.S, N, KX, KY, F, stats, Fw);
        return 0;
    }
    // x pass from the real volumes into [vol][z][y][KX], y pass on that, z pass on |ky| <= R only
    SvaXP XP; XP.vol = vols; XP.stats = stats; XP.out = T.A; XP.plan = g.plans[N].plan; XP.n = N; XP.KX = KX; XP.nlines = (long)mv * NN2; XP.W = T.W;
    XP.L = std::max(1, std::min(16, 7000 / N));
    while (NN2 % XP.L) XP.L--;
    hipLaunchKernelGGL(k_sva_xpass, dim3((unsigned)((XP.nlines + XP.L - 1) / XP.L)), dim3(256), (size_t)XP.L * N * sizeof(float2), cur_stream(), XP);
    if (int rc = fft_lines_pass(T.A, N, (long)mv * N * KX, KX, 1, (long)N * KX, KX, 1, false)) return rc;
    if (2 * R + 1 >= N) {
        if (int rc = fft_lines_pass(T.A, N, (long)mv * N * KX, (long)N * KX, 1, NN2 * KX, (long)N * KX, 1, false)) return rc;
    } else {
        if (int rc = fft_lines_pass(T.A, N, (long)mv * (R + 1) * KX, (long)(R + 1) * KX, 1, NN2 * KX, (long)N * KX, 1, false)) return rc;
        if (int rc = fft_lines_pass(T.A + (size_t)(N - R) * KX, N, (long)mv * R * KX, (long)R * KX, 1, NN2 * KX, (long)N * KX, 1, false)) return rc;
    }
    if (F) hipLaunchKernelGGL(k_sva_gather, dim3((unsigned)((T.S + 255) / 256), mv), dim3(256), 0, cur_stream(), T.A, T.samples, T.S, N, KX, F);
    return 0;
}

// ------------------------------------------------------------------------------ sub-tomogram average
// include/ppm.h: ppm_sva_insert.  Per batch of <= 32 sub-volumes: the FULL 3-D transforms (the pruned passes of the alignment with
// the band at Nyquist; normalisation (v - mean) / sigma applied through the statistics the x pass gathers), then one k_sva_insert
// launch that gathers them into the accumulator.
// one batch-wise pass over DEVICE-resident sub-volumes (d_vols: n_vol x N^3 floats); runs on the caller's current stream scope
static int sva_insert_device(ppm_accum_t *a, const ppm_sva_cfg *cfg, const float *d_vols, int n_vol, const float *wedges, const double *poses,
                             const long *index, long index_base) {
    const int N = cfg->box;
    if (!box_ok(N) || N != a->N) return fail(-22, "sub-volume box differs from the accumulator's box (even, 32..512, prime factors 2, 3, 5, 7)");
    if (a->nsym < 1 || a->nsym > kSvaInsMaxSym) return fail(-22, "sub-tomogram averaging: the accumulator has more point-group operators than the kernel holds");
    const size_t n3 = (size_t)N * N * N;
    const int NB = std::min(n_vol, kSvaInsBatch);
    SvaXform T = sva_xform(N, N / 2, nullptr);        // the average is made of the whole sub-volumes: no window, no band-pass
    if (int rc = ensure_plan(N)) return rc;
    DevTmp<double> d_spart, d_stats, d_poses; DevTmp<float> d_wedges; DevTmp<int> d_half;
    if (int rc = sva_bind_work(T, a->sva, NB, d_spart)) return rc;
    HIPCHK(d_stats.alloc((size_t)2 * NB)); HIPCHK(d_poses.alloc((size_t)12 * NB));
    HIPCHK(d_wedges.alloc((size_t)2 * NB)); HIPCHK(d_half.alloc(NB));
    std::vector<float> hw((size_t)2 * NB); std::vector<int> hh(NB);
    long added[2] = { 0, 0 };
    for (int v0 = 0; v0 < n_vol; v0 += NB) {
        const int m = std::min(NB, n_vol - v0);
        const float *dv = d_vols + (size_t)v0 * n3;
        for (int v = 0; v < m; v++) {
            const long key = index ? index[v0 + v] : index_base + (long)(v0 + v);
            hh[v] = (int)(((key % 2) + 2) % 2);
            added[hh[v]]++;
        }
        if (int rc = stage_wedges(hw, wedges, (size_t)v0, m, d_wedges.p)) return rc;
        HIPCHK(hipMemcpyAsync(d_half.p, hh.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
        HIPCHK(hipMemcpyAsync(d_poses.p, poses + (size_t)v0 * 12, (size_t)12 * m * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
        SvaInsP IP;
        {
            ProfScope ps(PPM_K_PREP);
            if (!T.fast16) {
                HIPCHK(hipMemsetAsync(d_stats.p, 0, (size_t)2 * m * sizeof(double), cur_stream()));
                hipLaunchKernelGGL(k_sva_stats, dim3(64, m), dim3(256), 0, cur_stream(), dv, n3, d_stats.p);
            }
            if (int rc = sva_transform(T, 1, dv, m, d_stats.p, nullptr, nullptr)) return rc;
            if (T.fast16) { IP.T = T.B; IP.layout = 1; IP.stats = d_stats.p; }
            else { IP.T = T.A; IP.layout = 0; IP.stats = nullptr; }
        }
        IP.N = N; IP.KX = T.KX; IP.KY = T.KY; IP.nv = m; IP.poses = d_poses.p; IP.wedges = d_wedges.p; IP.half = d_half.p;
        IP.use_wedge = cfg->use_missing_wedge != 0; IP.scale = 1.0f / (float)N; IP.acc = a->acc; IP.sym = a->d_sym; IP.nsym = a->nsym;
        {
            ProfScope ps(PPM_K_INSERT);
            const dim3 grid((unsigned)(((long)N * N * (N / 2 + 1) + 255) / 256));
            if (a->nsym == 1) hipLaunchKernelGGL(k_sva_insert<false>, grid, dim3(256), 0, cur_stream(), IP);
            else hipLaunchKernelGGL(k_sva_insert<true>, grid, dim3(256), 0, cur_stream(), IP);      // every operator's copy of every sub-volume
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(cur_stream()));          // the host tables of the batch are reused
        // the counters follow every completed batch: after an error in a later one they still say which sub-volumes are in the sums
        for (int h = 0; h < 2; h++) { ppm_accum_set_count(a, h, a->counts[h] + added[h]); added[h] = 0; }
    }
    return 0;
}

// ------------------------------------------------------------------------------ sub-tomogram alignment
// Sample list of the band (half space, shell by shell), common to all sub-volumes; the wedge is applied per volume.  Built and sorted
// on the host, uploaded with its `pos` table and kept in ref->sva_band while the band-pass settings stay (S, shell_off: there).
static int sva_band_plan(ppm_ref *ref, const ppm_sva_cfg *cfg, double rband) {
    const int N = cfg->box, R = (int)std::ceil(rband);
    SvaBandPlan &bp = ref->sva_band;
    SvaBandKey key; key.box = (float)N; key.highpass_cutoff = cfg->highpass_cutoff; key.highpass_decay = cfg->highpass_decay;
    key.lowpass_cutoff = cfg->lowpass_cutoff; key.lowpass_decay = cfg->lowpass_decay;
    if (bp.valid && key == bp.key) return 0;
    std::vector<uint32_t> samples; std::vector<float> bandw; std::vector<int> shell_off(R + 2, 0);
    // one pass over the half space, bucketed by shell (the order inside a shell is the scan order kz, ky, kx)
    std::vector<std::vector<uint32_t>> sh_s(R + 1); std::vector<std::vector<float>> sh_w(R + 1);
    for (int kz = -R; kz <= R; kz++) for (int ky = -R; ky <= R; ky++) for (int kx = 0; kx <= R; kx++) {
        const double k2 = (double)kx * kx + (double)ky * ky + (double)kz * kz;
        if (k2 == 0 || k2 >= rband * rband) continue;
        if (kx == 0 && (ky < 0 || (ky == 0 && kz < 0))) continue;
        const double kr = std::sqrt(k2);
        const int sh = (int)std::floor(kr);
        if (sh > R) continue;
        const double w = sva_band_weight(*cfg, kr / N);
        if (w < 1e-3) continue;
        sh_s[sh].push_back(sva_pack(kx, ky, kz)); sh_w[sh].push_back((float)w);
    }
    // inside a shell the samples are grouped by tilt angle and follow a Z-order curve inside a group: the 64 lanes of a wave gather
    // from a compact patch of the reference cube
    auto spread = [](uint32_t v) { uint64_t x = v & 0x3ffu; x = (x | x << 16) & 0x30000ffull; x = (x | x << 8) & 0x300f00full; x = (x | x << 4) & 0x30c30c3ull; x = (x | x << 2) & 0x9249249ull; return x; };
    for (int sh = 0; sh <= R; sh++) {
        std::vector<std::pair<uint64_t, int>> key(sh_s[sh].size());
        for (size_t i = 0; i < key.size(); i++) {
            int kx, ky, kz; sva_unpack(sh_s[sh][i], kx, ky, kz);
            // major key: the tilt angle of the sample's (kx, kz) direction in 4-degree bins, so that the samples a missing wedge
            // removes are whole waves (k_sva_eval skips zero weights)
            double ang = (kx == 0 && kz == 0) ? 0.0 : std::atan2((double)kz, (double)kx) * 180.0 / kPi;
            if (ang > 90.0) ang -= 180.0;
            if (ang <= -90.0) ang += 180.0;
            const uint64_t bin = (uint64_t)std::floor((ang + 90.0) / 4.0);
            key[i] = { bin << 40 | spread((uint32_t)kx) | spread((uint32_t)(ky + R)) << 1 | spread((uint32_t)(kz + R)) << 2, (int)i };
        }
        std::sort(key.begin(), key.end());
        for (const auto &k : key) { samples.push_back(sh_s[sh][k.second]); bandw.push_back(sh_w[sh][k.second]); }
        shell_off[sh + 1] = (int)samples.size();
    }
    const int S = (int)samples.size();
    if (S == 0) return fail(-22, "the band-pass filter leaves no Fourier samples");
    bp.valid = false; bp.fw_valid = false;
    if (int rc = bp.samples.ensure(S)) return rc;
    if (int rc = bp.bandw.ensure(S)) return rc;
    HIPCHK(hipMemcpyAsync(bp.samples.p, samples.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(bp.bandw.p, bandw.data(), (size_t)S * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
    // where a coefficient (kx, kyi, kzi) of the pruned transform sits in the sample list (k_sva_yz16's z pass emits the samples itself)
    const int KX = sva_kx(N, R), KYp = sva_ky(N, R);
    std::vector<unsigned> pos((size_t)KX * KYp * KYp, 0x7fffffffu);
    for (int i = 0; i < S; i++) {
        int kx, ky, kz; sva_unpack(samples[i], kx, ky, kz);
        if (kx >= KX) continue;
        const int kyi = ky >= 0 ? ky : ky + KYp, kzi = kz >= 0 ? kz : kz + KYp;
        pos[((size_t)kx * KYp + kyi) * KYp + kzi] = (unsigned)i | (((kx + ky + kz) & 1) ? 0x80000000u : 0u);
    }
    if (int rc = bp.pos.ensure(pos.size())) return rc;
    HIPCHK(hipMemcpyAsync(bp.pos.p, pos.data(), pos.size() * sizeof(unsigned), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));        // the host vectors go out of use here
    bp.key = key; bp.S = S; bp.shell_off = shell_off; bp.valid = true;
    return 0;
}

namespace {
// search plan of a call (the particle unit of the constrained search: rotations about the specimen axes + 3-D shift)
struct SvaPlan {
    int en[6]; double tol[6];           // the compass search about the start pose
    int eng[6]; double tolg[6];         // ... and about a grid rotation (global search)
    bool global = false; double gstep = 15.0; std::vector<double> grid_d; int n_grid = 0, Kc = 0;
    bool left = false;                  // the grid is cut to the asymmetric unit of ppm_sva_cfg.symmetry: candidates are G N0, not N0 G
    int ncand = 1, T = 0; double steptol = 0.05, ha0 = 0, hs0 = 0;
    double rg = 0;                      // coarse band the grid step allows (probe Delta / 2, rotations only)
};
// The evaluation side of a chunk's search: k_sva_eval's parameters, the state buffers on the device and the accounting.  A "state" is
// a pose under refinement: one per sub-volume, or Kc per sub-volume in the global search.
struct SvaSearch {
    SvaEvalP EP;
    int N = 0, R = 0; double rband = 0, bf = 3.0, rm_px = 0; const std::vector<int> *shell_off = nullptr;
    double *d_poses = nullptr, *d_delta = nullptr, *d_out = nullptr; int *d_vmap = nullptr;     // DevTmps of the call: they never move
    CompassWs *compass = nullptr;       // the compass search's state (k_csp_step_*), the handle's: ensured for a chunk's states before the chunk loop
    std::vector<double> hp, hout;
    double acct_gathers = 0; long acct_sweeps = 0;      // for the roofline: band samples x rotations gathered, summed over the sweeps (wedge-masked samples included)
    int prefix_of(double rb) const { int rg = (int)std::ceil(rb); if (rg > R + 1) rg = R + 1; return (*shell_off)[rg]; }
};
}  // namespace

// states -> device (poses are per STATE; `vm` maps a state to its sub-volume, null = identity)
static int sva_upload_states(SvaSearch &Q, const std::vector<CUnit> &st, const std::vector<int> *vm) {
    const int ns = (int)st.size();
    Q.hp.resize((size_t)12 * ns);
    for (int v = 0; v < ns; v++) pose_pack(st[v], &Q.hp[(size_t)12 * v]);
    HIPCHK(hipMemcpyAsync(Q.d_poses, Q.hp.data(), Q.hp.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    if (vm) HIPCHK(hipMemcpyAsync(Q.d_vmap, vm->data(), vm->size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    Q.EP.vmap = vm ? Q.d_vmap : nullptr;
    return 0;
}

// one evaluation of `nc` candidates per state (nr of them rotated: 0 or 6) at band rb: k_sva_eval + k_sva_finish -> out
static int sva_launch_eval(SvaSearch &Q, int ns, int nc, int nr, double rb, const double *delta, double *out) {
    SvaEvalP &EP = Q.EP;
    EP.delta = delta; EP.ncand = nc; EP.nrot = nr; EP.S_used = Q.prefix_of(rb); EP.rmax2 = (float)(rb * rb);
    Q.acct_gathers += (double)ns * EP.S_used * (1 + nr); Q.acct_sweeps++;
    ProfScope ps(PPM_K_LOCAL);
    // A compass sweep runs best at TWO blocks per CU (8 waves): the seven rotations of a sample patch touch almost the same lines of the
    // reference, and with 16-20 patches in flight per CU the 32 KB L1 keeps none of them (9.6 L2 requests per load instruction;
    // search 0.084 ms per sub-volume at 4-5 blocks, 0.080 at 3, 0.075 at 2, 0.113 at 1: CHANGELOG.md, Round 4, "k_sva_eval").  The
    // blocks per CU are set through the size of the dynamic LDS request: more than a third of the CU's 160 KB.
    size_t tab_lds = cube_tab_bytes(EP.tabR);
    if (nr == 6) tab_lds = std::max(tab_lds, (size_t)(160 * 1024 / 3 + 1024) & ~(size_t)1023);
    if (tab_lds > (size_t)64 * 1024) tab_lds = (size_t)64 * 1024;
    if (nr == 0) hipLaunchKernelGGL(k_sva_eval<0>, dim3(ns, kSvaParts), dim3(256), tab_lds, cur_stream(), EP);
    else if (nr == 6) hipLaunchKernelGGL(k_sva_eval<6>, dim3(ns, kSvaParts), dim3(256), tab_lds, cur_stream(), EP);
    else return fail(-22, "ppm_sva_align: a sweep has 0 or 6 rotated candidates");
    hipLaunchKernelGGL(k_sva_finish, dim3((unsigned)((ns * nc + 255) / 256)), dim3(256), 0, cur_stream(), EP.partial, ns, nc, nr, out);
    return 0;
}

// `Tn` compass iterations of all states at once, steps halved after each: state and decisions on the device (k_csp_step_*), six
// launches per iteration enqueued back to back, the poses come back once at the end
static int sva_compass(SvaSearch &Q, std::vector<CUnit> &st, const std::vector<int> *vm, const int *en, const double *tol, double ha, double hs, int Tn) {
    const int ns = (int)st.size();
    const int nrot = en[0] ? 6 : 0, nsh = en[3] ? 6 : 0, nc = 1 + nrot + nsh;
    if (nc == 1 || ns == 0 || Tn <= 0) return 0;
    if (int rc = sva_upload_states(Q, st, vm)) return rc;
    std::vector<double> hacc((size_t)ns * 6);
    for (int v = 0; v < ns; v++) std::memcpy(&hacc[(size_t)v * 6], st[v].acc, 6 * sizeof(double));
    HIPCHK(hipMemcpyAsync(Q.compass->acc.p, hacc.data(), hacc.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    CompassPoses at;
    at.n_active = ns; at.Nmat = Q.d_poses; at.nstride = 12; at.pshift = Q.d_poses + 9; at.pstride = 12; at.delta = Q.d_delta; at.mean = Q.d_out;
    if (int rc = compass_enqueue(*Q.compass, at, en, tol, Tn, ha, hs,
            [&](double ha_, double hs_) { return march_band(Q.bf, Q.N, Q.rm_px, ha_, hs_, en[0] != 0, en[3] != 0, Q.rband); },
            [&](const double *delta, int ncand, double rb, double *out) { return sva_launch_eval(Q, ns, ncand, ncand > 1 ? nrot : 0, rb, delta, out); })) return rc;      // the compass sweep has the rotated candidates, the trial (one candidate) none
    Q.EP.delta = Q.d_delta;
    Q.hp.resize((size_t)12 * ns);
    HIPCHK(hipMemcpyAsync(Q.hp.data(), Q.d_poses, Q.hp.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(hacc.data(), Q.compass->acc.p, hacc.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    for (int v = 0; v < ns; v++) {
        pose_unpack(&Q.hp[(size_t)12 * v], st[v]);
        std::memcpy(st[v].acc, &hacc[(size_t)v * 6], 6 * sizeof(double));
    }
    return 0;
}

// scores of all states at the full band (one candidate each, zero displacement) -> Q.hout[state]
static int sva_final_scores(SvaSearch &Q, const std::vector<CUnit> &st, const std::vector<int> *vm) {
    const int ns = (int)st.size();
    if (int rc = sva_upload_states(Q, st, vm)) return rc;
    HIPCHK(hipMemsetAsync(Q.d_delta, 0, (size_t)ns * 6 * sizeof(double), cur_stream()));
    if (int rc = sva_launch_eval(Q, ns, 1, 0, Q.rband, Q.d_delta, Q.d_out)) return rc;
    HIPCHK(hipGetLastError());
    Q.hout.resize((size_t)ns);
    HIPCHK(hipMemcpyAsync(Q.hout.data(), Q.d_out, Q.hout.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

// Global search, first half: the grid rotations ranked by the amplitude correlation on the coarse band (k_sva_global), the top Kc per
// sub-volume (ties -> lower grid index) as states of their own, from the start shift -> cand, vm
static int sva_global_candidates(SvaSearch &Q, const SvaPlan &P, const std::vector<CUnit> &st, const float *d_grid, float *d_gscore,
                                 std::vector<CUnit> &cand, std::vector<int> &vm) {
    const int nb = (int)st.size(), n_grid = P.n_grid, Kc = P.Kc;
    if (int rc = sva_upload_states(Q, st, nullptr)) return rc;
    const SvaEvalP &EP = Q.EP;
    SvaGlobalP GP;
    GP.cv = EP.cv; GP.samples = EP.samples; GP.bandw = EP.bandw; GP.F = EP.F; GP.S = EP.S; GP.N = EP.N; GP.S_used = Q.prefix_of(P.rg); GP.rmax2 = (float)(P.rg * P.rg);
    GP.use_wedge = EP.use_wedge; GP.wedges = EP.wedges; GP.poses = Q.d_poses; GP.grid = d_grid; GP.n_grid = n_grid; GP.RC = 8; GP.score = d_gscore; GP.left = P.left;
    { ProfScope ps(PPM_K_GLOBAL); hipLaunchKernelGGL(k_sva_global, dim3((n_grid + GP.RC - 1) / GP.RC, nb), dim3(256), 0, cur_stream(), GP); }
    HIPCHK(hipGetLastError());
    std::vector<float> gsc((size_t)nb * n_grid);
    HIPCHK(hipMemcpyAsync(gsc.data(), d_gscore, gsc.size() * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    cand.clear(); vm.clear(); cand.reserve((size_t)nb * Kc); vm.reserve((size_t)nb * Kc);
    std::vector<int> order(n_grid);
    for (int v = 0; v < nb; v++) {
        const float *sc_ = &gsc[(size_t)v * n_grid];
        for (int q = 0; q < n_grid; q++) order[q] = q;
        std::partial_sort(order.begin(), order.begin() + Kc, order.end(), [&](int x, int y) { return sc_[x] > sc_[y] || (sc_[x] == sc_[y] && x < y); });
        for (int k = 0; k < Kc; k++) {
            CUnit c = st[v];
            const double *G = &P.grid_d[(size_t)order[k] * 9];
            double Nq[9]; if (P.left) mat_mul3(G, st[v].N, Nq); else mat_mul3(st[v].N, G, Nq);
            std::memcpy(c.N, Nq, sizeof(Nq));
            cand.push_back(c); vm.push_back(v);
        }
    }
    return 0;
}

// the search of one chunk's states `st` (one per sub-volume, at the start poses): compass about the start, or the global search —
// candidates, two compass iterations of each, the best at the full band refined again from Delta / 4 and tol_shift / 4 down
static int sva_search_chunk(SvaSearch &Q, const SvaPlan &P, const ppm_sva_cfg *cfg, std::vector<CUnit> &st, const float *d_grid, float *d_gscore) {
    if (!P.global) return sva_compass(Q, st, nullptr, P.en, P.tol, P.ha0, P.hs0, P.T);
    const int nb = (int)st.size(), Kc = P.Kc;
    std::vector<CUnit> cand; std::vector<int> vm;
    if (int rc = sva_global_candidates(Q, P, st, d_grid, d_gscore, cand, vm)) return rc;
    if (int rc = sva_compass(Q, cand, &vm, P.eng, P.tolg, 0.5 * P.gstep, 0.5 * cfg->tol_shift, 2)) return rc;
    if (int rc = sva_final_scores(Q, cand, &vm)) return rc;
    for (int v = 0; v < nb; v++) {
        int bk = 0;
        for (int k = 1; k < Kc; k++) if (Q.hout[(size_t)v * Kc + k] > Q.hout[(size_t)v * Kc + bk]) bk = k;
        st[v] = cand[(size_t)v * Kc + bk];
    }
    const double ha = 0.25 * P.gstep, hs = 0.25 * cfg->tol_shift;
    return sva_compass(Q, st, nullptr, P.eng, P.tolg, ha, hs, compass_iterations(ha, hs, P.steptol, 0));
}

// (the symbol of the global search's point group: checked by the caller, "" for every other search mode)
static SvaPlan sva_search_plan(const ppm_sva_cfg *cfg, const char *sym, int nsym, double rband, double rm_px, double bf) {
    SvaPlan P;
    for (int k = 0; k < 3; k++) { P.en[k] = cfg->tol_angle > 0 && cfg->search_mode != 2; P.tol[k] = cfg->tol_angle; P.en[3 + k] = cfg->tol_shift > 0; P.tol[3 + k] = cfg->tol_shift; }
    P.global = cfg->search_mode == 1;
    P.gstep = cfg->global_step > 0 ? cfg->global_step : 15.0;
    if (P.global) { P.grid_d = sva_rotation_grid(P.gstep, sym); P.n_grid = (int)(P.grid_d.size() / 9); P.left = nsym > 1; }
    P.Kc = cfg->n_candidates > 0 ? cfg->n_candidates : 25; P.Kc = std::min(std::min(P.Kc, 64), std::max(P.n_grid, 1));
    for (int k = 0; k < 6; k++) { P.eng[k] = k < 3 ? 1 : P.en[k]; P.tolg[k] = k < 3 ? P.gstep : P.tol[k]; }
    const int nrot = (P.en[0] || P.global) ? 6 : 0, nsh = P.en[3] ? 6 : 0;
    P.ncand = 1 + nrot + nsh;
    P.steptol = cfg->step_tolerance > 0 ? cfg->step_tolerance : 0.05;
    P.ha0 = 0.5 * cfg->tol_angle; P.hs0 = 0.5 * cfg->tol_shift;
    P.T = cfg->max_iterations;
    if (P.T <= 0) P.T = compass_iterations(P.ha0, P.hs0, P.steptol, 1);
    if (P.ncand == 1) P.T = 0;
    P.rg = P.global ? march_band(bf, cfg->box, rm_px, 0.5 * P.gstep, 0.0, true, false, rband) : rband;
    return P;
}

namespace {
struct SvaUploader {        // the helper thread that copies the next chunk of host volumes; joins on every exit path
    std::thread t; hipError_t err = hipSuccess;
    void join() { if (t.joinable()) t.join(); }
    void start(float *dst, const float *src, size_t bytes, int dev, hipStream_t cs) {
        err = hipSuccess;
        t = std::thread([this, dst, src, bytes, dev, cs] {
            hipError_t e = hipSetDevice(dev);
            if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs);
            if (e == hipSuccess) e = hipStreamSynchronize(cs);
            err = e;
        });
    }
    ~SvaUploader() { join(); }
};
}  // namespace

// band transforms of a chunk's `nb` sub-volumes at `dv` -> F[nb][S], NB per launch; statistics -> d_stats[nb][2]
static int sva_transform_chunk(ppm_ref *ref, const SvaXform &T, const float *dv, int nb, int NB, double *d_stats, float2 *F) {
    const size_t n3 = (size_t)T.N * T.N * T.N;
    HIPCHK(hipMemsetAsync(d_stats, 0, (size_t)2 * nb * sizeof(double), cur_stream()));
    ProfScope ps(PPM_K_PREP);
    if (!T.fast16) hipLaunchKernelGGL(k_sva_stats, dim3(64, nb), dim3(256), 0, cur_stream(), dv, n3, d_stats);       // (the two-step x pass gathers the statistics itself)
    for (int v0 = 0; v0 < nb; v0 += NB) {
        const int m = std::min(NB, nb - v0);
        if (T.fast16) {
            SvaBandPlan &bp = ref->sva_band;
            SvaWindowKey wkey; for (int k = 0; k < 3; k++) wkey.w[k] = T.W.w[k];
            wkey.sigma = T.W.sigma;
            if (!bp.fw_valid || !(wkey == bp.wkey)) {     // the window's own transform, once per window
                if (int rc = bp.Fw.ensure(T.S)) return rc;
                if (int rc = sva_transform(T, 2, dv, 1, nullptr, bp.Fw.p, nullptr)) return rc;
                bp.wkey = wkey; bp.fw_valid = true;
            }
        }
        if (int rc = sva_transform(T, 1, dv + (size_t)v0 * n3, m, d_stats + 2 * v0, F + (size_t)v0 * T.S, T.fast16 ? ref->sva_band.Fw.p : nullptr)) return rc;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

namespace {
// what is fixed before the chunk loop of ppm_sva_align / ppm_sva_align_average
struct SvaRun {
    ppm_ref *ref = nullptr; const ppm_sva_cfg *cfg = nullptr; const float *volumes = nullptr; bool on_device = false; int n_vol = 0;
    int N = 0, R = 0; size_t n3 = 0; double rband = 0, bf = 3.0, rm_px = 0;
    SvaPlan P; SvaXform T; SvaChunks ch;
};
// the call's device temporaries (freed on every exit) and the wedges' staging vector
struct SvaTmp { DevTmp<float> wedges, grid, gscore; DevTmp<double> stats, poses, delta, out, partial, spart; DevTmp<int> vmap; std::vector<float> hw; };
}  // namespace

// validation, the band's sample list (ref->sva_band) and the search plan
static int sva_plan_call(SvaRun &r) {
    ppm_ref *ref = r.ref; const ppm_sva_cfg *cfg = r.cfg;
    const int N = r.N = cfg->box;
    if (!box_ok(N) || N != ref->N) return fail(-22, "sub-volume box differs from the reference box (even, 32..512, prime factors 2, 3, 5, 7)");
    if (ref->pad != 1) return fail(-22, "sub-tomogram alignment needs a reference prepared with padding 1");
    r.rband = sva_band_radius(*cfg);
    if (r.rband > ref->B) return fail(-22, "low-pass limit exceeds the band the reference was prepared for");
    r.n3 = (size_t)N * N * N; r.R = (int)std::ceil(r.rband);
    if (int rc = sva_band_plan(ref, cfg, r.rband)) return rc;
    r.bf = cfg->band_factor == 0 ? 3.0 : cfg->band_factor;
    r.rm_px = std::max(cfg->window[0], std::max(cfg->window[1], cfg->window[2]));
    if (!(r.rm_px > 0)) r.rm_px = 0.4 * N;
    // the reference's point group cuts the global search's grid to the asymmetric unit; no other search mode reads the field
    char sym[9] = { 0 }; int nsym = 1;
    if (cfg->search_mode == 1) {
        std::memcpy(sym, cfg->symmetry, 8);
        std::vector<double> ops;
        nsym = symmetry_ops(sym, ops);
        const char t = sym[0] >= 'a' ? sym[0] - 32 : sym[0];
        const int order = std::atoi(sym + 1);
        // (symmetry_ops stops at 60 operators: an axis of a higher order would come back as a group it is not)
        if (nsym < 1 || (t == 'C' && nsym != order) || (t == 'D' && nsym != 2 * order))
            return fail(-22, std::string("unknown symmetry symbol '") + sym + "' in the sub-tomogram alignment settings (C1, Cn, Dn, T, O, I; at most 60 operators)");
    }
    r.P = sva_search_plan(cfg, sym, nsym, r.rband, r.rm_px, r.bf);
    return 0;
}

// Workspaces of the call and what points into them.  Every ensure of the handle's buffers that r.T and Q.EP name (sva.f, sva.g, sva.F; the
// band's samples, pos and bandw were ensured by sva_band_plan) and the compass state's come first, then the pointers are read; nothing grows
// those buffers again before the call returns.  sva_band.Fw, which sva_transform_chunk may grow, is read from its DevBuf there.
static int sva_workspaces(SvaRun &r, SvaTmp &t, SvaSearch &Q) {
    ppm_ref *ref = r.ref; const SvaPlan &P = r.P; const SvaBandPlan &bp = ref->sva_band;
    const size_t CH = (size_t)r.ch.CH, CHS = r.ch.states;
    if (int rc = sva_bind_work(r.T, ref->sva, r.ch.NB, t.spart)) return rc;
    if (int rc = ref->sva.F.ensure(CH * bp.S)) return rc;
    if (int rc = ref->compass.ensure(CHS)) return rc;
    if (r.ch.staging) if (int rc = ref->sva.vols.ensure((size_t)r.ch.staging * CH * r.n3)) return rc;
    HIPCHK(t.stats.alloc(2 * CH)); HIPCHK(t.poses.alloc(12 * CHS)); HIPCHK(t.delta.alloc(CHS * P.ncand * 6)); HIPCHK(t.out.alloc(CHS * P.ncand));
    HIPCHK(t.vmap.alloc(CHS)); HIPCHK(t.partial.alloc(CHS * kSvaParts * (2 * kMaxCand + 1))); HIPCHK(t.wedges.alloc(2 * CH));
    if (P.global) {
        std::vector<float> gf(P.grid_d.begin(), P.grid_d.end());
        HIPCHK(t.grid.alloc(gf.size())); HIPCHK(t.gscore.alloc(CH * P.n_grid));
        HIPCHK(hipMemcpy(t.grid.p, gf.data(), gf.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    t.hw.resize(2 * CH);
    r.T.S = bp.S; r.T.samples = bp.samples.p; r.T.pos = bp.pos.p;
    Q.N = r.N; Q.R = r.R; Q.rband = r.rband; Q.bf = r.bf; Q.rm_px = r.rm_px; Q.shell_off = &bp.shell_off; Q.compass = &ref->compass;
    Q.d_poses = t.poses.p; Q.d_delta = t.delta.p; Q.d_out = t.out.p; Q.d_vmap = t.vmap.p;
    SvaEvalP &EP = Q.EP;
    EP.cv = cube_view(ref);         // scale = 1: a reference with pad != 1 was refused above
    EP.samples = bp.samples.p; EP.bandw = bp.bandw.p; EP.F = ref->sva.F.p; EP.S = bp.S; EP.N = r.N; EP.use_wedge = r.cfg->use_missing_wedge != 0;
    EP.tabR = ref->B + 4;           // every sample of the band (|k| <= B + 1) and its upper taps
    EP.wedges = t.wedges.p; EP.poses = t.poses.p; EP.delta = t.delta.p; EP.out = t.out.p; EP.vmap = nullptr; EP.partial = t.partial.p;
    return 0;
}

// The volumes of chunk `ci` (from c0 on) in device memory: where the caller has them, or the staging buffer the helper thread filled,
// whose upload of the NEXT chunk starts here (the host drives this chunk's search, a synchronisation per sweep: the copy gets its own
// thread and stream).
static int sva_stage_volumes(const SvaRun &r, SvaUploader &up, int c0, int ci, const float **dv) {
    const size_t chunk = (size_t)r.ch.CH * r.n3;
    *dv = r.volumes + (size_t)c0 * r.n3;
    if (r.on_device) return 0;
    up.join();
    if (up.err != hipSuccess) return fail(-5, std::string("HIP: ") + hipGetErrorString(up.err) + " while uploading sub-volumes");
    float *d_vols = r.ref->sva.vols.p;
    *dv = d_vols + (r.ch.staging == 2 ? (size_t)(ci & 1) * chunk : 0);
    if (c0 + r.ch.CH < r.n_vol) {
        const int nn = std::min(r.ch.CH, r.n_vol - (c0 + r.ch.CH));
        up.start(d_vols + (size_t)((ci + 1) & 1) * chunk, r.volumes + (size_t)(c0 + r.ch.CH) * r.n3, (size_t)nn * r.n3 * sizeof(float), g.device, cur_copy());
    }
    return 0;
}

// ppm_sva_align and ppm_sva_align_average: with an accumulator every chunk is added to the average at its refined poses while it is
// still in device memory (host volumes cross PCIe once per iteration)
static int sva_align_impl(ppm_ref_t *ref, ppm_accum_t *avg, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol, const float *wedges,
                          double *poses, double *scores, const long *index) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!ref || !cfg || !volumes || !poses) return fail(-22, "null argument");
    StreamScope ss_(ref->stream, ref->copy);
    if (n_vol <= 0) return 0;
    const Trace trace_("ppm_sva_align");
    SvaRun r;
    r.ref = ref; r.cfg = cfg; r.volumes = (const float *)volumes; r.on_device = volumes_on_device != 0; r.n_vol = n_vol;
    if (int rc = sva_plan_call(r)) return rc;
    const SvaPlan &P = r.P;
    const int knob = getenv("PPM_SVA_CHUNK") ? std::max(1, atoi(getenv("PPM_SVA_CHUNK"))) : 0;
    r.ch = sva_chunks(n_vol, (size_t)ref->sva_band.S, r.n3, r.on_device, knob, P.global, P.Kc);
    r.T = sva_xform(r.N, r.R, cfg);
    SvaTmp t; SvaSearch Q;
    if (int rc = sva_workspaces(r, t, Q)) return rc;
    trace_.mark("set up");
    const int CH = r.ch.CH;
    if (!r.on_device) {       // first chunk
        HIPCHK(hipMemcpyAsync(ref->sva.vols.p, volumes, (size_t)std::min(CH, n_vol) * r.n3 * sizeof(float), hipMemcpyHostToDevice, cur_copy()));
        HIPCHK(hipStreamSynchronize(cur_copy()));
    }
    SvaUploader up;
    for (int c0 = 0, ci = 0; c0 < n_vol; c0 += CH, ci++) {
        const int nb = std::min(CH, n_vol - c0);
        const float *dv = nullptr;
        if (int rc = sva_stage_volumes(r, up, c0, ci, &dv)) return rc;
        if (int rc = stage_wedges(t.hw, wedges, (size_t)c0, nb, t.wedges.p)) return rc;
        if (int rc = sva_transform_chunk(ref, r.T, dv, nb, r.ch.NB, t.stats.p, ref->sva.F.p)) return rc;
        trace_.mark("chunk pre-processed");
        std::vector<CUnit> st(nb);
        for (int v = 0; v < nb; v++) pose_unpack(poses + (size_t)(c0 + v) * 12, st[v]);
        if (int rc = sva_search_chunk(Q, P, cfg, st, t.grid.p, t.gscore.p)) return rc;
        trace_.mark("chunk searched");
        if (int rc = sva_final_scores(Q, st, nullptr)) return rc;
        for (int v = 0; v < nb; v++) {
            pose_pack(st[v], poses + (size_t)(c0 + v) * 12);
            if (scores) scores[c0 + v] = Q.hout[v];
        }
        if (avg) {
            if (int rc = sva_insert_device(avg, cfg, dv, nb, wedges ? wedges + 2 * (size_t)c0 : nullptr, poses + (size_t)c0 * 12, index ? index + c0 : nullptr, c0)) return rc;
            trace_.mark("chunk averaged");
        }
    }
    // ppm_refine_last_counts after an alignment: grid rotations of the global search, sweeps (k_sva_eval launches), samples of the band
    // (half space, before the wedge), band samples x gathered rotations per sub-volume summed over the sweeps
    ref->last_counts[0] = P.n_grid; ref->last_counts[1] = Q.acct_sweeps; ref->last_counts[2] = ref->sva_band.S; ref->last_counts[3] = (long)(Q.acct_gathers / n_vol);
    return 0;
}

extern "C" int ppm_sva_align(ppm_ref_t *ref, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol, const float *wedges,
                             double *poses, double *scores) {
    return sva_align_impl(ref, nullptr, cfg, volumes, volumes_on_device, n_vol, wedges, poses, scores, nullptr);
}

extern "C" int ppm_sva_align_average(ppm_ref_t *ref, ppm_accum_t *acc, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol,
                                     const float *wedges, double *poses, double *scores, const long *index) {
    if (!acc) return fail(-22, "null accumulator");
    if (cfg && acc->N != cfg->box) return fail(-22, "sub-volume box differs from the accumulator's box");
    return sva_align_impl(ref, acc, cfg, volumes, volumes_on_device, n_vol, wedges, poses, scores, index);
}


extern "C" int ppm_sva_insert(ppm_accum_t *a, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol, const float *wedges,
                              const double *poses, const long *index) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!a || !cfg || !volumes || !poses) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    if (n_vol <= 0) return 0;
    if (volumes_on_device) return sva_insert_device(a, cfg, (const float *)volumes, n_vol, wedges, poses, index, 0);
    const int N = cfg->box;
    if (!box_ok(N) || N != a->N) return fail(-22, "sub-volume box differs from the accumulator's box (even, 32..512, prime factors 2, 3, 5, 7)");
    const size_t n3 = (size_t)N * N * N;
    const int NB = std::min(n_vol, kSvaInsBatch);
    if (int rc = a->sva.vols.ensure((size_t)NB * n3)) return rc;
    for (int v0 = 0; v0 < n_vol; v0 += NB) {            // host volumes: staged batch by batch
        const int m = std::min(NB, n_vol - v0);
        HIPCHK(hipMemcpyAsync(a->sva.vols.p, (const float *)volumes + (size_t)v0 * n3, (size_t)m * n3 * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
        if (int rc = sva_insert_device(a, cfg, a->sva.vols.p, m, wedges ? wedges + 2 * (size_t)v0 : nullptr, poses + (size_t)v0 * 12, index ? index + v0 : nullptr, v0)) return rc;
    }
    return 0;
}
