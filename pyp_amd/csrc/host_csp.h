// host_csp.h — constrained refinement (ppm_csp_refine).
#pragma once

// ------------------------------------------------------------------------------ constrained refinement (csp)
namespace {
struct CUnit { double N[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, p[3] = { 0, 0, 0 }, tl[4] = { 0, 0, 0, 0 }, acc[6] = { 0, 0, 0, 0, 0, 0 }; };

// a unit's pose <-> 12 doubles (N row-major, then the shift): the layout of ppm_sva_align's poses and of the device's state rows
inline void pose_pack(const CUnit &u, double *q) { std::memcpy(q, u.N, 9 * sizeof(double)); std::memcpy(q + 9, u.p, 3 * sizeof(double)); }
inline void pose_unpack(const double *q, CUnit &u) { std::memcpy(u.N, q, 9 * sizeof(double)); std::memcpy(u.p, q + 9, 3 * sizeof(double)); }

// host tables of one ppm_csp_refine call: rows -> units (csp_build_units)
struct CspUnits {
    std::vector<int> row_part, row_tilt;            // [n_proj] unit indices of a row
    std::vector<unsigned char> usable;              // [n_proj] the row takes part in the search
    std::vector<CUnit> parts, tls;
    std::vector<double> s0, g0;                     // [n_proj][2] row shift (pixels) and geometric shift at the start
    std::vector<TiltRot> trot;                      // one set of rotations per tilt instead of four sin / cos pairs per row
    int nu_all = 0;                                 // units of the refined kind
    std::vector<std::vector<int>> urows;            // rows of every unit
    std::vector<unsigned char> refined;
    std::vector<int> unit_slot, active;             // active: refined units with at least one usable row
    std::vector<int> eval_rows, final_rows;         // usable rows of the active units, grouped by unit; all rows of the refined units
    std::vector<int> uoff;                          // [active + 1] the active units' offsets in eval_rows (csp_upload_tables)
    int n_slots = 0;
};
// free parameters and step schedule of the compass search
struct CspSearch { int en[6] = { 0, 0, 0, 0, 0, 0 }; double tol[6] = { 0, 0, 0, 0, 0, 0 }; int nfree = 0, T = 0; double ha0 = 0, hs0 = 0; };
// where the poses of a compass search live on the device, and what it scores into
struct CompassPoses {
    int kind = PPM_CSP_PARTICLES, n_active = 0;
    double *Nmat = nullptr; int nstride = 9;        // rotation matrices, doubles from one unit's to the next
    double *pshift = nullptr; int pstride = 3;      // shifts likewise (the sub-volume search keeps N and p in one row of 12)
    double *tl = nullptr;                           // tilt parameters (null: particles only)
    const int *active = nullptr, *unit_slot = nullptr;      // active list and slot table (null: the identity)
    double *delta = nullptr, *mean = nullptr;       // [slot][ncand][6] candidates of the compass sweep and its [unit][ncand] means
};
// One compass search on the stream, for every search whose state and decisions live on the device (k_csp_step_*): the first candidates,
// then per iteration band -> candidates' scores -> trial step -> its score -> accept, steps halved after each; nothing waits on the host.
// `ws` is the state (ensured by the caller for at.n_active states, ws.acc filled); en / tol: free parameters and their bounds, 1 + 2 per
// free parameter candidates a sweep.  band_of(ha, hs) gives an iteration's band, eval(delta, ncand, band, means_out) enqueues the caller's
// evaluation of `ncand` candidates per unit (1: the trial step; non-zero: give up with that code).
template <class BandOf, class Eval>
static int compass_enqueue(CompassWs &ws, const CompassPoses &at, const int *en, const double *tol, int T, double ha, double hs, BandOf band_of, Eval eval) {
    CspStepP SP;
    SP.kind = at.kind; SP.n_active = at.n_active; SP.ncand = 1; SP.active = at.active; SP.unit_slot = at.unit_slot;
    for (int i = 0; i < 6; i++) { SP.en[i] = en[i]; SP.tol[i] = tol[i]; SP.ncand += en[i] ? 2 : 0; }
    SP.acc = ws.acc.p; SP.dtrial = ws.dtrial.p; SP.fpm = ws.fpm.p; SP.delta_c = at.delta; SP.delta_t = ws.delta_t.p;
    SP.Nmat = at.Nmat; SP.pshift = at.pshift; SP.tl = at.tl; SP.nstride = at.nstride; SP.pstride = at.pstride;
    SP.mean = at.mean; SP.tmean = ws.tmean.p;
    const unsigned gstep = (unsigned)((SP.n_active + 127) / 128);
    SP.ha = ha; SP.hs = hs; SP.ha_next = ha; SP.hs_next = hs;
    hipLaunchKernelGGL(k_csp_step_init, dim3(gstep), dim3(128), 0, cur_stream(), SP);
    for (int it = 0; it < T; it++) {
        const double band = band_of(ha, hs);
        SP.ha = ha; SP.hs = hs; SP.ha_next = 0.5 * ha; SP.hs_next = 0.5 * hs;
        if (int rc = eval(SP.delta_c, SP.ncand, band, at.mean)) return rc;
        hipLaunchKernelGGL(k_csp_step_trial, dim3(gstep), dim3(128), 0, cur_stream(), SP);
        if (int rc = eval(SP.delta_t, 1, band, ws.tmean.p)) return rc;
        hipLaunchKernelGGL(k_csp_step_accept, dim3(gstep), dim3(128), 0, cur_stream(), SP);
        ha *= 0.5; hs *= 0.5;
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// what the stages of a call share
struct CspRun {
    ppm_ref *ref = nullptr; const ppm_refine_cfg *cfg = nullptr; const ppm_csp_cfg *cc = nullptr;
    Geom gm; SampleList sl; int S_pad = 0, nrings = 0; double rm_px = 0;
    int kind = 0, n_proj = 0, n_part = 0, n_tilt = 0;
    CspEvalP EP; bool tab = false;
    const double *particles_in = nullptr;           // the caller's particle block (identifiers of the searched particles)
    std::vector<double> hN, hp, htl, rowtab;        // staging: the units as the device holds them, the exhaustive stage's row tables
    double acct_gathers = 0; long acct_sweeps = 0;  // for the roofline (ppm_refine_last_counts)
    double bf() const { return cfg->band_factor == 0 ? 3.0 : cfg->band_factor; }
    int prefix_of(double rband) const { int rg = (int)std::ceil(rband); if (rg > gm.B + 1) rg = gm.B + 1; return sl.ring_off[rg]; }
};
}  // namespace

// device first: sample list and the prepared spectra of all rows are enqueued before the host builds its unit tables, which then
// happens while the device works (20 k rows: ~1.5 ms of hash maps and poses against ~3 ms of pre-processing).
// The scratch of the constrained search lives in the reference handle (grown on demand, freed with it): allocating and freeing
// several hundred MB per call cost a third of a call on a 20 k-projection series
static int csp_prepare_spectra(CspRun &c, const void *images, int images_on_device, const double *rows, bool mode4) {
    ppm_ref *ref = c.ref; const ppm_refine_cfg *cfg = c.cfg; const Geom &gm = c.gm; const int n_proj = c.n_proj, S_pad = c.S_pad;
    const size_t NN = (size_t)gm.N * gm.N, HW = (size_t)gm.H * gm.W;
    if (int rc = ref->samples.ensure(S_pad)) return rc;
    HIPCHK(hipMemcpyAsync(ref->samples.p, c.sl.packed.data(), S_pad * sizeof(uint32_t), hipMemcpyHostToDevice, cur_stream()));
    const int CH = (int)std::min<size_t>((size_t)n_proj, std::max<size_t>(64, ((size_t)2 << 30) / (NN * 4 + HW * 8)));
    if (int rc = ref->spectra.Il.ensure((size_t)n_proj * S_pad)) return rc;
    if (int rc = ref->spectra.cw.ensure((size_t)n_proj * S_pad)) return rc;
    if (int rc = ref->spectra.band.ensure((size_t)CH * HW)) return rc;
    if (int rc = ref->spectra.rows.ensure((size_t)n_proj * PPM_NCOL)) return rc;
    if (mode4) if (int rc = ref->spectra.wring.ensure((size_t)n_proj * (gm.B + 2))) return rc;
    if (!images_on_device) if (int rc = ref->spectra.img.ensure((size_t)CH * NN)) return rc;
    HIPCHK(hipMemcpyAsync(ref->spectra.rows.p, rows, (size_t)n_proj * PPM_NCOL * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    const double fall = cfg->mask_falloff > 0 ? cfg->mask_falloff : 20.0;
    for (int c0 = 0; c0 < n_proj; c0 += CH) {
        const int nb = std::min(CH, n_proj - c0);
        const float *d_img = (const float *)images + (size_t)c0 * NN;
        if (!images_on_device) {
            HIPCHK(hipMemcpyAsync(ref->spectra.img.p, (const float *)images + (size_t)c0 * NN, (size_t)nb * NN * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
            d_img = ref->spectra.img.p;
        }
        if (int rc = launch_prep(ref->spill, d_img, ref->spectra.rows.p + (size_t)c0 * PPM_NCOL, nb, gm, c.rm_px, (float)(fall / gm.a), cfg->normalize, cfg->invert, 1, 1,
                                 ref->spectra.band.p, mode4 ? ref->spectra.wring.p + (size_t)c0 * (gm.B + 2) : nullptr, ref->samples.p, S_pad, ref->spectra.Il.p + (size_t)c0 * S_pad,
                                 ref->spectra.cw.p + (size_t)c0 * S_pad, nullptr, nullptr, nullptr)) return rc;
        if (!images_on_device) HIPCHK(hipStreamSynchronize(cur_stream()));     // the staging buffer is reused by the next chunk
    }
    return 0;
}

// rows -> units: the particles' and tilts' start state, every row's two units and start shifts, the refined units and their rows
static int csp_build_units(const CspRun &c, const double *rows, const double *particles, const double *tilts, CspUnits &U) {
    const ppm_csp_cfg *cc = c.cc; const Geom &gm = c.gm; const int kind = c.kind, n_proj = c.n_proj, n_part = c.n_part, n_tilt = c.n_tilt;
    std::unordered_map<long, int> pmap, tmap;          // tilt key: (TIND, RIND) folded into one integer
    pmap.reserve((size_t)n_part * 2); tmap.reserve((size_t)n_tilt * 2);
    auto tkey = [](long tind, long rind) { return tind * 1000003L + rind; };
    for (int i = 0; i < n_part; i++) pmap[(long)particles[(size_t)i * PPM_NPCOL]] = i;
    for (int i = 0; i < n_tilt; i++) tmap[tkey((long)tilts[(size_t)i * PPM_NTCOL], (long)tilts[(size_t)i * PPM_NTCOL + 1])] = i;
    U.row_part.resize(n_proj); U.row_tilt.resize(n_proj); U.usable.resize(n_proj);
    U.parts.assign(n_part, CUnit()); U.tls.assign(n_tilt, CUnit());
    for (int i = 0; i < n_part; i++) {
        const double *P = particles + (size_t)i * PPM_NPCOL;
        euler_matrix(-P[4], -P[5], -P[6], U.parts[i].N);
        U.parts[i].p[0] = P[1]; U.parts[i].p[1] = P[2]; U.parts[i].p[2] = P[3];
    }
    for (int i = 0; i < n_tilt; i++) {
        const double *T = tilts + (size_t)i * PPM_NTCOL;
        U.tls[i].tl[0] = T[4]; U.tls[i].tl[1] = T[5]; U.tls[i].tl[2] = T[2]; U.tls[i].tl[3] = T[3];
    }
    U.s0.resize((size_t)2 * n_proj); U.g0.resize((size_t)2 * n_proj);
    U.trot.resize(n_tilt);
    for (int i = 0; i < n_tilt; i++) tilt_rotations(U.tls[i].tl[0], U.tls[i].tl[1], U.trot[i]);
    for (int j = 0; j < n_proj; j++) {
        const double *row = rows + (size_t)j * PPM_NCOL;
        auto ip = pmap.find((long)row[PPM_PIND]); auto it = tmap.find(tkey((long)row[PPM_TIND], (long)row[28]));
        if (ip == pmap.end() || it == tmap.end()) return fail(-22, "csp: row " + std::to_string(j + 1) + " refers to a particle or tilt missing from the extended parameters");
        U.row_part[j] = ip->second; U.row_tilt[j] = it->second;
        const long tind = (long)row[PPM_TIND];
        U.usable[j] = row[PPM_OCC] > 0 && tind >= cc->tind_min && (cc->tind_max < 0 || tind <= cc->tind_max);
        U.s0[2 * j] = row[PPM_XSHIFT] / gm.a; U.s0[2 * j + 1] = row[PPM_YSHIFT] / gm.a;
        double M[9];
        const CUnit &pu = U.parts[U.row_part[j]], &tu = U.tls[U.row_tilt[j]];
        csp_row_pose(pu.N, pu.p, U.trot[U.row_tilt[j]], tu.tl[2], tu.tl[3], M, &U.g0[2 * j]);
    }
    const int nu_all = U.nu_all = kind == PPM_CSP_PARTICLES ? n_part : n_tilt;
    U.urows.assign(nu_all, std::vector<int>());
    for (int j = 0; j < n_proj; j++) U.urows[kind == PPM_CSP_PARTICLES ? U.row_part[j] : U.row_tilt[j]].push_back(j);
    U.unit_slot.assign(nu_all, -1); U.active.clear();
    U.refined.assign(nu_all, 0);
    for (int u = 0; u < nu_all; u++) {
        const long id = (long)(kind == PPM_CSP_PARTICLES ? particles[(size_t)u * PPM_NPCOL] : tilts[(size_t)u * PPM_NTCOL]);
        if (id < cc->first || (cc->last >= 0 && id > cc->last)) continue;
        U.refined[u] = 1;
        int nus = 0; for (int j : U.urows[u]) nus += U.usable[j];
        if (nus) { U.unit_slot[u] = (int)U.active.size(); U.active.push_back(u); }
    }
    for (int u : U.active) for (int j : U.urows[u]) if (U.usable[j]) U.eval_rows.push_back(j);
    for (int u = 0; u < nu_all; u++) if (U.refined[u]) for (int j : U.urows[u]) U.final_rows.push_back(j);
    // units without usable rows still need a slot for the final scoring of their rows (zero displacement)
    U.n_slots = (int)U.active.size();
    for (int u = 0; u < nu_all; u++) if (U.refined[u] && U.unit_slot[u] < 0) U.unit_slot[u] = U.n_slots++;
    // in the other kind's lookups (a particle sweep reads the tilt of a row and vice versa) no slot is needed
    return 0;
}

static CspSearch csp_search_plan(const ppm_csp_cfg *cc, int kind, bool any_active) {
    CspSearch P;
    int *en = P.en; double *tol = P.tol;
    if (kind == PPM_CSP_PARTICLES) {
        for (int k = 0; k < 3; k++) { en[k] = cc->refine_rotation != 0; tol[k] = cc->tol_angle[k]; en[3 + k] = cc->refine_translation != 0; tol[3 + k] = cc->tol_shift; }
    } else {
        en[0] = en[1] = cc->refine_rotation != 0; tol[0] = cc->tol_angle[0]; tol[1] = cc->tol_angle[1];
        en[3] = en[4] = cc->refine_translation != 0; tol[3] = tol[4] = cc->tol_shift;
    }
    for (int k = 0; k < 6; k++) { if (!(tol[k] > 0)) en[k] = 0; P.nfree += en[k]; }
    for (int k = 0; k < 3; k++) if (en[k] && 0.5 * tol[k] > P.ha0) P.ha0 = 0.5 * tol[k];
    for (int k = 3; k < 6; k++) if (en[k] && 0.5 * tol[k] > P.hs0) P.hs0 = 0.5 * tol[k];
    const double steptol = cc->step_tolerance > 0 ? cc->step_tolerance : 0.01;
    P.T = cc->max_iterations;
    if (P.T <= 0) P.T = compass_iterations(P.ha0, P.hs0, steptol, 1);
    if (!P.nfree || !any_active) P.T = 0;
    return P;
}

// csp mode 4: every row's score for every defocus offset in one sweep (k_defocus), averaged per tilt on the host
static int csp_defocus_sweep(CspRun &c, const CspUnits &U, double *rows) {
    ppm_ref *ref = c.ref; const ppm_csp_cfg *cc = c.cc; const Geom &gm = c.gm; const int n_proj = c.n_proj;
    const double step = cc->defocus_step > 0 ? cc->defocus_step : 50.0;
    const int nt = ppm::defocus_steps(cc->defocus_range, step, PPM_MAX_DEFOCUS_STEPS);
    const int Tn = 2 * nt + 1;
    if (int rc = ref->csp.states.ensure(n_proj)) return rc;
    if (int rc = ref->csp.out.ensure((size_t)n_proj * Tn)) return rc;
    hipLaunchKernelGGL(k_states_from_rows, dim3((n_proj + 255) / 256), dim3(256), 0, cur_stream(), ref->spectra.rows.p, ref->csp.states.p, n_proj, gm.a, 1.0, 1.0);
    launch_defocus(cube_view(ref), gm, ref->samples.p, c.S_pad, ref->spectra.Il.p, ref->spectra.wring.p, ref->spectra.rows.p, ref->csp.states.p, n_proj, nt, (float)step,
                   nullptr, ref->csp.out.p, 0.f);
    HIPCHK(hipGetLastError());
    std::vector<double> sc((size_t)n_proj * Tn);
    HIPCHK(hipMemcpyAsync(sc.data(), ref->csp.out.p, sc.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    for (int u = 0; u < c.n_tilt; u++) {
        if (!U.refined[u]) continue;
        double best = -1e300; int bt = nt;
        for (int pass = 0; pass < 2; pass++)
            for (int t = (pass ? 0 : nt); t < (pass ? Tn : nt + 1); t++) {
                if (pass && t == nt) continue;
                double ssum = 0; int sn = 0;
                for (int j : U.urows[u]) if (U.usable[j]) { ssum += sc[(size_t)j * Tn + t]; sn++; }
                if (sn && ssum / sn > best) { best = ssum / sn; bt = t; }
            }
        for (int j : U.urows[u]) {
            double *row = rows + (size_t)j * PPM_NCOL;
            row[PPM_DF1] += (bt - nt) * step; row[PPM_DF2] += (bt - nt) * step;
            score_columns(sc[(size_t)j * Tn + bt], gm.r_lo, gm.r_hi, &row[PPM_SCORE], &row[PPM_SIGMA], &row[PPM_LOGP]);
        }
    }
    return 0;
}

// the units' state -> device and back (U.parts / U.tls through the staging vectors of the run); both wait for their copies
static int csp_upload_units(CspRun &c, const CspUnits &U) {
    ppm_ref *ref = c.ref;
    for (int i = 0; i < c.n_part; i++) { std::memcpy(&c.hN[(size_t)9 * i], U.parts[i].N, 9 * sizeof(double)); std::memcpy(&c.hp[(size_t)3 * i], U.parts[i].p, 3 * sizeof(double)); }
    for (int i = 0; i < c.n_tilt; i++) std::memcpy(&c.htl[(size_t)4 * i], U.tls[i].tl, 4 * sizeof(double));
    HIPCHK(hipMemcpyAsync(ref->csp.N.p, c.hN.data(), c.hN.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.p.p, c.hp.data(), c.hp.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.tl.p, c.htl.data(), c.htl.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}
static int csp_download_units(CspRun &c, CspUnits &U) {
    ppm_ref *ref = c.ref;
    HIPCHK(hipMemcpyAsync(c.hN.data(), ref->csp.N.p, c.hN.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(c.hp.data(), ref->csp.p.p, c.hp.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(c.htl.data(), ref->csp.tl.p, c.htl.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    for (int i = 0; i < c.n_part; i++) { std::memcpy(U.parts[i].N, &c.hN[(size_t)9 * i], 9 * sizeof(double)); std::memcpy(U.parts[i].p, &c.hp[(size_t)3 * i], 3 * sizeof(double)); }
    for (int i = 0; i < c.n_tilt; i++) std::memcpy(U.tls[i].tl, &c.htl[(size_t)4 * i], 4 * sizeof(double));
    return 0;
}

// static tables of the search on the device, the evaluation parameters (c.EP) and the units' start state
static int csp_upload_tables(CspRun &c, CspUnits &U, int ncand_max) {
    ppm_ref *ref = c.ref; const Geom &gm = c.gm; const int n_proj = c.n_proj, n_part = c.n_part, n_tilt = c.n_tilt, n_slots = U.n_slots;
    CspWs &w = ref->csp;
    // Every ensure of a buffer c.EP names happens HERE, ahead of its filling below, and nowhere later in the call (out and eval are sized
    // for the search and the final scores alike); samples, spectra.Il and spectra.cw were ensured by csp_prepare_spectra.  What later stages
    // grow (csp.active, csp.states, csp.search.*, the compass state) is read from its DevBuf where it is used.
    if (int rc = w.rp.ensure(n_proj)) return rc;
    if (int rc = w.rt.ensure(n_proj)) return rc;
    if (int rc = w.slot.ensure(U.nu_all)) return rc;
    if (int rc = w.s0.ensure((size_t)2 * n_proj)) return rc;
    if (int rc = w.g0.ensure((size_t)2 * n_proj)) return rc;
    if (int rc = w.N.ensure((size_t)9 * n_part)) return rc;
    if (int rc = w.p.ensure((size_t)3 * n_part)) return rc;
    if (int rc = w.tl.ensure((size_t)4 * n_tilt)) return rc;
    if (ncand_max > kMaxCand) return fail(-22, "csp: too many free parameters");
    if (int rc = w.delta.ensure((size_t)std::max(n_slots, 1) * ncand_max * 6)) return rc;
    if (int rc = w.eval.ensure(std::max(U.eval_rows.size(), U.final_rows.size()))) return rc;
    if (int rc = w.out.ensure(std::max(U.eval_rows.size() * ncand_max, U.final_rows.size()))) return rc;
    if (int rc = w.uoff.ensure(U.active.size() + 1)) return rc;
    if (int rc = w.mean.ensure(std::max<size_t>(U.active.size() * ncand_max, 1))) return rc;
    HIPCHK(hipMemcpyAsync(w.rp.p, U.row_part.data(), n_proj * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(w.rt.p, U.row_tilt.data(), n_proj * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(w.slot.p, U.unit_slot.data(), U.nu_all * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(w.s0.p, U.s0.data(), U.s0.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(w.g0.p, U.g0.data(), U.g0.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    c.hN.resize((size_t)9 * n_part); c.hp.resize((size_t)3 * n_part); c.htl.resize((size_t)4 * n_tilt);
    CspEvalP &EP = c.EP;
    EP.cv = cube_view(ref);
    EP.samples = ref->samples.p; EP.Il = ref->spectra.Il.p; EP.cw = ref->spectra.cw.p; EP.S_pad = c.S_pad; EP.N = gm.N; EP.nr = c.nrings;
    EP.tabR = cube_tab_radius(gm.B, EP.cv.scale);
    c.tab = local_tables_wanted(EP.tabR) && tables_fit_lds(ring_lds_bytes8(4, kMaxCand, c.nrings), EP.tabR);
    EP.rlo2 = (float)(gm.r_lo * gm.r_lo); EP.ring_signed = (float)std::min(gm.ring_signed, 1e30);
    EP.kind = c.kind; EP.eval_rows = w.eval.p; EP.row_part = w.rp.p; EP.row_tilt = w.rt.p; EP.unit_slot = w.slot.p;
    EP.Nmat = w.N.p; EP.pshift = w.p.p; EP.tl = w.tl.p; EP.delta = w.delta.p; EP.s0 = w.s0.p; EP.g0 = w.g0.p; EP.out = w.out.p;
    // evaluation list of the search (the usable rows of the active units, grouped by unit) and the units' offsets in it: uploaded once
    U.uoff.assign(U.active.size() + 1, 0);
    for (size_t a = 0; a < U.active.size(); a++) { int n = 0; for (int j : U.urows[U.active[a]]) n += U.usable[j] ? 1 : 0; U.uoff[a + 1] = U.uoff[a] + n; }
    HIPCHK(hipMemcpyAsync(w.uoff.p, U.uoff.data(), U.uoff.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    return csp_upload_units(c, U);
}

// one block of 256 threads per evaluation row
static void launch_csp_eval(const CspRun &c, size_t n_rows) {
    ProfScope ps(PPM_K_LOCAL);
    const size_t lds = ring_lds_bytes8(4, kMaxCand, c.nrings) + (c.tab ? cube_tab_bytes(c.EP.tabR) : 0);
    if (c.tab) hipLaunchKernelGGL(k_csp_eval<true>, dim3((unsigned)n_rows), dim3(256), lds, cur_stream(), c.EP);
    else hipLaunchKernelGGL(k_csp_eval<false>, dim3((unsigned)n_rows), dim3(256), lds, cur_stream(), c.EP);
}

// The compass search: state and decisions on the device (ppm_csp_kernels.h), the iterations enqueued back to back — six launches
// each (candidates, unit means, trial step, its score, its means, accept) and no host wait until the units come back at the end.
// The bands follow from the step schedule alone, so the host knows them up front.
static int csp_compass(CspRun &c, CspUnits &U, const CspSearch &P, int ncand_max) {
    ppm_ref *ref = c.ref; const Geom &gm = c.gm; CspEvalP &EP = c.EP; CspWs &w = ref->csp;
    const int na = (int)U.active.size(); const size_t n_slots = (size_t)std::max(U.n_slots, 1);
    if (int rc = ref->compass.ensure(n_slots)) return rc;       // delta_t has a row per slot, the rest per active unit: slots >= active units
    if (int rc = w.active.ensure((size_t)na)) return rc;
    HIPCHK(hipMemcpyAsync(w.active.p, U.active.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(w.eval.p, U.eval_rows.data(), U.eval_rows.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemsetAsync(w.delta.p, 0, n_slots * ncand_max * 6 * sizeof(double), cur_stream()));      // slots of units without usable rows stay zero
    HIPCHK(hipMemsetAsync(ref->compass.delta_t.p, 0, n_slots * 6 * sizeof(double), cur_stream()));
    HIPCHK(hipMemsetAsync(ref->compass.acc.p, 0, (size_t)na * 6 * sizeof(double), cur_stream()));
    CompassPoses at;
    at.kind = c.kind; at.n_active = na; at.Nmat = w.N.p; at.nstride = 9; at.pshift = w.p.p; at.pstride = 3; at.tl = w.tl.p;
    at.active = w.active.p; at.unit_slot = w.slot.p; at.delta = w.delta.p; at.mean = w.mean.p;
    int nrot_c = 0;         // accounting: gathers = samples x rotations that differ (shift candidates share the centre's)
    for (int i = 0; i < 3; i++) nrot_c += P.en[i] ? 2 : 0;
    const bool any_ang = P.en[0] || P.en[1] || P.en[2], any_sh = P.en[3] || P.en[4] || P.en[5];
    if (int rc = compass_enqueue(ref->compass, at, P.en, P.tol, P.T, P.ha0, P.hs0,
            [&](double ha, double hs) { return march_band(c.bf(), gm.N, c.rm_px, ha, hs, any_ang, any_sh, gm.r_hi); },
            [&](const double *delta, int nc, double rband, double *means) {
                EP.delta = delta; EP.ncand = nc; EP.S_used = c.prefix_of(rband); EP.rmax2 = (float)(rband * rband);
                c.acct_gathers += (double)U.eval_rows.size() * EP.S_used * (nc > 1 ? 1 + nrot_c : 1); c.acct_sweeps++;
                launch_csp_eval(c, U.eval_rows.size());
                const int nm = na * nc;
                hipLaunchKernelGGL(k_csp_unit_means, dim3((nm + 255) / 256), dim3(256), 0, cur_stream(), w.out.p, w.uoff.p, na, nc, means);
                return 0;
            })) return rc;
    EP.delta = w.delta.p;
    return csp_download_units(c, U);        // the units as the search left them
}

// ---- exhaustive particle search (ppm_csp_cfg.search_points; the plan: ppm_csp_search.h)
constexpr size_t kCspSearchTableBytes = (size_t)256 << 20;      // per-rotation maxima of one particle chunk (score + shift index = 8 bytes per rotation)
constexpr int kCspSearchRotsPerLaunch = 1 << 16;                // rotations one k_csp_global launch takes (PPM_CSP_SEARCH_ROTS lowers it)

// Stage 1: every grid point of every active particle scored on the coarse band (k_csp_global), the K best rotations of each with their
// best shifts (k_csp_global_topk) -> the handle's candidate tables, [active unit][K]
static int csp_global_rank(CspRun &c, const CspUnits &U, const ppm_csp_search_info &G) {
    ppm_ref *ref = c.ref; const Geom &gm = c.gm;
    const int na = (int)U.active.size(), K = G.n_candidates;
    const size_t n_eval = U.eval_rows.size();
    std::vector<double> &rowtab = c.rowtab;
    rowtab.resize(n_eval * kCspRowTab);
    for (size_t e = 0; e < n_eval; e++) {
        const int j = U.eval_rows[e], it = U.row_tilt[j];
        const TiltRot &r = U.trot[it]; const CUnit &tu = U.tls[it];
        double *t = &rowtab[e * kCspRowTab], A[9];
        mat_mul3(r.a, r.b, t); mat_mul3(r.ai, r.bi, A);
        std::memcpy(t + 9, A, 6 * sizeof(double));
        t[15] = U.s0[2 * j] - U.g0[2 * j] + tu.tl[2]; t[16] = U.s0[2 * j + 1] - U.g0[2 * j + 1] + tu.tl[3];
    }
    if (int rc = ref->csp.search.rowtab.ensure(rowtab.size())) return rc;
    if (int rc = ref->csp.active.ensure((size_t)na)) return rc;
    HIPCHK(hipMemcpyAsync(ref->csp.search.rowtab.p, rowtab.data(), rowtab.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.active.p, U.active.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.eval.p, U.eval_rows.data(), n_eval * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    const size_t n_rot = (size_t)G.n_rot;
    const int chunk = (int)std::min<size_t>(std::min<size_t>((size_t)na, 65535), std::max<size_t>(1, kCspSearchTableBytes / (n_rot * 8)));
    if (int rc = ref->csp.search.gbest.ensure((size_t)chunk * n_rot)) return rc;
    if (int rc = ref->csp.search.gshift.ensure((size_t)chunk * n_rot)) return rc;
    if (int rc = ref->csp.search.crot.ensure((size_t)na * K)) return rc;
    if (int rc = ref->csp.search.cshift.ensure((size_t)na * K)) return rc;
    if (int rc = ref->csp.search.cscore.ensure((size_t)na * K)) return rc;
    long cap = kCspSearchRotsPerLaunch;
    if (const char *e = std::getenv("PPM_CSP_SEARCH_ROTS")) { long v = std::atol(e); if (v > 0) cap = std::min(cap, v); }   // tests: force several launches
    CspGlobalP GP;
    GP.cv = c.EP.cv; GP.samples = ref->samples.p; GP.Il = ref->spectra.Il.p; GP.cw = ref->spectra.cw.p; GP.S_pad = c.S_pad; GP.N = gm.N;
    GP.rlo2 = c.EP.rlo2; GP.ring_signed = c.EP.ring_signed; GP.S_used = c.prefix_of(G.r_g); GP.rmax2 = (float)(G.r_g * G.r_g);
    GP.eval_rows = ref->csp.eval.p; GP.uoff = ref->csp.uoff.p; GP.active = ref->csp.active.p; GP.Nmat = ref->csp.N.p; GP.pshift = ref->csp.p.p;
    GP.rowtab = ref->csp.search.rowtab.p; GP.G = G; GP.best = ref->csp.search.gbest.p; GP.best_shift = ref->csp.search.gshift.p;
    GP.edge_ring = (int)std::floor(G.r_g); GP.max_rows = 1;
    for (int u : U.active) { int n = 0; for (int j : U.urows[u]) n += U.usable[j] ? 1 : 0; GP.max_rows = std::max(GP.max_rows, n); }
    const size_t lds = csp_global_lds_bytes(GP.S_used, GP.max_rows);
    if (lds + 256 > (size_t)64 * 1024) return fail(-22, "csp: the coarse band of the exhaustive search does not fit the LDS");
    for (int a0 = 0; a0 < na; a0 += chunk) {
        const int npc = std::min(chunk, na - a0);
        GP.a0 = a0;
        for (long r0 = 0; r0 < G.n_rot; r0 += cap) {
            GP.rot0 = r0; GP.nrot = (int)std::min<long>(cap, G.n_rot - r0);
            GP.rc = (int)std::min<long>(64, std::max<long>(1, (long)GP.nrot * npc / 8192));
            ProfScope ps(PPM_K_GLOBAL);
            hipLaunchKernelGGL(k_csp_global, dim3((unsigned)((GP.nrot + GP.rc - 1) / GP.rc), (unsigned)npc), dim3(64), lds, cur_stream(), GP);
        }
        hipLaunchKernelGGL(k_csp_global_topk, dim3((unsigned)npc), dim3(256), 0, cur_stream(), ref->csp.search.gbest.p, ref->csp.search.gshift.p, (long)G.n_rot, K,
                           ref->csp.search.crot.p + (size_t)a0 * K, ref->csp.search.cshift.p + (size_t)a0 * K, ref->csp.search.cscore.p + (size_t)a0 * K);
        HIPCHK(hipGetLastError());
    }
    const long passes = (G.n_shift + 64 * kCspGlobalShifts - 1) / (64 * kCspGlobalShifts);
    c.acct_gathers += (double)n_eval * (double)G.n_rot * GP.S_used * (double)passes;
    ref->csp.search.cand_K = K;
    ref->csp.search.cand_unit.resize(na); ref->csp.search.cand_rot.resize((size_t)na * K); ref->csp.search.cand_shift.resize((size_t)na * K); ref->csp.search.cand_score.resize((size_t)na * K);
    HIPCHK(hipMemcpyAsync(ref->csp.search.cand_rot.data(), ref->csp.search.crot.p, (size_t)na * K * sizeof(long), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.search.cand_shift.data(), ref->csp.search.cshift.p, (size_t)na * K * sizeof(int), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.search.cand_score.data(), ref->csp.search.cscore.p, (size_t)na * K * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

// mean score of every active unit at its current state on the band `rband` (zero displacement) -> hmean[active unit]
static int csp_unit_scores(CspRun &c, const CspUnits &U, int ncand_max, double rband, std::vector<double> &hmean) {
    ppm_ref *ref = c.ref; CspEvalP &EP = c.EP; const int na = (int)U.active.size();
    HIPCHK(hipMemsetAsync(ref->csp.delta.p, 0, (size_t)std::max(U.n_slots, 1) * ncand_max * 6 * sizeof(double), cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.eval.p, U.eval_rows.data(), U.eval_rows.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    EP.delta = ref->csp.delta.p; EP.ncand = 1; EP.S_used = c.prefix_of(rband); EP.rmax2 = (float)(rband * rband);
    c.acct_gathers += (double)U.eval_rows.size() * EP.S_used; c.acct_sweeps++;
    launch_csp_eval(c, U.eval_rows.size());
    hipLaunchKernelGGL(k_csp_unit_means, dim3((na + 255) / 256), dim3(256), 0, cur_stream(), ref->csp.out.p, ref->csp.uoff.p, na, 1, ref->csp.mean.p);
    HIPCHK(hipGetLastError());
    hmean.resize(na);
    HIPCHK(hipMemcpyAsync(hmean.data(), ref->csp.mean.p, (size_t)na * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

// The exhaustive search of the active particles: stage 1 ranks the grid; stage 2 gives the k-th candidate of every particle two compass
// iterations (first steps D / 2 and h_s / 2, bounds +-D / +-h_s about the candidate) and scores it at the band that pass ended on, the
// best pass of a particle wins (ties to the lower k); stage 3 is the compass search of the winners from D / 4 and h_s / 4 down to the
// step tolerance, bounded by +-D / 2 and +-h_s / 2.  csp_compass serves both as it is.
static int csp_exhaustive(CspRun &c, CspUnits &U, const CspSearch &P, const ppm_csp_search_info &G, int ncand_max) {
    const ppm_csp_cfg *cc = c.cc; const Geom &gm = c.gm;
    if (int rc = csp_global_rank(c, U, G)) return rc;
    ppm_ref *ref = c.ref;
    const int na = (int)U.active.size(), K = G.n_candidates;
    for (int a = 0; a < na; a++) ref->csp.search.cand_unit[a] = (long)c.particles_in[(size_t)U.active[a] * PPM_NPCOL];
    const double hs_grid = G.shift_grid ? G.h_s : cc->tol_shift;
    const bool any_ang = P.en[0] || P.en[1] || P.en[2], any_sh = P.en[3] || P.en[4] || P.en[5];
    CspSearch P2 = P;
    for (int k = 0; k < 3; k++) { P2.tol[k] = G.step; P2.tol[3 + k] = hs_grid; }
    P2.ha0 = any_ang ? 0.5 * G.step : 0; P2.hs0 = any_sh ? 0.5 * hs_grid : 0; P2.T = 2;
    const double band2 = march_band(c.bf(), gm.N, c.rm_px, 0.5 * P2.ha0, 0.5 * P2.hs0, any_ang, any_sh, gm.r_hi);      // of the second iteration
    const std::vector<CUnit> start = U.parts;
    std::vector<CUnit> win(na); std::vector<double> fbest(na, -1e300), hmean;
    for (int k = 0; k < K; k++) {
        for (int a = 0; a < na; a++) {
            CUnit q = start[U.active[a]];
            const long rot = ref->csp.search.cand_rot[(size_t)a * K + k];
            if (rot >= 0) { double d[6]; csp_search_delta(G, rot, ref->csp.search.cand_shift[(size_t)a * K + k], d); unit_apply_delta(q.N, q.p, d); }
            U.parts[U.active[a]] = q;
        }
        if (int rc = csp_upload_units(c, U)) return rc;
        if (int rc = csp_compass(c, U, P2, ncand_max)) return rc;
        if (int rc = csp_unit_scores(c, U, ncand_max, band2, hmean)) return rc;
        for (int a = 0; a < na; a++) if (hmean[a] > fbest[a]) { fbest[a] = hmean[a]; win[a] = U.parts[U.active[a]]; }
    }
    for (int a = 0; a < na; a++) U.parts[U.active[a]] = win[a];
    if (int rc = csp_upload_units(c, U)) return rc;
    CspSearch P3 = P;
    for (int k = 0; k < 3; k++) { P3.tol[k] = 0.5 * G.step; P3.tol[3 + k] = 0.5 * hs_grid; }
    P3.ha0 = 0.5 * P2.ha0; P3.hs0 = 0.5 * P2.hs0;
    const double steptol = cc->step_tolerance > 0 ? cc->step_tolerance : 0.01;
    P3.T = cc->max_iterations > 0 ? cc->max_iterations : compass_iterations(P3.ha0, P3.hs0, steptol, 1);
    return csp_compass(c, U, P3, ncand_max);
}

// scores of every row of the refined units at the full band, at the units' current state (zero displacement) -> hout[final row]
static int csp_final_scores(CspRun &c, const CspUnits &U, std::vector<double> &hout) {
    ppm_ref *ref = c.ref; const Geom &gm = c.gm; CspEvalP &EP = c.EP;
    HIPCHK(hipMemsetAsync(ref->csp.delta.p, 0, (size_t)U.n_slots * 6 * sizeof(double), cur_stream()));
    HIPCHK(hipMemcpyAsync(ref->csp.eval.p, U.final_rows.data(), U.final_rows.size() * sizeof(int), hipMemcpyHostToDevice, cur_stream()));
    EP.ncand = 1; EP.S_used = c.prefix_of(gm.r_hi); EP.rmax2 = (float)(gm.r_hi * gm.r_hi);
    c.acct_gathers += (double)U.final_rows.size() * EP.S_used; c.acct_sweeps++;
    launch_csp_eval(c, U.final_rows.size());
    HIPCHK(hipGetLastError());
    hout.resize(U.final_rows.size());
    HIPCHK(hipMemcpyAsync(hout.data(), ref->csp.out.p, hout.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

// the refined units -> particles / tilts, and every row of theirs: pose, shifts and the score columns
static void csp_write_back(const CspRun &c, CspUnits &U, const std::vector<double> &hout, double *rows, double *particles, double *tilts) {
    const Geom &gm = c.gm; const int kind = c.kind;
    std::vector<double> row_score(c.n_proj, 0.0);
    for (size_t q = 0; q < U.final_rows.size(); q++) row_score[U.final_rows[q]] = hout[q];
    for (int i = 0; i < c.n_tilt; i++) tilt_rotations(U.tls[i].tl[0], U.tls[i].tl[1], U.trot[i]);       // the tilts may have moved
    const std::vector<CUnit> &units = kind == PPM_CSP_PARTICLES ? U.parts : U.tls;
    for (int u = 0; u < U.nu_all; u++) {
        if (!U.refined[u]) continue;
        if (kind == PPM_CSP_PARTICLES) {
            double *P = particles + (size_t)u * PPM_NPCOL, a1, a2, a3;
            angles_from_matrix(units[u].N, a1, a2, a3);
            P[4] = -a1; P[5] = -a2; P[6] = -a3; P[1] = units[u].p[0]; P[2] = units[u].p[1]; P[3] = units[u].p[2];
        } else {
            double *Tt = tilts + (size_t)u * PPM_NTCOL;
            Tt[4] = units[u].tl[0]; Tt[5] = units[u].tl[1]; Tt[2] = units[u].tl[2]; Tt[3] = units[u].tl[3];
        }
        double ssum = 0; int sn = 0;
        for (int j : U.urows[u]) {
            double *row = rows + (size_t)j * PPM_NCOL, M[9], gq[2];
            const CUnit &pu = U.parts[U.row_part[j]], &tu = U.tls[U.row_tilt[j]];
            csp_row_pose(pu.N, pu.p, U.trot[U.row_tilt[j]], tu.tl[2], tu.tl[3], M, gq);
            angles_from_matrix(M, row[PPM_PSI], row[PPM_THETA], row[PPM_PHI]);
            row[PPM_XSHIFT] = (U.s0[2 * j] + gq[0] - U.g0[2 * j]) * gm.a; row[PPM_YSHIFT] = (U.s0[2 * j + 1] + gq[1] - U.g0[2 * j + 1]) * gm.a;
            score_columns(row_score[j], gm.r_lo, gm.r_hi, &row[PPM_SCORE], &row[PPM_SIGMA], &row[PPM_LOGP]);
            if (U.usable[j]) { ssum += row[PPM_SCORE]; sn++; }
        }
        if (kind == PPM_CSP_PARTICLES) particles[(size_t)u * PPM_NPCOL + 10] = sn ? ssum / sn : -1.0;
    }
}

extern "C" int ppm_csp_refine(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const ppm_csp_cfg *cc, const void *images, int images_on_device,
                              int n_proj, double *rows, double *particles, int n_part, double *tilts, int n_tilt) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!ref || !cfg || !cc || !images || !rows || !particles || !tilts) return fail(-22, "null argument");
    StreamScope ss_(ref->stream, ref->copy);
    if (cc->unit != PPM_CSP_PARTICLES && cc->unit != PPM_CSP_MICROGRAPHS) return fail(-22, "csp: unit must be particles (1) or micrographs (2)");
    if (cc->search_points < 0 || cc->search_candidates < 0) return fail(-22, "csp: search_points and search_candidates must not be negative");
    if (n_proj <= 0) return 0;
    if (n_part <= 0 || n_tilt <= 0) return fail(-22, "csp: the extended parameters hold no particles or no tilts");
    ref->csp.search.cand_K = 0; ref->csp.search.cand_unit.clear();       // ppm_csp_search_candidates answers from the last call
    CspRun c; c.particles_in = particles; c.ref = ref; c.cfg = cfg; c.cc = cc; c.kind = cc->unit; c.n_proj = n_proj; c.n_part = n_part; c.n_tilt = n_tilt;
    const Geom &gm = c.gm;
    ppm_refine_cfg c2 = *cfg; c2.global_search = 0;
    std::string err;
    if (!geom_init(c.gm, c2, err)) return fail(-22, err);
    if (gm.N != ref->N) return fail(-22, "particle box differs from the reference box");
    if (gm.B > (ref->B + 1) / ref->pad - 1) return fail(-22, "high-resolution limit exceeds the band the reference was prepared for");
    const Trace trace_("ppm_csp_refine");
    c.rm_px = cfg->mask_radius / gm.a;
    build_samples(gm, c.sl);
    c.S_pad = (int)c.sl.packed.size(); c.nrings = gm.B + 2;
    const bool mode4 = cc->refine_defocus != 0;
    if (mode4 && c.kind != PPM_CSP_MICROGRAPHS) return fail(-22, "csp: defocus refinement works on tilts (unit = micrographs)");
    CspUnits U; std::vector<double> hout;
    DrainOnError drain;             // below c, U and hout: what the asynchronous copies of this call read and write outlives the drain
    drain.armed = true;
    if (int rc = csp_prepare_spectra(c, images, images_on_device, rows, mode4)) return rc;
    if (int rc = csp_build_units(c, rows, particles, tilts, U)) return rc;
    if (U.final_rows.empty()) return 0;         // (still armed: the copy of the caller's rows may be in flight)
    const CspSearch P = csp_search_plan(cc, c.kind, !U.active.empty());
    trace_.mark("host tables");
    if (mode4) { if (int rc = csp_defocus_sweep(c, U, rows)) return rc; return drain.ok(); }
    const int ncand_max = 1 + 2 * P.nfree;
    if (int rc = csp_upload_tables(c, U, ncand_max)) return rc;
    trace_.mark("spectra prepared, units uploaded");
    // the exhaustive stage: particles only, and only where the compass search itself has something to do
    ppm_csp_search_info G = csp_search_from_cfg(*cfg, *cc, gm);
    if (cc->search_points > 0 && c.kind == PPM_CSP_PARTICLES && P.T > 0) {
        char b[320];
        if (G.active)
            std::snprintf(b, sizeof(b), "csp: exhaustive search of %ld x %ld grid points per particle (step %g degrees, band %.2f Fourier pixels, %d x %d x %d "
                          "rotations x %d^3 shifts within a budget of %d), %d candidates each refined", G.n_rot, G.n_shift, G.step, G.r_g, G.n_angle[0], G.n_angle[1],
                          G.n_angle[2], G.n_shift_axis, cc->search_points, G.n_candidates);
        else
            std::snprintf(b, sizeof(b), "csp: search_points = %d is below the %ld rotations of the 30 degree grid: no exhaustive search, the compass search "
                          "starts from the given poses", cc->search_points, G.n_rot);
        ref->note = b;
    }
    if (P.T <= 0) G.active = 0;
    if (G.active) { if (int rc = csp_exhaustive(c, U, P, G, ncand_max)) return rc; }
    else if (P.T > 0) if (int rc = csp_compass(c, U, P, ncand_max)) return rc;
    trace_.mark("searched");
    if (int rc = csp_final_scores(c, U, hout)) return rc;
    trace_.mark("final scores");
    csp_write_back(c, U, hout, rows, particles, tilts);
    // ppm_refine_last_counts after a constrained refinement: 0, sweeps (k_csp_eval launches), in-band samples of the full band, gathered
    // samples per projection summed over the sweeps
    ref->last_counts[0] = G.active ? G.n_rot * G.n_shift : 0; ref->last_counts[1] = c.acct_sweeps; ref->last_counts[2] = (long)std::floor(kPi * gm.r_hi * gm.r_hi / 2);
    ref->last_counts[3] = (long)(c.acct_gathers / std::max(n_proj, 1));
    return drain.ok();
}

extern "C" int ppm_csp_search_plan(const ppm_refine_cfg *cfg, const ppm_csp_cfg *cc, ppm_csp_search_info *out) {
    if (!cfg || !cc || !out) return fail(-22, "null argument");
    if (cc->search_points < 0 || cc->search_candidates < 0) return fail(-22, "csp: search_points and search_candidates must not be negative");
    Geom gm; ppm_refine_cfg c2 = *cfg; c2.global_search = 0;
    std::string err;
    if (!geom_init(gm, c2, err)) return fail(-22, err);
    *out = csp_search_from_cfg(*cfg, *cc, gm);
    return 0;
}

extern "C" int ppm_csp_search_candidates(ppm_ref_t *ref, long unit, int max_k, long *rot_index, long *shift_index, double *score) {
    if (!ref || max_k < 0 || (max_k > 0 && (!rot_index || !shift_index || !score))) return fail(-22, "null argument");
    for (size_t a = 0; a < ref->csp.search.cand_unit.size(); a++) {
        if (ref->csp.search.cand_unit[a] != unit) continue;
        const int K = std::min(max_k, ref->csp.search.cand_K);
        int n = 0;
        for (int k = 0; k < K; k++) {
            const size_t o = a * ref->csp.search.cand_K + k;
            if (ref->csp.search.cand_rot[o] < 0) break;
            rot_index[n] = ref->csp.search.cand_rot[o]; shift_index[n] = ref->csp.search.cand_shift[o]; score[n] = 100.0 * (double)ref->csp.search.cand_score[o]; n++;
        }
        return n;
    }
    return 0;
}

