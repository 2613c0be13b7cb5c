// ppm_csp_kernels.h — constrained (tilt-series) scoring kernel of libpypmatch (gfx950).
//
// A projection row's pose follows from its particle's 3-D pose and its tilt's geometry (include/ppm.h, ppm_csp_cfg; the
// relation restates csp_euler_angles, src/pyp/analysis/geometry/core.py:1081-1213).  The optimiser's state lives on the device
// (round 5): a compass iteration is a fixed sequence of launches — score the candidates (k_csp_eval), average per unit
// (k_csp_unit_means), parabolic trial step (k_csp_step_trial), score it, average, accept and lay out the next iteration's candidates
// (k_csp_step_accept) — and the host (ppm_csp_refine in ppm_lib.hip) enqueues all iterations without waiting in between; the rows of a
// unit are averaged in a fixed order, so results do not depend on the launch shape.
#pragma once
#include "ppm_kernels2.h"
#include "ppm_csp_search.h"

namespace ppm {

struct CspEvalP {
    CubeView cv; const uint32_t *samples; const float2 *Il; const float *cw;
    int S_pad, N, nr; float rlo2, ring_signed;
    int tabR;                             // radius of the LDS address tables (k_csp_eval<true>)
    int S_used; float rmax2;              // band of this sweep (frequency marching)
    int kind, ncand;                      // PPM_CSP_PARTICLES / PPM_CSP_MICROGRAPHS; candidates per unit (<= kMaxCand)
    const int *eval_rows;                 // [grid] row evaluated by each block
    const int *row_part, *row_tilt;       // [n_proj] unit indices of a row
    const int *unit_slot;                 // [n_part] or [n_tilt]: position of the unit in `delta` (-1: not refined)
    const double *Nmat;                   // [n_part][9] particle orientation E(-ppsi, -ptheta, -pphi)
    const double *pshift;                 // [n_part][3] particle shift, pixels
    const double *tl;                     // [n_tilt][4] tilt angle, tilt-axis angle, shift x, shift y
    const double *delta;                  // [n_units][ncand][6] displacement of every candidate
    const double *s0, *g0;                // [n_proj][2] row shift (pixels) and geometric shift at the start
    double *out;                          // [grid][ncand] scores
};

// Block = one projection row, 256 threads: thread q < ncand derives candidate q's row pose in double precision; the
// candidates that keep the unit's rotation share one gather group (shift variants), every rotated candidate is a group
// of its own; one sweep (sweep_plan) scores them all.
template <bool TAB>
__global__ void __launch_bounds__(256, 4) k_csp_eval(CspEvalP P) {
    __shared__ SweepPlan plan;
    extern __shared__ float lsm[];
    __shared__ double score[kMaxCand];
    __shared__ float cm[kMaxCand][6], csh[kMaxCand][2];
    __shared__ int csame[kMaxCand], cslot[kMaxCand];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6, nr = P.nr;
    const int j = P.eval_rows[blockIdx.x], ip = P.row_part[j], it = P.row_tilt[j];
    const int ncand = P.ncand;
    if (tid < ncand) {
        const int unit = P.kind == PPM_CSP_PARTICLES ? ip : it;
        const double *d = P.delta + ((size_t)P.unit_slot[unit] * ncand + tid) * 6;
        double N[9], p[3], tl[4], M[9], g[2];
#pragma unroll
        for (int k = 0; k < 9; k++) N[k] = P.Nmat[(size_t)ip * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = P.pshift[(size_t)ip * 3 + k];
#pragma unroll
        for (int k = 0; k < 4; k++) tl[k] = P.tl[(size_t)it * 4 + k];
        int same;
        if (P.kind == PPM_CSP_PARTICLES) {
            same = d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0;
            unit_apply_delta(N, p, d);
        } else {
            same = d[0] == 0.0 && d[1] == 0.0;
            tl[0] += d[0]; tl[1] += d[1]; tl[2] += d[3]; tl[3] += d[4];
        }
        csp_row_pose(N, p, tl[0], tl[1], tl[2], tl[3], M, g);
        cm[tid][0] = (float)M[0]; cm[tid][1] = (float)M[1]; cm[tid][2] = (float)M[3]; cm[tid][3] = (float)M[4]; cm[tid][4] = (float)M[6]; cm[tid][5] = (float)M[7];
        csh[tid][0] = (float)(P.s0[2 * j] + g[0] - P.g0[2 * j]); csh[tid][1] = (float)(P.s0[2 * j + 1] + g[1] - P.g0[2 * j + 1]);
        csame[tid] = same;
    }
    __syncthreads();
    if (tid == 0) {
        int ng = 0, q = 0, first_same = -1;
        for (int c = 0; c < ncand; c++) if (csame[c]) { first_same = c; break; }
        if (first_same >= 0) {                     // group 0: the unit's own rotation with all its shift variants
            for (int k = 0; k < 6; k++) plan.m[0][k] = cm[first_same][k];
            plan.slot0[0] = 0;
            for (int c = 0; c < ncand; c++) if (csame[c]) { plan.sh[q][0] = csh[c][0]; plan.sh[q][1] = csh[c][1]; cslot[c] = q++; }
            plan.nv[0] = q; ng = 1;
        }
        for (int c = 0; c < ncand; c++) {
            if (csame[c]) continue;
            for (int k = 0; k < 6; k++) plan.m[ng][k] = cm[c][k];
            plan.slot0[ng] = q; plan.nv[ng] = 1; plan.sh[q][0] = csh[c][0]; plan.sh[q][1] = csh[c][1]; cslot[c] = q++; ng++;
        }
        plan.ng = ng; plan.nslots = q; plan.q_same = 0; plan.S_used = P.S_used; plan.rmax2 = P.rmax2;
    }
    __syncthreads();
    SweepCtx SC;
    SC.cv = P.cv; SC.samples = P.samples; SC.Il = P.Il + (size_t)j * P.S_pad; SC.cw = P.cw + (size_t)j * P.S_pad;
    SC.invN = 1.0f / (float)P.N; SC.rlo2 = P.rlo2; SC.ring_signed = P.ring_signed; SC.nr = nr; SC.nw = nw;
    SC.ringA = lsm; SC.sumB = lsm + kMaxCand * nw * nr; SC.sumC = SC.sumB + kMaxCand * nw; SC.score = score;
    if constexpr (TAB) SC.tab = cube_tab_fill(P.cv, (char *)lsm + ring_lds_bytes8(nw, kMaxCand, nr), P.tabR, tid, nthr);
    sweep_plan<TAB>(plan, SC, tid, nthr);
    if (tid < ncand) P.out[(size_t)blockIdx.x * ncand + tid] = score[cslot[tid]];
}

// Mean score of every (active unit, candidate) over the unit's evaluated rows: the rows of a unit are consecutive in the evaluation
// list (uoff[a] .. uoff[a + 1]) and are added in that order, like the host loop this replaces (2 MB of per-row scores per sweep
// stay on the device; 50 KB of means go back).
__global__ void k_csp_unit_means(const double *__restrict__ out, const int *__restrict__ uoff, int n_units, int ncand, double *__restrict__ mean) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_units * ncand) return;
    const int a = i / ncand, c = i - a * ncand, lo = uoff[a], hi = uoff[a + 1];
    double s = 0;
    for (int r = lo; r < hi; r++) s += out[(size_t)r * ncand + c];
    mean[i] = s / (double)(hi - lo);
}

// ---- the compass search's decisions, one thread per active unit (double precision): compass_trial / compass_accept of
// ppm_geom.h, the rule k_local applies as well.  Candidate 0 is the unit as it stands; then +h and -h for every enabled parameter in order.
struct CspStepP {
    int kind, n_active, ncand;
    const int *active;        // [n_active] index of the unit in the particle / tilt tables (null: the identity)
    const int *unit_slot;     // [n_units] row of the unit in the displacement tables (null: the identity)
    int en[6]; double tol[6];
    double ha, hs;            // steps of THIS iteration (degrees, pixels)
    double ha_next, hs_next;  // steps of the next one (k_csp_step_accept lays out its candidates)
    const double *mean;       // [n_active][ncand] unit means of the compass sweep
    const double *tmean;      // [n_active] unit means of the trial sweep
    double *acc;              // [n_active][6] displacement accumulated so far (bounded by +-tol)
    double *dtrial;           // [n_active][6] trial step
    double *fpm;              // [n_active][2][6] f(+h) of every parameter, then f(-h) (kNoProbe: outside the bounds)
    double *delta_c;          // [n_slots][ncand][6] candidates of the compass sweep
    double *delta_t;          // [n_slots][6] the trial step as k_csp_eval reads it
    double *Nmat, *pshift, *tl;   // unit state (k_csp_eval's tables; the sub-volume search keeps N and p in one row of 12)
    int nstride, pstride;         // doubles between two units' N / p (9 and 3 in k_csp_eval's tables, 12 and 12 in k_sva_eval's)
};
__device__ __forceinline__ int d_csp_unit(const CspStepP &P, int a) { return P.active ? P.active[a] : a; }
__device__ __forceinline__ int d_csp_slot(const CspStepP &P, int u) { return P.unit_slot ? P.unit_slot[u] : u; }

__device__ __forceinline__ void d_csp_layout_candidates(const CspStepP &P, int slot, double ha, double hs) {
    double *d = P.delta_c + (size_t)slot * P.ncand * 6;
    for (int k = 0; k < P.ncand * 6; k++) d[k] = 0.0;
    int c = 1;
    for (int i = 0; i < 6; i++) {
        if (!P.en[i]) continue;
        const double h = i < 3 ? ha : hs;
        d[(size_t)c * 6 + i] = h; d[(size_t)(c + 1) * 6 + i] = -h;
        c += 2;
    }
}

// candidates of the first iteration
__global__ void k_csp_step_init(CspStepP P) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= P.n_active) return;
    d_csp_layout_candidates(P, d_csp_slot(P, d_csp_unit(P, a)), P.ha_next, P.hs_next);
}

// after the compass sweep: the parabolic trial step of every unit
__global__ void k_csp_step_trial(CspStepP P) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= P.n_active) return;
    const double *mean = P.mean + (size_t)a * P.ncand;
    double *d = P.dtrial + (size_t)a * 6, *fpm = P.fpm + (size_t)a * 12;
    compass_trial<6>(mean[0], mean + 1, nullptr, P.en, P.ha, P.hs, P.acc + (size_t)a * 6, P.tol, d, fpm, fpm + 6);
    double *dt = P.delta_t + (size_t)d_csp_slot(P, d_csp_unit(P, a)) * 6;
    for (int i = 0; i < 6; i++) dt[i] = d[i];
}

// after the trial sweep: keep the trial step, the best single probe, or nothing; move the unit; lay out the next candidates
__global__ void k_csp_step_accept(CspStepP P) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= P.n_active) return;
    const int u = d_csp_unit(P, a);
    const double f0 = P.mean[(size_t)a * P.ncand], ft = P.tmean[a];
    const double *fpm = P.fpm + (size_t)a * 12, *dtr = P.dtrial + (size_t)a * 6;
    int bi, bs; double fb;
    const CompassMove mv = compass_accept<6>(f0, ft, fpm, fpm + 6, P.en, bi, bs, fb);
    double d[6] = { 0, 0, 0, 0, 0, 0 };
    if (mv == kCompassTrial) for (int i = 0; i < 6; i++) d[i] = dtr[i];
    else if (mv == kCompassProbe) d[bi] = bs * (bi < 3 ? P.ha : P.hs);
    if (mv != kCompassStay) {
        if (P.kind == PPM_CSP_PARTICLES) {
            unit_apply_delta(P.Nmat + (size_t)u * P.nstride, P.pshift + (size_t)u * P.pstride, d);
        } else {
            double *tl = P.tl + (size_t)u * 4;
            tl[0] += d[0]; tl[1] += d[1]; tl[2] += d[3]; tl[3] += d[4];
        }
        for (int k = 0; k < 6; k++) P.acc[(size_t)a * 6 + k] += d[k];
    }
    d_csp_layout_candidates(P, d_csp_slot(P, u), P.ha_next, P.hs_next);
}

// ---- exhaustive particle search, stage 1 (ppm_csp_cfg.search_points; the plan: ppm_csp_search.h).  Every (rotation, shift) grid point of a
// particle is scored on the coarse band r_g: the mean over the particle's usable rows of the K5 local score, the number k_csp_eval gives at
// that pose and band.  Kept per (particle, rotation): the best shift (ties to the lower shift index) and its score.
//
// Block = ONE wave: one particle and a run of `rc` rotations.  Per (rotation, row) the lanes first take SAMPLES: gather the slice, form
// X = al c I conj(slice) and the two power sums, write X to LDS.  Then the lanes take SHIFTS: each walks the ring-ordered samples out of
// LDS (every lane reads the same address: a broadcast), turns X by its shift's phase and keeps the ring sums of the current band of four
// rings (the list interleaves the 16-sample groups of four rings; a group's ring is wave-uniform), folded as signed or absolute values
// when the band ends.  A pass serves up to 256 shifts (four per lane); more shifts take further passes over the rows.  No atomics; every
// sum runs in list order, rows in eval_rows order, so a result depends neither on the launch shape nor on how the rotations are cut
// into launches.
// The edge ring: the prepared spectra carry ring weights (1 / sqrt of the ring's mean power) taken over the full band's rings, and the
// ring that holds r_g lies only partly inside the coarse band.  Its samples are re-weighted by the mean power of its in-band part (image
// value and CTF weight alike, once per row), which is how a refinement whose high-resolution limit is r_g prepares that ring: the score is
// that refinement's K5 score, the number the oracle gives with res_high at r_g, and no partial ring enters with a weight it did not earn.
constexpr int kCspRowTab = 17;        // doubles per evaluation row: Ta = Ry(-tilt) Rz(axis) [9], A = rows x, y of Rz(-axis) Ry(tilt) [6], s0 - g0 + tilt shift [2]
struct CspGlobalP {
    CubeView cv; const uint32_t *samples; const float2 *Il; const float *cw;
    int S_pad, N; float rlo2, ring_signed;
    int S_used; float rmax2;              // the coarse band
    int edge_ring, max_rows;              // floor(r_g); most rows of one particle (sizes the per-row LDS table)
    const int *eval_rows, *uoff, *active; // evaluation list, the active units' offsets in it, the active units
    const double *Nmat, *pshift;          // [n_part][9], [n_part][3]: the start poses
    const double *rowtab;                 // [n_eval][kCspRowTab]
    ppm_csp_search_info G;
    int a0;                               // first active unit of this particle chunk (blockIdx.y counts from it)
    long rot0; int nrot, rc;              // this launch: rotations rot0 .. rot0 + nrot, rc per block
    float *best; int *best_shift;         // [chunk particle][n_rot]: mean correlation of the best shift, its index
};
constexpr int kCspGlobalShifts = 4;       // shifts per lane and pass
__host__ __device__ inline size_t csp_global_lds_bytes(int S_used, int max_rows) { return (size_t)S_used * 16 + (size_t)(S_used / 16 + 1) * 4 + (size_t)max_rows * 4; }

__global__ void __launch_bounds__(64) k_csp_global(CspGlobalP P) {
    extern __shared__ float gsm[];
    float2 *const kxy = (float2 *)gsm, *const X = kxy + P.S_used;
    int *const gring = (int *)(X + P.S_used);
    float *const trow = (float *)(gring + (P.S_used / 16 + 1));
    __shared__ double Nc[9];
    __shared__ float m6[6];
    const int lane = threadIdx.x, S_used = P.S_used;
    const int a = P.a0 + blockIdx.y, u = P.active[a], e0 = P.uoff[a], e1 = P.uoff[a + 1];
    const ppm_csp_search_info &G = P.G;
    const long n_shift = G.n_shift;
    for (int s = lane; s < S_used; s += 64) {
        int kx, ky, al, ring;
        unpack_sample(P.samples[s], kx, ky, al, ring);
        kxy[s] = make_float2((float)kx, (float)ky);
        if ((s & 15) == 0) gring[s >> 4] = ring;
    }
    for (int e = e0; e < e1; e++) {         // the edge ring's weight of every row (see above): rotations do not change it
        const float2 *Il = P.Il + (size_t)P.eval_rows[e] * P.S_pad;
        float pw = 0.f, pc = 0.f;
        for (int s = lane; s < S_used; s += 64) {
            int kx, ky, al, ring;
            unpack_sample(P.samples[s], kx, ky, al, ring);
            if (ring != P.edge_ring || !((float)(kx * kx + ky * ky) < P.rmax2)) continue;
            const float2 iv = Il[s];
            pw += (float)al * (iv.x * iv.x + iv.y * iv.y); pc += (float)al;
        }
        pw = wave_sum(pw); pc = wave_sum(pc);
        if (lane == 0) trow[e - e0] = (pw > 0.f && pc > 0.f) ? 1.0f / sqrtf(pw / pc) : 1.0f;
    }
    const double p0 = P.pshift[(size_t)u * 3], p1 = P.pshift[(size_t)u * 3 + 1], p2 = P.pshift[(size_t)u * 3 + 2];
    const float invN = 1.0f / (float)P.N;
    CubeView one = P.cv; one.scale = 1.f;
    const long r_begin = P.rot0 + (long)blockIdx.x * P.rc, r_last = P.rot0 + (long)P.nrot, r_end = r_begin + P.rc < r_last ? r_begin + P.rc : r_last;
    for (long r = r_begin; r < r_end; r++) {
        __syncthreads();
        if (lane == 0) {            // the candidate's orientation N0 Rx(a) Ry(b) Rz(c), as unit_apply_delta composes it
            double N[9], R[9], d[6];
#pragma unroll
            for (int k = 0; k < 9; k++) N[k] = P.Nmat[(size_t)u * 9 + k];
            csp_search_delta(G, r, 0, d);
            if (d[0] != 0.0) { rot_xyz(0, d[0], R); mat_mul3(N, R, N); }
            if (d[1] != 0.0) { rot_xyz(1, d[1], R); mat_mul3(N, R, N); }
            if (d[2] != 0.0) { rot_xyz(2, d[2], R); mat_mul3(N, R, N); }
#pragma unroll
            for (int k = 0; k < 9; k++) Nc[k] = N[k];
        }
        double bestv = -1e300; int bestq = 0x7fffffff;
        for (long q0 = 0; q0 < n_shift; q0 += 64 * kCspGlobalShifts) {
            double msum[kCspGlobalShifts];
#pragma unroll
            for (int c = 0; c < kCspGlobalShifts; c++) msum[c] = 0.0;
            for (int e = e0; e < e1; e++) {
                const double *rt = P.rowtab + (size_t)e * kCspRowTab;
                __syncthreads();
                if (lane < 6) {     // M_row = Nc Ta: its first two columns, in double, then as k_csp_eval hands them to the sweep
                    const int i = lane >> 1, jc = lane & 1;
                    m6[lane] = (float)(Nc[i * 3] * rt[jc] + Nc[i * 3 + 1] * rt[3 + jc] + Nc[i * 3 + 2] * rt[6 + jc]) * P.cv.scale;
                }
                __syncthreads();
                // ---- lanes = samples
                const int j = P.eval_rows[e];
                const float2 *Il = P.Il + (size_t)j * P.S_pad; const float *cw = P.cw + (size_t)j * P.S_pad;
                const float ma = m6[0], mb = m6[1], mc = m6[2], md = m6[3], me = m6[4], mf = m6[5], te = trow[e - e0];
                float pB = 0.f, pC = 0.f;
                for (int s = lane; s < S_used; s += 64) {
                    int kx, ky, al, ring;
                    unpack_sample(P.samples[s], kx, ky, al, ring);
                    const float k2 = (float)(kx * kx + ky * ky);
                    if (!(k2 < P.rmax2 && k2 >= P.rlo2)) al = 0;
                    float2 iv = Il[s]; float c = cw[s];
                    if (ring == P.edge_ring) { iv.x *= te; iv.y *= te; c *= te; }
                    const float fal = (float)al, fkx = (float)kx, fky = (float)ky;
                    pC += fal * (iv.x * iv.x + iv.y * iv.y);
                    const float ac = fal * c, ax = ac * iv.x, ay = ac * iv.y, w = ac * c;
                    const float2 v = cube_interp(cube_fetch(one, ma * fkx + mb * fky, mc * fkx + md * fky, me * fkx + mf * fky));
                    pB += w * (v.x * v.x + v.y * v.y);
                    X[s] = make_float2(ax * v.x + ay * v.y, ay * v.x - ax * v.y);
                }
                const double sb = (double)wave_sum(pB), sc = (double)wave_sum(pC);
                const double inv = (sb > 0 && sc > 0) ? 1.0 / sqrt(sb * sc) : 0.0;
                __syncthreads();
                // ---- lanes = shifts
#pragma unroll
                for (int c = 0; c < kCspGlobalShifts; c++) {
                    if (q0 + c * 64 >= n_shift) continue;                           // wave-uniform
                    const long qq = q0 + c * 64 + lane, q = qq < n_shift ? qq : n_shift - 1;      // lanes beyond the grid repeat its last point; their sums are dropped
                    double d[6];
                    csp_search_delta(G, 0, q, d);
                    const double px = p0 + d[3], py = p1 + d[4], pz = p2 + d[5];
                    const float shx = (float)(rt[15] - (rt[9] * px + rt[10] * py + rt[11] * pz)), shy = (float)(rt[16] - (rt[12] * px + rt[13] * py + rt[14] * pz));
                    const float nx = -shx * invN, ny = -shy * invN;
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f; double sa = 0.0;
                    int band = 0;
                    auto fold = [&](int b, float v) { sa += ((float)b <= P.ring_signed) ? (double)v : fabs((double)v); };
                    for (int g = 0; g < (S_used >> 4); g++) {
                        const int ring = __builtin_amdgcn_readfirstlane(gring[g]);
                        if ((ring >> 2) != band) {
                            fold(4 * band, a0); fold(4 * band + 1, a1); fold(4 * band + 2, a2); fold(4 * band + 3, a3);
                            a0 = a1 = a2 = a3 = 0.f; band = ring >> 2;
                        }
                        float acc = 0.f;
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            const float2 k = kxy[g * 16 + i], x = X[g * 16 + i];
                            float rev = k.x * nx + k.y * ny;                        // phase in revolutions
                            rev -= floorf(rev);
                            acc += x.x * __cosf(6.283185307179586f * rev) + x.y * __sinf(6.283185307179586f * rev);
                        }
                        switch (ring & 3) { case 0: a0 += acc; break; case 1: a1 += acc; break; case 2: a2 += acc; break; default: a3 += acc; }
                    }
                    fold(4 * band, a0); fold(4 * band + 1, a1); fold(4 * band + 2, a2); fold(4 * band + 3, a3);
                    msum[c] += sa * inv;
                }
            }
#pragma unroll
            for (int c = 0; c < kCspGlobalShifts; c++) {
                const long q = q0 + c * 64 + lane;
                if (q < n_shift && msum[c] > bestv) { bestv = msum[c]; bestq = (int)q; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bestv, m, 64); const int oq = __shfl_xor(bestq, m, 64);
            if (ov > bestv || (ov == bestv && oq < bestq)) { bestv = ov; bestq = oq; }
        }
        if (lane == 0) {
            const size_t o = (size_t)blockIdx.y * (size_t)G.n_rot + (size_t)r;
            P.best[o] = (float)(bestv / (double)(e1 - e0)); P.best_shift[o] = bestq;
        }
    }
}

// The K best rotations of every particle of a chunk out of best[particle][n_rot]: ties to the lower rotation index.  One block per
// particle; pass k takes the best entry that ranks after pass k - 1's (score lower, or equal with a higher index), every thread over a
// strided share, combined in a fixed order.
__global__ void __launch_bounds__(256) k_csp_global_topk(const float *__restrict__ best, const int *__restrict__ best_shift, long n_rot, int K,
                                                         long *__restrict__ out_rot, int *__restrict__ out_shift, float *__restrict__ out_score) {
    __shared__ float sv[256]; __shared__ long si[256];
    const int tid = threadIdx.x;
    const float *b = best + (size_t)blockIdx.x * (size_t)n_rot;
    float pv = 0.f; long pi = -1;
    for (int k = 0; k < K; k++) {
        float v = -3.0e38f; long idx = -1;
        for (long r = tid; r < n_rot; r += 256) {
            const float x = b[r];
            const bool after = pi < 0 || x < pv || (x == pv && r > pi);
            if (after && (idx < 0 || x > v)) { v = x; idx = r; }
        }
        sv[tid] = v; si[tid] = idx;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (tid < h) {
                const float ov = sv[tid + h]; const long oi = si[tid + h];
                if (oi >= 0 && (si[tid] < 0 || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) { sv[tid] = ov; si[tid] = oi; }
            }
            __syncthreads();
        }
        pv = sv[0]; pi = si[0];
        if (tid == 0) {
            const size_t o = (size_t)blockIdx.x * K + k;
            out_rot[o] = pi; out_score[o] = pv; out_shift[o] = pi >= 0 ? best_shift[(size_t)blockIdx.x * (size_t)n_rot + (size_t)pi] : 0;
        }
        __syncthreads();
    }
}

}  // namespace ppm
