// ppm_geom.h — derived geometry of a refinement call (band limits, shift grid, orientation grid, ring-ordered sample list) and the rules
// that host and kernels share: the pose algebra, the compass rule (PPM_HD) and the constexpr prep_lds.  Plain C++, no HIP types.
//
// The quantities restate the numeric answers of the refine3d prompt script
// (src/pyp/refine/frealign/frealign.py:3918-3994) in Fourier-pixel units; the grid is the
// build-defined global grid of SURVEY.md §8a K6 (theta = 0..180 step D, n_phi = round(360 sin(theta)/D)).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ppm.h"

namespace ppm {

constexpr double kPi = 3.14159265358979323846;

// What the kernels call as well as the host is marked PPM_HD: `__host__ __device__` under hipcc, nothing under a plain C++ compiler
// (the CPU tests compile this header alone with g++).
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#define PPM_FORCEINLINE __forceinline__
#define PPM_UNROLL _Pragma("unroll")
#else
#define PPM_HD
#define PPM_FORCEINLINE inline
#define PPM_UNROLL
#endif
// Sine and cosine of a rotation step (radians; rot_xyz, rot_step), the call each side has always made: sincos in device code,
// std::sin and std::cos on the host.  Nobody has shown that the two agree to the last bit, and nothing depends on it.
PPM_HD inline void sincos_rad(double t, double *s, double *c) {
#ifdef __HIP_DEVICE_COMPILE__
    ::sincos(t, s, c);
#else
    *c = std::cos(t); *s = std::sin(t);
#endif
}

struct Geom {
    int N = 0;
    double a = 0;
    double r_hi = 0, r_lo = 0, r_s = 0, ring_signed = 0;
    double r_cls = 0;             // band of LOGP / SIGMA (answer 22, ppm_refine_cfg.res_classification); = r_hi when unset
    int B = 0, W = 0, H = 0;      // full band: half-width, row width B+1, rows 2B+1
    int Bs = 0, Hs = 0;           // search band
    int Ns = 0, RSx = 0, RSy = 0;
    double step = 0;              // global-search shift grid: Ns points over the box, step = N/Ns pixels
    int n_theta = 0, n_psi = 0, n_dir = 0, n_orient = 0, npsi_store = 0, half = 0;
    double dpsi = 0, dstep = 0, phi_max = 360, theta_max = 180;
    double range_asked_px = 0;    // largest shift search range the caller asked for, pixels (0: 'mask radius' / unlimited)
    bool range_capped = false;    // the window of the grid search is narrower than that
    double r_s_asked = 0;         // search band the caller asked for (> r_s when the 64-pixel cap of the grid search applied)
};

// asymmetric unit of the global grid (include/ppm.h, field `symmetry`)
inline void sym_limits(const char *sym, double &phi_max, double &theta_max) {
    phi_max = 360.0; theta_max = 180.0;
    if (!sym || !sym[0]) return;
    char t = sym[0] >= 'a' ? sym[0] - 32 : sym[0];
    int n = std::atoi(sym + 1);
    if (t == 'C' && n >= 1) phi_max = 360.0 / n;
    else if (t == 'D' && n >= 1) { phi_max = 360.0 / n; theta_max = 90.0; }
    else if (t == 'T' || t == 'I') { phi_max = 180.0; theta_max = 90.0; }
    else if (t == 'O') { phi_max = 90.0; theta_max = 90.0; }
}

// box sizes the FFTs handle: even, 32..512, prime factors 2, 3, 5, 7 only
inline bool box_ok(int n) {
    if (n < 32 || n > 512 || n % 2) return false;
    while (n % 2 == 0) n /= 2;
    while (n % 3 == 0) n /= 3;
    while (n % 5 == 0) n /= 5;
    while (n % 7 == 0) n /= 7;
    return n == 1;
}
// factors (4s first, then 2, 3, 5, 7) and the digit-reversal staging permutation of an FFT length
inline void fft_factors(int n, std::vector<int> &fac, std::vector<unsigned short> &perm) {
    fac.clear();
    int m = n;
    while (m % 4 == 0) { fac.push_back(4); m /= 4; }
    while (m % 2 == 0) { fac.push_back(2); m /= 2; }
    while (m % 3 == 0) { fac.push_back(3); m /= 3; }
    while (m % 5 == 0) { fac.push_back(5); m /= 5; }
    while (m % 7 == 0) { fac.push_back(7); m /= 7; }
    perm.resize(n);
    for (int i = 0; i < n; i++) {
        int pos = 0, rem = i, L = n;
        for (int st = (int)fac.size() - 1; st >= 0; st--) { int r = fac[st]; L /= r; pos += (rem % r) * L; rem /= r; }
        perm[i] = (unsigned short)pos;
    }
}

inline int n_phi_at(double theta_deg, double dstep, double phi_max = 360.0) {
    int np = (int)std::floor(phi_max * std::sin(theta_deg * kPi / 180.0) / dstep + 0.5);
    return np < 1 ? 1 : np;
}

inline bool geom_init(Geom &g, const ppm_refine_cfg &c, std::string &err) {
    g = Geom();
    g.N = c.box; g.a = c.pixel_size;
    if (!box_ok(g.N)) { err = "box size must be even, 32..512, with prime factors 2, 3, 5 and 7 only"; return false; }
    if (!(g.a > 0) || !(c.res_high > 0)) { err = "pixel size and high-resolution limit must be positive"; return false; }
    double na = g.N * g.a;
    g.r_hi = na / c.res_high; if (g.r_hi > g.N / 2) g.r_hi = g.N / 2;
    g.r_lo = c.res_low > 0 ? na / c.res_low : 0.0;
    g.r_s = c.res_search > 0 ? na / c.res_search : g.r_hi; if (g.r_s > g.r_hi) g.r_s = g.r_hi;
    g.r_s_asked = g.r_s;
    if (c.global_search && g.r_s > 64.0) g.r_s = 64.0;   // the grid-search kernel covers 64 Fourier pixels (lane = kx); finer
                                                         // detail only enters through the refinement of the hits
    g.ring_signed = c.res_signed_cc > 0 ? na / c.res_signed_cc : 1e30;
    // answer 22 (frealign.py:3945): 0, beyond res_high, or a band of less than one Fourier pixel above r_lo -> the full band
    g.r_cls = c.res_classification > 0 ? na / c.res_classification : g.r_hi;
    if (g.r_cls > g.r_hi || g.r_cls < g.r_lo + 1.0) g.r_cls = g.r_hi;
    g.B = (int)std::ceil(g.r_hi) - 1; g.W = g.B + 1; g.H = 2 * g.B + 1;
    g.Bs = (int)std::ceil(g.r_s) - 1; g.Hs = 2 * g.Bs + 1;
    if (g.B < 2) { err = "resolution limits leave fewer than 3 Fourier pixels"; return false; }
    g.Ns = 2; while (g.Ns < 2 * (g.Bs + 1)) g.Ns <<= 1;
    g.step = (double)g.N / g.Ns;
    // answers 27 / 28: 0 means the mask radius ("0.0 = mask radius", config/pyp_config.toml:5338-5343); the window is limited
    // only by the search grid itself (shifts beyond Ns / 2 - 1 steps alias).  Windows wider than PPM_MAX_SHIFT_STEPS steps
    // either side are searched as overlapping tiles of that half-width (ppm_refine_batch).
    double rx = (c.search_range_x > 0 ? c.search_range_x : c.mask_radius) / g.a, ry = (c.search_range_y > 0 ? c.search_range_y : c.mask_radius) / g.a;
    g.RSx = (int)std::ceil(rx / g.step); g.RSy = (int)std::ceil(ry / g.step);
    if (g.RSx < 1) g.RSx = 1;
    if (g.RSy < 1) g.RSy = 1;
    g.range_asked_px = std::max(rx, ry);
    const int rs_max = g.Ns / 2 - 1;
    g.range_capped = g.RSx > rs_max || g.RSy > rs_max;
    if (g.RSx > rs_max) g.RSx = rs_max;
    if (g.RSy > rs_max) g.RSy = rs_max;
    g.dstep = c.angular_step > 0 ? c.angular_step : 15.0;
    char symbuf[9]; std::memcpy(symbuf, c.symmetry, 8); symbuf[8] = 0;
    sym_limits(symbuf, g.phi_max, g.theta_max);
    g.n_theta = (int)std::floor(g.theta_max / g.dstep + 0.5) + 1;
    if (g.n_theta < 2) g.n_theta = 2;
    g.n_psi = (int)std::floor(360.0 / g.dstep + 0.5); if (g.n_psi < 1) g.n_psi = 1;
    g.dpsi = 360.0 / g.n_psi;
    g.n_dir = 0;
    for (int i = 0; i < g.n_theta; i++) g.n_dir += n_phi_at(g.theta_max * i / (g.n_theta - 1), g.dstep, g.phi_max);
    g.n_orient = g.n_dir * g.n_psi;
    g.half = (g.n_psi % 2 == 0);
    g.npsi_store = g.half ? g.n_psi / 2 : g.n_psi;
    return true;
}

inline void grid_direction(const Geom &g, int dir, double &theta, double &phi) {
    int acc = 0;
    for (int i = 0; i < g.n_theta; i++) {
        double th = g.theta_max * i / (g.n_theta - 1);
        int np = n_phi_at(th, g.dstep, g.phi_max);
        if (dir < acc + np) { theta = th; phi = g.phi_max * (dir - acc) / np; return; }
        acc += np;
    }
    theta = phi = 0;
}

// ---- pose algebra: one text for the host, the kernels and the CPU tests.  PPM_HD marks what device code calls as well.
// M = Rz(phi) Ry(theta) Rz(psi), row-major 3x3 ("rotates the reference by PHI -> THETA -> PSI",
// src/pyp/analysis/geometry/core.py:1186-1187)
PPM_HD inline void euler_matrix(double psi, double theta, double phi, double M[9]) {
    // the kernels have always multiplied by the folded constant pi / 180 here and the host by pi, then divided: one rounding apart,
    // kept on each side (every other conversion below is the host's text on both)
#ifdef __HIP_DEVICE_COMPILE__
    const double d2r = kPi / 180.0, ps = psi * d2r, th = theta * d2r, ph = phi * d2r;
#else
    const double ps = psi * kPi / 180, th = theta * kPi / 180, ph = phi * kPi / 180;
#endif
    double cps = std::cos(ps), sps = std::sin(ps), cth = std::cos(th), sth = std::sin(th), cph = std::cos(ph), sph = std::sin(ph);
    M[0] = cph * cth * cps - sph * sps; M[1] = -cph * cth * sps - sph * cps; M[2] = cph * sth;
    M[3] = sph * cth * cps + cph * sps; M[4] = -sph * cth * sps + cph * cps; M[5] = sph * sth;
    M[6] = -sth * cps;                  M[7] = sth * sps;                    M[8] = cth;
}

// (psi, theta, phi) in degrees of M = Rz(phi) Ry(theta) Rz(psi); at theta = 0 / 180 everything goes into psi
// (theta = 0: M = Rz(phi + psi), M[0] = cos, M[3] = sin; theta = 180: M = Rz(phi) Ry(180) Rz(psi) has M[0] = -cos(psi - phi),
// M[3] = sin(psi - phi), so psi - phi = atan2(M[3], -M[0]))
PPM_HD inline void angles_from_matrix(const double M[9], double &psi, double &theta, double &phi) {
    const double r2d = 180.0 / kPi;
    double ct = M[8] > 1 ? 1 : (M[8] < -1 ? -1 : M[8]);
    double st = std::sqrt(M[2] * M[2] + M[5] * M[5]);
    if (st > 1e-7) { theta = std::atan2(st, ct) * r2d; phi = std::atan2(M[5], M[2]) * r2d; psi = std::atan2(M[7], -M[6]) * r2d; }
    else { theta = ct > 0 ? 0.0 : 180.0; phi = 0.0; psi = (ct > 0 ? std::atan2(M[3], M[0]) : std::atan2(M[3], -M[0])) * r2d; }
    if (psi < 0) psi += 360;
    if (phi < 0) phi += 360;
}

PPM_HD inline void mat_mul3(const double *a, const double *b, double *c) {      // c may be a or b
    double t[9];
    PPM_UNROLL
    for (int i = 0; i < 3; i++)
        PPM_UNROLL
        for (int j = 0; j < 3; j++) {
            double v = 0;
            PPM_UNROLL
            for (int k = 0; k < 3; k++) v += a[i * 3 + k] * b[k * 3 + j];
            t[i * 3 + j] = v;
        }
    PPM_UNROLL
    for (int i = 0; i < 9; i++) c[i] = t[i];
}
PPM_HD inline void rot_xyz(int k, double deg, double R[9]) {      // right-handed rotation about x (0), y (1), z (2)
    double s, c;
    sincos_rad(deg * kPi / 180.0, &s, &c);
    if (k == 0) { R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = c; R[5] = -s; R[6] = 0; R[7] = s; R[8] = c; }
    else if (k == 1) { R[0] = c; R[1] = 0; R[2] = s; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = -s; R[7] = 0; R[8] = c; }
    else { R[0] = c; R[1] = -s; R[2] = 0; R[3] = s; R[4] = c; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1; }
}
// Rotations of the sub-tomogram global search (ppm_sva_cfg.search_mode 1, include/ppm.h), row-major 3x3 each: G = E(psi, theta, phi)
// on rings theta = theta_max i / (n - 1), n = round(theta_max / step) + 1, with n_phi = round(phi_max sin theta / step) directions
// phi = phi_max j / n_phi each and n_psi = round(360 / step) in-plane angles.  (phi_max, theta_max) = sym_limits(sym): the whole of
// SO(3) for "" / "C1" - candidates N0 G -, the asymmetric unit of the point group otherwise - candidates G N0, because pose N is
// equivalent to S N for every operator S (F_v(k) = Ref(N k) and Ref(S x) = Ref(x)) and the cut in phi and theta is one on the left.
inline std::vector<double> sva_rotation_grid(double gstep, const char *sym) {
    std::vector<double> grid_d;
    double phi_max, theta_max;
    sym_limits(sym, phi_max, theta_max);
    int n_theta = (int)std::floor(theta_max / gstep + 0.5) + 1; if (n_theta < 2) n_theta = 2;
    int n_psi = (int)std::floor(360.0 / gstep + 0.5); if (n_psi < 1) n_psi = 1;
    for (int i = 0; i < n_theta; i++) {
        const double th = theta_max * i / (n_theta - 1);
        int np = (int)std::floor(phi_max * std::sin(th * kPi / 180.0) / gstep + 0.5); if (np < 1) np = 1;
        for (int j = 0; j < np; j++) for (int k = 0; k < n_psi; k++) {
            double G[9]; euler_matrix(k * 360.0 / n_psi, th, phi_max * j / np, G);
            grid_d.insert(grid_d.end(), G, G + 9);
        }
    }
    return grid_d;
}

// Row pose of the constrained geometry (include/ppm.h, ppm_csp_cfg): M_row = N Ry(-tilt) Rz(axis),
// g = [Rz(-axis) Ry(tilt) (-p)]_xy + tilt shift (pixels)
// the four rotations a tilt contributes to its rows' poses (the trigonometry of csp_row_pose, shared by all rows of the tilt)
struct TiltRot { double a[9], b[9], ai[9], bi[9]; };     // Ry(-tilt), Rz(axis), Rz(-axis), Ry(tilt)
PPM_HD inline void tilt_rotations(double tilt, double axis, TiltRot &r) { rot_xyz(1, -tilt, r.a); rot_xyz(2, axis, r.b); rot_xyz(2, -axis, r.ai); rot_xyz(1, tilt, r.bi); }
PPM_HD inline void csp_row_pose(const double N[9], const double p[3], const TiltRot &r, double tsx, double tsy, double M[9], double g[2]) {
    double t[9];
    mat_mul3(N, r.a, t); mat_mul3(t, r.b, M);
    const double q0 = -p[0], q1 = -p[1], q2 = -p[2];
    double u[3], v[2];
    PPM_UNROLL
    for (int i = 0; i < 3; i++) u[i] = r.bi[i * 3] * q0 + r.bi[i * 3 + 1] * q1 + r.bi[i * 3 + 2] * q2;
    PPM_UNROLL
    for (int i = 0; i < 2; i++) v[i] = r.ai[i * 3] * u[0] + r.ai[i * 3 + 1] * u[1] + r.ai[i * 3 + 2] * u[2];
    g[0] = v[0] + tsx; g[1] = v[1] + tsy;
}
PPM_HD inline void csp_row_pose(const double N[9], const double p[3], double tilt, double axis, double tsx, double tsy, double M[9], double g[2]) {
    TiltRot r; tilt_rotations(tilt, axis, r);
    csp_row_pose(N, p, r, tsx, tsy, M, g);
}
// a displacement d[6] applied to a particle unit: N <- N Rx(d0) Ry(d1) Rz(d2) (a zero angle is skipped, not multiplied in), p += d[3..5]
PPM_HD inline void unit_apply_delta(double *N, double *p, const double *d) {
    for (int k = 0; k < 3; k++)
        if (d[k] != 0.0) { double R[9]; rot_xyz(k, d[k], R); mat_mul3(N, R, N); }
    for (int k = 0; k < 3; k++) p[k] += d[3 + k];
}

// One step of the local refinement's search.  which: 0 = in-plane (psi), 1 / 2 = tilt about image x / y when tilt_frame, else
// theta / phi Euler steps.  The three image-frame steps are right-multiplications by Rz / Rx / Ry: plain column mixes.
// (column indices are compile-time constants: with run-time indices the 3 x 3 temporaries lived in scratch memory, ~1.2 MB
// of scratch traffic per particle from the serial set-up sections)
template <int A, int B, int K>
PPM_HD PPM_FORCEINLINE void col_mix(const double *M, double s, double c, double *out) {
    // M R with R rotating the (A, B) coordinate pair: out[:,A] = c M[:,A] + s M[:,B], out[:,B] = -s M[:,A] + c M[:,B]
    PPM_UNROLL
    for (int r = 0; r < 3; r++) {
        const double ma = M[r * 3 + A], mb = M[r * 3 + B];
        out[r * 3 + A] = ma * c + mb * s;
        out[r * 3 + B] = mb * c - ma * s;
        out[r * 3 + K] = M[r * 3 + K];
    }
}
PPM_HD inline void rot_step(const double *M, int which, int tilt_frame, double hdeg, double *out) {
    double s, c;
    sincos_rad(hdeg * kPi / 180.0, &s, &c);
    if (which == 0) { col_mix<0, 1, 2>(M, s, c, out); return; }
    if (tilt_frame) {
        if (which == 1) col_mix<1, 2, 0>(M, s, c, out); else col_mix<2, 0, 1>(M, s, c, out);
        return;
    }
    if (which == 2) { double r[9] = { c, -s, 0, s, c, 0, 0, 0, 1 }; mat_mul3(r, M, out); return; }
    double psi, th, ph; angles_from_matrix(M, psi, th, ph);
    double cp = std::cos(ph * kPi / 180.0), sp = std::sin(ph * kPi / 180.0);
    double rz[9] = { cp, -sp, 0, sp, cp, 0, 0, 0, 1 }, rzt[9] = { cp, sp, 0, -sp, cp, 0, 0, 0, 1 }, ry[9] = { c, 0, s, 0, 1, 0, -s, 0, c };
    double T[9], L[9];
    mat_mul3(rz, ry, T); mat_mul3(T, rzt, L); mat_mul3(L, M, out);
}

// ---- the compass rule: what one iteration of every search (k_local; k_csp_step_trial / k_csp_step_accept for the constrained and the
// sub-tomogram searches) decides from its scores.  It restates the oracle's loops operand for operand; tests/test_compass_rule_cpu.py
// holds it to them bit for bit.  NP parameters, the first three angles (step ha), the rest shifts (step hs); en[] switches them.
constexpr double kNoProbe = -1e300;       // score of a probe outside the bounds, and of a disabled parameter's
// Trial step d[] from the centre's score f0 and the probes' scores: per enabled parameter the vertex of the parabola through f(-h), f0,
// f(+h), clamped to +-h; without usable curvature (den <= 1e-12) a full step towards the better probe if that beats f0.  The probes
// come two per enabled parameter, + before -, in parameter order: `pang` those of the angles, `psh` those of the shifts (null: they
// follow the angles'; k_local's sweep keeps the centre between the two runs).  With bounds (tol != null; acc = the displacement so far) a probe that would
// leave +-tol counts as kNoProbe, a parameter with one probe left steps towards it if it beats f0, and acc + d is clamped to +-tol;
// tol == null is the unbounded search: both probes in bounds and no clamp, the same arithmetic and nothing more.
// fp[] / fm[] receive the probes' scores as compass_accept wants them.
template <int NP>
PPM_HD inline void compass_trial(double f0, const double *pang, const double *psh, const int *en, double ha, double hs,
                                 const double *acc, const double *tol, double *d, double *fp, double *fm) {
    const double *q = pang;
    for (int i = 0; i < NP; i++) {
        d[i] = 0; fp[i] = fm[i] = kNoProbe;
        if (i == 3 && psh) q = psh;
        if (!en[i]) continue;
        const double h = i < 3 ? ha : hs;
        const bool okp = !tol || std::fabs(acc[i] + h) <= tol[i] + 1e-9, okm = !tol || std::fabs(acc[i] - h) <= tol[i] + 1e-9;
        const double p = okp ? q[0] : kNoProbe, m = okm ? q[1] : kNoProbe;
        q += 2;
        fp[i] = p; fm[i] = m;
        if (okp && okm) {
            const double den = 2.0 * f0 - p - m;
            if (den > 1e-12) { const double t = 0.5 * h * (p - m) / den; d[i] = t > h ? h : (t < -h ? -h : t); }
            else { const double best = p > m ? p : m; d[i] = best > f0 ? (p > m ? h : -h) : 0.0; }
        } else if (okp) d[i] = p > f0 ? h : 0.0;
        else if (okm) d[i] = m > f0 ? -h : 0.0;
        if (tol) {
            if (acc[i] + d[i] > tol[i]) d[i] = tol[i] - acc[i];
            if (acc[i] + d[i] < -tol[i]) d[i] = -tol[i] - acc[i];
        }
    }
}
// What the iteration does once the trial pose is scored (ft): the trial step if it beats the centre and is no worse than the best probe,
// else the best single probe (scanned in parameter order, + before -, a later one has to be strictly better), else nothing.
// bi / bs: parameter and sign of the best probe (bi < 0: none beats f0), fb its score.
enum CompassMove { kCompassStay = 0, kCompassTrial, kCompassProbe };
template <int NP>
PPM_HD inline CompassMove compass_accept(double f0, double ft, const double *fp, const double *fm, const int *en, int &bi, int &bs, double &fb) {
    bi = -1; bs = 0; fb = f0;
    for (int i = 0; i < NP; i++) {
        if (!en[i]) continue;
        if (fp[i] > fb) { fb = fp[i]; bi = i; bs = 1; }
        if (fm[i] > fb) { fb = fm[i]; bi = i; bs = -1; }
    }
    if (ft > f0 && ft >= fb) return kCompassTrial;
    return bi >= 0 ? kCompassProbe : kCompassStay;
}

// Frequency marching: band of one compass iteration from its probe displacement (angle step `ha` degrees at the mask radius `rm_px`,
// shift step `hs` pixels).  Rings whose phase moves by more than about `bf` radians under the larger of the two carry no usable
// gradient; bf < 0 or no probe at all leaves the cap.  The one rule of every search (refinement, csp, sub-tomograms, and the coarse
// band of a rotation grid: ha = half the grid step, no shifts); it restates the oracle's iter_band, operand for operand.
inline double march_band(double bf, int N, double rm_px, double ha, double hs, bool any_ang, bool any_sh, double rcap) {
    if (bf < 0) return rcap;
    double d = 0;
    if (any_ang) d = rm_px * ha * kPi / 180.0;
    if (any_sh && hs > d) d = hs;
    if (!(d > 0)) return rcap;
    double rit = bf * N / (2.0 * kPi * d);
    if (rit < 4.0) rit = 4.0;
    return rit < rcap ? rit : rcap;
}
// Compass iterations until the larger first step has halved below `steptol`: ceil(log2(max(ha, hs) / steptol)), min_iters .. 12
inline int compass_iterations(double ha, double hs, double steptol, int min_iters) {
    const double m = std::max(ha, hs);
    const int T = m > steptol ? (int)std::ceil(std::log(m / steptol) / std::log(2.0)) : min_iters;
    return std::min(12, std::max(min_iters, T));
}
// ---- tap reuse in the compass sweep of k_local's full-band launch (ppm_dev.h, "tap reuse"): the neighbour poses of an iteration lie
// `ha` degrees from the centre pose, so their sample at |k| lies ha |k| pad voxels of the padded cube from the centre's, at the edge
// of the iteration's band `rband` (Fourier pixels) near_move() voxels.  The reusing loop pays ~24 more vector instructions per
// neighbour gather and saves the line look-ups of the lanes that stay in the centre's cell; it is taken while the move at the band's
// edge is at most kNearMove voxels (CHANGELOG.md, "k_local: compass neighbours reuse the centre's taps", has the measurement).
constexpr double kNearMove = 1.6;
inline double near_move(double ha, double pad, double rband) { return ha * kPi / 180.0 * pad * rband; }
inline bool near_reuse_pays(bool any_ang, double ha, double pad, double rband) { return any_ang && near_move(ha, pad, rband) <= kNearMove; }

// ---- launch plan of the pre-processing kernel (k_prep, ppm_kernels.h): block shape, row pairs per row pass, column chunks and the
// carve-up of the block's dynamic LDS.  launch_prep (host_refine.h) launches from it and the kernel takes its pointers from the same
// prep_lds, so the two cannot disagree; tests/test_prep_plan_cpu.py pins the Python restatement of the box sweep to it.
struct LdsRegion { unsigned off, bytes, elem; };      // byte offset, extent, element size (= the alignment the region needs)
struct PrepLds {
    LdsRegion T;        // float2 [nc][TS]  column chunk
    LdsRegion Wk;       // float2 [L][WS]   row work buffer; shares T's storage on the scratch-free path (the phases alternate)
    LdsRegion ringq;    // u64 [B+2]        ring power sums, 64-bit fixed point
    LdsRegion ringc;    // u32 [B+2]        ring sample counts
    LdsRegion ringpw;   // float [B+2]      ring weights
    LdsRegion red;      // double [5 waves] block reduction slots of the statistics, 16-byte aligned
    LdsRegion stat;     // float [4 + waves] mean, scale, fixed-point scale, nI partials
    LdsRegion fmask;    // float [8]        mask disc (centre, radius), beam-tilt coefficients
    LdsRegion tw;       // float2 [N]       twiddles of the FFT plan
    LdsRegion perm;     // u16 [N]          staging position of sample i   (scratch path only: the scratch-free path stages in
    LdsRegion iperm;    // u16 [N]          sample staged at position d     natural order; both empty there)
    unsigned total;     // bytes the launch asks for
};
constexpr int prep_threads(bool scratch_free) { return scratch_free ? 512 : 256; }
// the regions in order; `total` is left to prep_lds
constexpr PrepLds prep_lds_regions(bool scratch_free, int N, int B, int L, int nc, int TS, int WS) {
    const unsigned waves = prep_threads(scratch_free) / 64, nb = (unsigned)(B + 2), n = (unsigned)N;
    const unsigned tb = (unsigned)nc * (unsigned)TS * 8, wb = (unsigned)L * (unsigned)WS * 8;
    PrepLds l = {};
    l.T = { 0, tb, 8 };
    l.Wk = { scratch_free ? 0 : tb, wb, 8 };
    l.ringq = { scratch_free ? (tb > wb ? tb : wb) : tb + wb, nb * 8, 8 };
    l.ringc = { l.ringq.off + l.ringq.bytes, nb * 4, 4 };
    l.ringpw = { l.ringc.off + l.ringc.bytes, nb * 4, 4 };
    l.red = { (l.ringpw.off + l.ringpw.bytes + 15) & ~15u, 5 * waves * 8, 16 };
    l.stat = { l.red.off + l.red.bytes, (4 + waves) * 4, 4 };
    l.fmask = { l.stat.off + l.stat.bytes, 8 * 4, 4 };
    l.tw = { l.fmask.off + l.fmask.bytes, n * 8, 8 };
    l.perm = { l.tw.off + l.tw.bytes, scratch_free ? 0 : n * 2, 2 };
    l.iperm = { l.perm.off + l.perm.bytes, scratch_free ? 0 : n * 2, 2 };
    return l;
}
// bytes budgeted behind the two buffers, known before L and nc are: the regions from ringq on as they lie behind empty buffers, 16 for
// the alignment of `red` behind buffers that end on an odd multiple of 8, and 16 spare
constexpr unsigned prep_lds_tail(bool scratch_free, int N, int B) {
    const PrepLds l = prep_lds_regions(scratch_free, N, B, 0, 0, 0, 0);
    return l.iperm.off + l.iperm.bytes + 16 + 16;
}
constexpr PrepLds prep_lds(bool scratch_free, int N, int B, int L, int nc, int TS, int WS) {
    PrepLds l = prep_lds_regions(scratch_free, N, B, L, nc, TS, WS);
    l.total = l.ringq.off + prep_lds_tail(scratch_free, N, B);
    return l;
}
struct PrepPlan {
    bool scratch_free;            // box 256: k_prep<512, 2>; every other box: k_prep<256, 3> through the global scratch
    int threads, L, nc, nchunks;  // row pairs per row pass, columns per column chunk, chunks
    int TS, WS;                   // line strides of T and Wk (float2)
    PrepLds lds;
    const char *err;              // null, or why box N / band B cannot be planned
};
inline PrepPlan prep_plan(int N, int B, int W) {
    PrepPlan p = {};
    p.scratch_free = N == 256; p.threads = prep_threads(p.scratch_free);
    if (p.scratch_free) {     // T (64 columns) and the row buffer (64 row pairs) share one 140 KB region; strides spread over the banks
        p.TS = 273; p.WS = 272;
        p.L = 64; p.nc = 64; p.nchunks = (std::min(W, 128) + 63) / 64;
        p.lds = prep_lds(true, N, B, p.L, p.nc, p.TS, p.WS);
        if (p.lds.total > 160u * 1024) p.err = "pre-processing kernel: LDS plan exceeds 160 KB";
        return p;
    }
    // L row pairs per row pass (L N <= 8 x threads: the next pass is prefetched into <= 8 register pairs per thread; L divides
    // N/2) and the nc columns of one column chunk; the whole half spectrum goes through a global scratch between the two phases
    constexpr size_t budget = 40 * 1024;
    const size_t tail = prep_lds_tail(false, N, B);
    p.TS = N + 1; p.WS = N;
    p.L = std::max(1, std::min(8 * p.threads / N, N / 2));
    // the row pass walks the image 2 L rows at a time; leave about half of the LDS to the column chunk
    while (p.L >= 1 && ((N / 2) % p.L || (size_t)p.L * p.WS * 8 + tail + (size_t)p.TS * 8 > budget / 2 + 8192)) p.L--;
    if (p.L < 1) { p.err = "pre-processing kernel: row buffer does not fit the LDS"; return p; }
    const size_t wk = (size_t)p.L * p.WS * 8;
    const size_t left = budget - tail > wk ? budget - tail - wk : 0;
    p.nc = std::max(1, std::min(W, (int)(left / ((size_t)p.TS * 8))));
    p.nc = std::max(1, std::min(p.nc, 12 * p.threads / N));      // k_prep prefetches one chunk into 12 register pairs per thread
    p.nchunks = (W + p.nc - 1) / p.nc;
    p.nc = (W + p.nchunks - 1) / p.nchunks;                      // even chunks
    p.lds = prep_lds(false, N, B, p.L, p.nc, p.TS, p.WS);
    if (p.lds.total > budget) p.err = "pre-processing kernel: LDS plan exceeds its budget";
    return p;
}

// SCORE / SIGMA / LOGP columns of a row from its correlation over the band r_lo .. r_hi (Fourier pixels)
PPM_HD inline void score_columns(double cc, double r_lo, double r_hi, double *score, double *sigma, double *logp) {
    double res = 1.0 - cc * cc; if (res < 1e-6) res = 1e-6;
    *score = 100.0 * cc; *sigma = std::sqrt(res);
    *logp = -0.5 * (kPi * (r_hi * r_hi - r_lo * r_lo)) * (std::log(2.0 * kPi * res) + 1.0);
}

// Ring-ordered sample list of the half plane kx >= 0, 0 < k^2 < r_hi^2, ring = floor(|k|); every
// ring padded to a multiple of 16 samples with weightless dummies so that a 16-lane group never
// straddles two rings.  Packed: kx (9 bits) | ky+256 (10 bits) << 9 | alpha (2 bits) << 19 | ring << 21.
struct SampleList {
    std::vector<uint32_t> packed;
    std::vector<int> ring_off;   // ring_off[b] = length of the list prefix holding all samples of rings < b; size B+3
};

inline uint32_t pack_sample(int kx, int ky, int alpha, int ring) {
    return (uint32_t)kx | ((uint32_t)(ky + 256) << 9) | ((uint32_t)alpha << 19) | ((uint32_t)ring << 21);
}

inline void build_samples(const Geom &g, SampleList &sl) {
    int B = g.B;
    std::vector<std::vector<uint32_t>> rings(B + 2);
    double r2 = g.r_hi * g.r_hi;
    for (int ky = -B; ky <= B; ky++) for (int kx = 0; kx <= B; kx++) {
        double k2 = (double)kx * kx + (double)ky * ky;
        if (k2 >= r2 || k2 == 0) continue;
        int b = (int)std::floor(std::sqrt(k2));
        rings[b].push_back(pack_sample(kx, ky, kx == 0 ? 1 : 2, b));
    }
    // List order: bands of kRingBand consecutive rings; inside a band the 16-sample groups (one ring each, ky-ordered = along
    // the arc) of all its rings are sorted by their angular position, so that the four groups a wavefront takes (64
    // consecutive entries) form a compact 4 x 16 patch of the slice rather than a 64-sample arc: fewer distinct cache lines
    // of the reference cube per gather.  ring_off[b] = length of the list prefix that holds every sample of the rings < b
    // (the end of the band of ring b - 1; samples beyond a band limit are masked individually by the kernels).
    constexpr int kRingBand = 4;
    sl.packed.clear(); sl.ring_off.assign(B + 3, 0);
    for (int b0 = 0; b0 <= B + 1; b0 += kRingBand) {
        struct Grp { double key; int ring; int first; };
        std::vector<Grp> grps;
        const int b1 = std::min(b0 + kRingBand - 1, B + 1);
        for (int b = b0; b <= b1; b++) {
            while (rings[b].size() % 16) rings[b].push_back(pack_sample(0, 0, 0, b));
            const int G = (int)rings[b].size() / 16;
            for (int gidx = 0; gidx < G; gidx++) grps.push_back({ (gidx + 0.5) / G, b, gidx * 16 });
        }
        std::stable_sort(grps.begin(), grps.end(), [](const Grp &x, const Grp &y) { return x.key < y.key; });
        for (const Grp &gr : grps) for (int i = 0; i < 16; i++) sl.packed.push_back(rings[gr.ring][gr.first + i]);
        for (int b = b0; b <= b1; b++) sl.ring_off[b + 1] = (int)sl.packed.size();
    }
    sl.ring_off[B + 2] = (int)sl.packed.size();
}

// Point-group operators (row-major 3x3 each); "C1","Cn","Dn","T","O","I"
inline void rot_axis(const double ax[3], double deg, double *m) {
    double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    double x = ax[0] / n, y = ax[1] / n, z = ax[2] / n, t = deg * kPi / 180, c = std::cos(t), s = std::sin(t), C = 1 - c;
    double r[9] = { c + x * x * C, x * y * C - z * s, x * z * C + y * s, y * x * C + z * s, c + y * y * C, y * z * C - x * s,
                    z * x * C - y * s, z * y * C + x * s, c + z * z * C };
    std::memcpy(m, r, sizeof(r));
}
inline int symmetry_ops(const char *sym, std::vector<double> &ops) {
    double gens[27]; int ng = 0;
    double z[3] = { 0, 0, 1 }, x[3] = { 1, 0, 0 }, d111[3] = { 1, 1, 1 };
    if (!sym || !sym[0]) sym = "C1";
    char t = sym[0] >= 'a' ? sym[0] - 32 : sym[0];
    int n = std::atoi(sym + 1);
    if (t == 'C' && n >= 1) { rot_axis(z, 360.0 / n, gens); ng = 1; }
    else if (t == 'D' && n >= 1) { rot_axis(z, 360.0 / n, gens); rot_axis(x, 180, gens + 9); ng = 2; }
    else if (t == 'T') { rot_axis(z, 180, gens); rot_axis(d111, 120, gens + 9); ng = 2; }
    else if (t == 'O') { rot_axis(z, 90, gens); rot_axis(d111, 120, gens + 9); ng = 2; }
    else if (t == 'I') {
        double phi = (1 + std::sqrt(5.0)) / 2, a5[3] = { 0, 1, phi };
        rot_axis(z, 180, gens); rot_axis(d111, 120, gens + 9); rot_axis(a5, 72, gens + 18); ng = 3;
    } else return -1;
    ops.assign(9, 0.0); ops[0] = ops[4] = ops[8] = 1.0;
    int cnt = 1;
    for (bool grew = true; grew;) {
        grew = false;
        for (int i = 0; i < cnt && cnt < 60; i++) for (int j = 0; j < ng && cnt < 60; j++) {
            double c[9]; mat_mul3(&ops[i * 9], gens + j * 9, c);
            bool found = false;
            for (int k = 0; k < cnt && !found; k++) {
                double d = 0; for (int q = 0; q < 9; q++) d += std::fabs(ops[k * 9 + q] - c[q]);
                if (d < 1e-6) found = true;
            }
            if (!found) { ops.insert(ops.end(), c, c + 9); cnt++; grew = true; }
        }
    }
    return cnt;
}

}  // namespace ppm
