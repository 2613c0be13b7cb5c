/* ppm.h — C ABI of libpypmatch.so: per-particle projection matching and Fourier-slice
 * insertion on one MI355X (gfx950).  This is the drop-in boundary for the numerics PYP
 * shells out to external binaries (none of which ship as source):
 *
 *   ppm_refine_batch      replaces the per-range `refine3d` process that
 *                         src/pyp/refine/frealign/frealign.py:3918-3994 (mrefine_version)
 *                         scripts and src/pyp/system/local_run.py:472-579 fans out; the
 *                         `.par` twin is src/pyp/system/wrapper_functions.py:512-561.
 *   ppm_insert_batch      replaces the per-range `reconstruct3d` process scripted at
 *                         src/pyp/refine/frealign/frealign.py:1780-1824 (split_reconstruction).
 *   ppm_accum_add /       replace `local_merge3d` (frealign.py:1878-1888): sum of dump pairs.
 *   ppm_accum_download
 *   ppm_finalize          replaces `merge3d` (frealign.py:2075-2093): FSC / part-FSC / SSNR table,
 *                         Wiener-filtered map and the two half maps.
*   ppm_sva_align /       replace the alignment and averaging steps of `external/TOMO/MPI_Classification`
 *   ppm_sva_insert        (src/pyp/refine/tomo_avg/sub_tomo_avg.py:468-555, src/pyp_main.py:3007-3107).
 *   ppm_reference_create  is the "input reconstruction" preparation both binaries do at start-up
 *                         (answer 4 of the refine3d script, frealign.py:3923).
 *
 * A parameter row is the 32-column `.cistem` row in file order
 * (src/pyp/inout/metadata/cistem_star_file.py:596-628), held as doubles like the reference
 * holds it in RAM (:716-727).  Angles in degrees, shifts in Angstrom (src/pyp/analysis/scores.py:693).
 *
 * Conventions: all functions return 0 on success, a negative errno-style code on failure and
 * leave a message for ppm_last_error() (thread-local).  The caller owns every host buffer; the library owns
 * device memory.  No torch types cross this boundary.
 *
 * Process model: one process per GPU.  ppm_init binds the process to one device (a second call with another index
 * fails).  Thread-compatible per handle: every reference / accumulator handle owns its HIP streams and workspaces, so calls on
 * DIFFERENT handles may be made concurrently from different threads (two class references refined side by side, an insertion
 * running next to a refinement); calls on ONE handle must be serialised by the caller.  Process-wide tables (FFT plans, the
 * profiling counters) are guarded inside the library.  Entry points without a handle (ppm_extract_boxes, ppm_device_*,
 * ppm_host_*) are thread-safe; ppm_extract_boxes calls share one stream and are serialised on the device.
 *
 * Stream ordering: device buffers handed in (resident particle stacks, an external accumulator buffer, extraction
 * outputs) are read / written on the handle's stream, which is NOT ordered against any stream of the caller: finish
 * (or synchronise) the work that produces them before the call; every entry point returns only after its own device
 * work has completed, so results may be used on any stream afterwards.
 */
#ifndef PPM_H
#define PPM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPM_NCOL 32 /* columns of a .cistem row */
/* column indices inside a row (cistem_star_file.py:596-628) */
enum {
    PPM_POS = 0, PPM_PSI = 1, PPM_THETA = 2, PPM_PHI = 3, PPM_XSHIFT = 4, PPM_YSHIFT = 5,
    PPM_DF1 = 6, PPM_DF2 = 7, PPM_ANGAST = 8, PPM_PSHIFT = 9, PPM_FILM = 10, PPM_OCC = 11,
    PPM_LOGP = 12, PPM_SIGMA = 13, PPM_SCORE = 14, PPM_PIXEL = 15, PPM_VOLTAGE = 16,
    PPM_CS = 17, PPM_AMP = 18, PPM_BTX = 19, PPM_BTY = 20, PPM_PIND = 26, PPM_TIND = 27
};
/* BEAM_TILT_X / BEAM_TILT_Y (milliradians): every particle spectrum is multiplied by exp(-i phi), phi(s) = 2 pi Cs lambda^2 |s|^2 (s . b), when
 * it is prepared (k_prep), i.e. the model is compared with, and the reconstruction receives, the image with the beam-tilt phase error
 * removed.  The sign follows the usual convention (the tilted beam multiplies the image transform by exp(+i phi)); the absent programs'
 * own convention is not visible: unpinned like the rest of the arithmetic. */

#define PPM_MAX_SHIFT_STEPS 8 /* half-width of the global-search shift window, in search-grid steps */
#define PPM_MAX_TOP_HITS 64
#define PPM_MAX_DEFOCUS_STEPS 20 /* defocus offsets tried on either side when refine_defocus is set */

/* Refinement settings = the numeric answers of the refine3d prompt script
 * (frealign.py:3918-3994; answer numbers as in SURVEY.md §9.1). */
typedef struct ppm_refine_cfg {
    int box;                  /* particle box edge N (power of two, 32..512) */
    float pixel_size;         /* 15: Angstrom per pixel */
    float molecular_mass_kda; /* 16 (kept for the log; not used by matching) */
    float mask_radius;        /* 18: outer mask radius, Angstrom */
    float res_low;            /* 19: low-resolution limit, Angstrom (0 = none) */
    float res_high;           /* 20: high-resolution limit, Angstrom */
    float res_signed_cc;      /* 21: rings at lower resolution than this are summed signed, the
                                 rest by absolute value; 0 = all signed */
    float search_mask_radius; /* 23: mask radius for the global search, Angstrom (0 = mask_radius) */
    float res_search;         /* 24: resolution limit of the global search, Angstrom; the grid search itself never uses more
                                 than 64 Fourier pixels (a finer limit is lowered to that and ppm_refine_note() says so; the hits
                                 are still refined up to res_high) */
    float angular_step;       /* 25: degrees */
    int top_hits;             /* 26: global-search hits that get refined (the caller passes 20) */
    float search_range_x;     /* 27: Angstrom, 0 = widest supported window */
    float search_range_y;     /* 28 */
    int global_search;        /* 36: grid search over the asymmetric unit; its `top_hits` best orientations are ALWAYS refined
                                 (iters_hit compass iterations each, at the search band) and the best one is kept - PYP's default
                                 call is global = yes, local = no with 20 hits to refine (frealign.py:3866-3871, :3953) */
    int local_refine;         /* 37: with global_search: the best hit continues at the full band (iters_final iterations);
                                 without: refinement starts at the row's pose (iters_hit + iters_final iterations).
                                 SCORE / LOGP / SIGMA always come from one last evaluation at the full band */
    int refine_psi, refine_theta, refine_phi, refine_x, refine_y; /* 38-42 */
    int normalize;            /* 46: normalise particles */
    int invert;               /* 47: invert contrast */
    /* build-defined knobs (0 = default), DESIGN.md "search driver" */
    float mask_falloff;       /* cosine edge width of the mask, Angstrom (default 20) */
    int iters_hit;            /* compass iterations run on every hit (0 = default 2; < 0 = none: hits stay on the grid, test hook) */
    int iters_final;          /* further iterations on the best hit / on a local-only start (default 7) */
    float local_angle_step;   /* first step of a local-only refinement, degrees (default 2.5) */
    float local_shift_step;   /* same for shifts, pixels (default 2) */
    char symmetry[8];         /* 11: point group of the reference ("C1", "C7", "D7", "T", "O", "I"; "" = C1).  The global grid
                                 is restricted to phi < 360/n for Cn / Dn and theta <= 90 for Dn; T and I search the D2 unit they
                                 contain, O the D4 unit.  Every pose found is symmetry-equivalent to the unrestricted optimum */
    float band_factor;        /* frequency marching: a compass iteration whose largest probe displacement is d pixels
                                 (mask radius x angular step in radians, or the shift step) scores only rings below
                                 band_factor * N / (2 pi d), capped by the stage's band.  0 = default 3, < 0 = off */
    int refine_defocus;       /* 45: after the pose, score defocus offsets -range..+range in steps of `defocus_step` at the final
                                 pose and full band (both DEFOCUS_1 and DEFOCUS_2 move together); the best offset is added to
                                 the two columns; ties keep the smaller index (0 first) */
    float defocus_range;      /* 33: Angstrom (the caller passes 500) */
    float defocus_step;       /* 34: Angstrom (the caller passes 50); at most 20 steps either side */
    float focus[4];           /* 29-32 + 44 "apply 2D masking" (class_focusmask, frealign.py:3846-3849, :3958): centre (x, y, z) of a sphere
                                 in the reference, Angstrom FROM THE BOX CENTRE, and its radius; radius > 0 replaces the centred circular
                                 mask of every particle image by a cosine-edged disc of that radius around the sphere's projection at the
                                 row's INPUT pose: centre = (M^T c)_xy + shift (M = Rz(phi) Ry(theta) Rz(psi)).  The background
                                 statistics keep using mask_radius.  Radius <= 0: off */
    int use_priors;           /* 7 "use priors" (refine_priors, frealign.py:3841-3844, :3927) with the statistics of answer 3
                                 (`<name>_stat.cistem`: row 0 = column means, row 1 = column variances over the data set,
                                 src/pyp_main.py:2667-2674): every score the compass search compares is lowered by a Gaussian restraint
                                 sum_i (p_i - mean_i)^2 / (2 var_i n_s) over the REFINED parameters with var_i > 0, angles wrapped to
                                 +-180 degrees, n_s = pi (r_hi^2 - r_lo^2) the in-band samples of the full plane (so the restraint is a
                                 log-prior in the units of LOGP).  SCORE / LOGP / SIGMA stay those of the data term alone.  Build-defined
                                 (the absent program's rule is not visible); 0 = off */
    float prior_mean[5];      /* psi, theta, phi (degrees), x, y (Angstrom) */
    float prior_var[5];       /* their variances (degrees^2, Angstrom^2); <= 0 leaves that parameter unrestrained */
    float res_classification; /* 22 "classification resolution limit" (class_rhcls, frealign.py:3945; default 8 A,
                                 config/pyp_config.toml:5091-5095): LOGP and SIGMA of the output row - what the occupancy update of
                                 3-D classification reads (src/pyp/analysis/occupancies.py:67-252) - are evaluated at the final pose
                                 over res_low .. this limit instead of res_low .. res_high; SCORE stays that of the full band.
                                 0, or a limit beyond res_high = res_high.  ppm_csp_refine ignores it (the csp program has no such
                                 setting) */
} ppm_refine_cfg;

/* Reconstruction settings = numeric answers of the reconstruct3d script (frealign.py:1780-1824). */
typedef struct ppm_recon_cfg {
    int box;
    float pixel_size;
    float res_limit;        /* reconstruction resolution limit, Angstrom (caller passes 2*pixel) */
    float score_weight_bfactor; /* "weighting factor" refine_bsc, A^2 per score unit; 0 = off */
    float score_average;    /* mean SCORE used by the weighting (from <name>_stat.cistem or the rows) */
    float score_threshold;  /* rows with SCORE below it are skipped (caller passes 0) */
    int normalize;
    int invert;
    int split_by_pind;      /* 1: half = PIND parity, 0: half = POSITION_IN_STACK parity */
    float mask_radius;      /* outer radius for the normalisation statistics, Angstrom */
    /* data-driven dose weighting (the five-line answer of frealign.py:1731-1753): a row of exposure t = TIND is attenuated by
     * q_t ^ (dose_exponent min(1, (s / (dose_transition s_Nyquist))^2)), q_t = dose_weights[t] in (0, 1] (the exposure's mean
     * score over the best exposure's, src/pyp/inout/metadata/core.py:3039-3075); exposures beyond the table or with
     * q <= 0 are not attenuated.  NULL / 0 = off. */
    const float *dose_weights; int n_dose_weights;
    float dose_exponent;    /* "fraction" answer (x frames per exposure when "multiply" is yes); larger = fewer exposures at high resolution */
    float dose_transition;  /* fraction of Nyquist at which the full attenuation is reached (0 = 1) */
} ppm_recon_cfg;

typedef struct ppm_final_cfg {
    float molecular_mass_kda;
    float inner_radius;     /* Angstrom */
    float outer_radius;     /* Angstrom */
    float mask_falloff;     /* Angstrom (default 10) */
} ppm_final_cfg;

/* Constrained refinement of tilt-series particles (the `csp` program, src/pyp/system/local_run.py:306-467 argv,
 * mode list src/pyp/align/core.py:1015-1023): every projection row belongs to one particle (PIND) and one tilt (TIND, RIND);
 * its pose is not free but follows from the particle's 3-D pose and the tilt geometry (the relation the reference states in
 * csp_euler_angles, src/pyp/analysis/geometry/core.py:1081-1213):
 *     M_row = E(-ppsi, -ptheta, -pphi) Ry(-tilt_angle) Rz(tilt_axis),   E = Rz(phi) Ry(theta) Rz(psi)
 *     (shx, shy) = [Rz(-tilt_axis) Ry(tilt_angle) (-pshift)]_xy + (tshift_x, tshift_y)            (pixels)
 * A unit (particle or tilt) is scored by the mean score of its rows. */
enum { PPM_CSP_PARTICLES = 1, PPM_CSP_MICROGRAPHS = 2 };
#define PPM_NPCOL 12 /* particle block columns of _extended.cistem (cistem_star_file.py:247): PIND, shift x y z, psi theta phi,
                        x y z position 3-D, score, occ */
#define PPM_NTCOL 6  /* tilt block columns (:248): TIND, RIND, shift x y, angle, axis */
typedef struct ppm_csp_cfg {
    int unit;               /* PPM_CSP_PARTICLES (csp modes 1 / 2 / 5) or PPM_CSP_MICROGRAPHS (modes 0 / 3 / 6) */
    int refine_rotation;    /* particles: the three rotations (about the specimen x, y, z axes); tilts: tilt angle and tilt-axis angle */
    int refine_translation; /* particles: the 3-D shift; tilts: the two image shifts */
    float tol_angle[3];     /* search bound either side of the start, degrees (csp_ToleranceParticlesPsi / Theta / Phi ->
                               specimen x / y / z; tilts: [0] csp_ToleranceMicrographTiltAngles, [1] ...TiltAxisAngles) */
    float tol_shift;        /* the same for shifts, pixels (csp_ToleranceParticlesShifts / csp_ToleranceMicrographShifts) */
    float step_tolerance;   /* smallest compass step, degrees / pixels (csp_OptimizerStepTolerance; default 0.01) */
    int max_iterations;     /* compass iterations; 0 = until the step falls below step_tolerance, at most 12 */
    int tind_min, tind_max; /* rows with TIND outside do not enter a unit's score (csp_UseImagesForRefinementMin / Max; max < 0 = no limit) */
    int first, last;        /* units to refine: PIND (particles) or TIND (tilts) in first..last; last < 0 = up to the end */
    /* csp mode 4 (tilts only; excludes the geometric parameters): one defocus offset per tilt, -range .. +range in steps, added
     * to DEFOCUS_1 and DEFOCUS_2 of all its rows; the offset with the best mean score of the usable rows wins (the unshifted
     * values on ties, then the lower offset) */
    int refine_defocus;
    float defocus_range;    /* csp_ToleranceMicrographDefocus1, Angstrom */
    float defocus_step;     /* Angstrom (default 50); at most PPM_MAX_DEFOCUS_STEPS either side */
    /* Exhaustive particle search (csp_NumberOfRandomIterations, "number of points to evaluate during reference-based exhaustive
     * search"; particles only - tilt units and mode 4 never search exhaustively).  0 = the compass search from the start pose alone.
     * > 0: a budget of (rotation, shift) grid points per particle.  The grid (build-defined; pyp_amd/csrc/ppm_csp_search.h, DESIGN.md
     * section 8) covers the tolerance box about the start pose at the finest step D of {30, 24, 20, 18, 15, 12, 10, 9, 8, 7.5, 6, 5, 4, 3,
     * 2.5, 2, 1.5, 1} degrees whose point count stays inside the budget; every point is scored on a coarse band, the best shift of
     * each rotation is kept, the search_candidates best rotations are refined by two compass iterations each (first steps D / 2 and
     * h_s / 2, bounds +-D / +-h_s about the candidate) and the best of them by the compass search from D / 4 and h_s / 4 down to
     * step_tolerance.  The result may therefore leave the tolerance box, by at most one and a quarter grid steps (D degrees, h_s =
     * mask radius x D pi / 180 pixels).  A budget too small for the 30 degree grid, even without its shifts, skips the stage
     * (ppm_refine_note() says so).  Negative values are refused (-22). */
    int search_points;
    int search_candidates;  /* rotations per particle that go on to the compass passes: 0 = 8, at most 32 */
} ppm_csp_cfg;

/* The plan of the exhaustive particle search (ppm_csp_search_plan). */
typedef struct ppm_csp_search_info {
    int active;             /* 0: no exhaustive stage (search_points = 0, tilt units, mode 4, or a budget below the 30 degree grid) */
    int shift_grid;         /* 0: the single shift 0 (translations off, or dropped because 30 degrees did not fit with it) */
    double step;            /* D, degrees */
    double r_g;             /* coarse band, Fourier pixels */
    double h_s;             /* shift grid step the rule asks for, pixels (the grid itself spans exactly +-tol_shift) */
    double tol_shift;       /* pixels */
    int n_angle[3];         /* angles about the specimen x, y, z axes */
    int full_turn[3];       /* the axis takes n_angle equally spaced angles from 0 over the full turn */
    int n_shift_axis;       /* points per shift axis */
    long n_rot, n_shift;    /* n_angle[0] n_angle[1] n_angle[2]; n_shift_axis^3 */
    int n_candidates;       /* K */
} ppm_csp_search_info;

#define PPM_STATS_COLS 7 /* shell, resolution A, ring radius, FSC, part-FSC, part-SSNR, rec-SSNR
                            (src/pyp/postprocess/core.py:203-221; frealign.py:2559) */

typedef struct ppm_ref ppm_ref_t;
typedef struct ppm_accum ppm_accum_t;

/* kernels whose device time the library accumulates when profiling is on */
enum { PPM_K_PREP = 0, PPM_K_BANK = 1, PPM_K_GLOBAL = 2, PPM_K_TOPK = 3, PPM_K_LOCAL = 4,
       PPM_K_INSERT = 5, PPM_K_FINAL = 6, PPM_K_EXTRACT = 7, PPM_K_NORMS = 8, PPM_K_COUNT = 9 };

int ppm_init(int device);
const char *ppm_last_error(void);
const char *ppm_version(void);
const char *ppm_build_id(void);       /* changes with every build of the library: a resident server and its clients compare it */
int ppm_device_mem_info(size_t *free_bytes, size_t *total_bytes);       /* of the library's device (hipMemGetInfo) */

/* vol: n*n*n floats, x fastest. max_band_px: largest Fourier radius (pixels) any later call will
 * use with this reference (<= n/2). */
ppm_ref_t *ppm_reference_create(const float *vol, int n, float max_band_px);
/* The same with the "padding factor" answer (refine_iblow, frealign.py:3962): the reference is zero-padded to (pad n)^3 before
 * its transform, which is then sampled pad times finer (smaller interpolation error).  pad = 1, 2 or 4, pad n <= 512. */
ppm_ref_t *ppm_reference_create_padded(const float *vol, int n, float max_band_px, int pad);
/* ... and with the "use statistics" answer (6, frealign.py:3903-3910): ring_weight[k], k = 0 .. n_weight-1, multiplies the
 * transform at |k| Fourier pixels of the unpadded box (linear interpolation; the last value beyond the table); NULL = none. */
ppm_ref_t *ppm_reference_create_weighted(const float *vol, int n, float max_band_px, int pad, const float *ring_weight, int n_weight);
void ppm_reference_destroy(ppm_ref_t *ref);

/* images: n_img * box * box floats. images_on_device != 0 means `images` is a device pointer.
 * rows_in / rows_out: n_img * PPM_NCOL doubles (host).  Image i belongs to row i. */
int ppm_refine_batch(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const void *images,
                     int images_on_device, int n_img, const double *rows_in, double *rows_out);
/* per particle, for the roofline's algorithmic byte count: orientations of the global grid, local score
 * evaluations, in-band samples S(r_search) of one grid orientation, and the in-band sample counts summed
 * over all local evaluations (frequency marching makes early ones cheaper) */
int ppm_refine_last_counts(ppm_ref_t *ref, long *n_global, long *n_local, long *samples_global,
                           long *samples_local);
/* After ppm_csp_refine: grid points per particle of the exhaustive stage (n_rot x n_shift; 0 without one - ppm_csp_search_plan gives
 * the factors and K), sweeps (k_csp_eval launches), in-band samples of the full band, gathered samples per projection summed over
 * the sweeps (the exhaustive stage gathers n_rot x S(r_g) per usable row of a searched particle).  After ppm_sva_align: grid rotations of a global search, sweeps (k_sva_eval launches), samples of the band (half space,
 * before the missing wedge), band samples x gathered rotations per sub-volume summed over the sweeps. */
/* remarks of the last ppm_refine_batch on this reference that the caller should log (e.g. the search band was capped);
 * "" if none */
const char *ppm_refine_note(ppm_ref_t *ref);
/* Sections of the last ppm_refine_batch's grid search on this reference, 0 when it had none.  The search builds and searches its slice
 * banks one section of the orientation grid at a time (contiguous ranges of grid directions) where the banks of the whole grid would
 * pass 4 GB on the transform path or their share of the device's memory; the result does not depend on the sectioning.  With more
 * than one section ppm_refine_note() says so. */
int ppm_refine_last_sections(ppm_ref_t *ref);
/* Whether the last ppm_refine_batch on this reference ran the refinement of a chunk's hits on a second stream beside the grid search of
 * the next chunk: the number of hit-stage blocks a compute unit takes beside one block of the search, 0 when the call kept the serial
 * order (one chunk, a search by transform, tiles or sections, no grid search, no room on a compute unit, or PPM_REFINE_OVERLAP=0).
 * The result does not depend on it. */
int ppm_refine_last_overlap(ppm_ref_t *ref);
/* Tap reuse in the full-band local refinement of the last ppm_refine_batch on this reference, counted only while the environment has
 * PPM_LOCAL_REUSE_COUNT=1 (both 0 otherwise): the cube gathers its compass sweeps made for the angular neighbours of a pose, one per
 * lane and in-list sample, and how many of them took the centre pose's taps instead of addressing the cube (0 with
 * PPM_LOCAL_REUSE=0).  The result does not depend on either. */
int ppm_refine_last_reuse(ppm_ref_t *ref, long *gathers, long *reused);

/* refine3d answers 8 / 43 "matching projections" (frealign.py:3929-3931, refine_fmatch): out[i] (box * box floats, host) = the
 * reference projected at row i's pose, times the row's CTF, moved to the row's X / Y shift and band-limited at cfg->res_high — the
 * noise-free model of the stored particle image (negated when cfg->invert is set, so that it overlays the stack as stored). */
int ppm_match_projections(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const double *rows, int n_rows, float *out);

/* Constrained refinement: rows (n_proj x PPM_NCOL, image i belongs to row i), particles (n_part x PPM_NPCOL) and tilts
 * (n_tilt x PPM_NTCOL) are read and updated in place: refined units get their parameters, their rows get the poses that
 * follow from them (angles from M_row, shifts moved by the change of the geometric shift) and SCORE / LOGP / SIGMA at the
 * full band; rows of units outside first..last are left untouched.  cfg gives box, pixel, mask radius, resolution limits
 * and band_factor as in ppm_refine_batch (its search fields are ignored). */
int ppm_csp_refine(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const ppm_csp_cfg *csp, const void *images, int images_on_device,
                   int n_proj, double *rows, double *particles, int n_part, double *tilts, int n_tilt);
/* The plan ppm_csp_refine would follow for csp->search_points (pure host: no device, no reference needed). */
int ppm_csp_search_plan(const ppm_refine_cfg *cfg, const ppm_csp_cfg *csp, ppm_csp_search_info *out);
/* What the ranking stage of the last ppm_csp_refine on this reference kept for the particle with identifier `unit` (PIND): its best
 * rotations in rank order (ties to the lower index) with the best shift of each (ties to the lower index) and that point's score on
 * the coarse band, in SCORE units (100 x the mean correlation of the particle's usable rows).  Indices as ppm_csp_search.h
 * enumerates them: rotation (ia n_b + ib) n_c + ic, shift (ix n + iy) n + iz.  Returns the number of entries written (<= max_k),
 * 0 for a particle that was not searched, negative on error. */
int ppm_csp_search_candidates(ppm_ref_t *ref, long unit, int max_k, long *rot_index, long *shift_index, double *score);

/* Movie-frame refinement (the `csp` program with its refine-frames flag, src/pyp/system/local_run.py:330-376; csp_frame_refinement,
 * config/pyp_config.toml:6473-6478): one shift per frame row from score maps pooled over the neighbouring frames.  Build-defined
 * (DESIGN.md section 8).  A GROUP is the set of rows with equal (PIND, TIND), ordered by FIND; a = pixel size, N = box.
 *   own map   S_r(d) = the local score of ppm_refine_batch at row r's pose and defocus with its shift moved by d, ALL RINGS SIGNED
 *             (cfg->res_signed_cc is ignored), over res_low .. res_high, for d = (jx, jy) h, |jx|, |jy| <= W, stored row-major (jy, jx)
 *   grid      h = step_px (0 = 0.5 pixel), W = min(ceil(range_px / h - 1e-6), PPM_FRAME_MAX_STEPS); a range that is cut sets
 *             info->clipped and ppm_refine_note() says so
 *   pooled    P_r(d) = sum g(FIND_r' - FIND_r) S_r'(d) / sum g over the rows r' of r's group with OCCUPANCY > 0 and |FIND_r' - FIND_r| <=
 *             half_width, g(D) = exp(-D^2 / (2 (half_width / 2)^2)), added in ascending FIND; half_width 0: P_r = S_r
 *   peak      the arg-max of P_r in row-major order, ties to the lower index; per axis, where the arg-max is not on the window's edge and
 *             l - 2c + r < 0 for its two neighbours l, r, plus (l - r) / (2 (l - 2c + r)) h.  The result is delta_r, pixels
 *   groups with TIND in first..last (last < 0: to the end) AND in tind_min..tind_max (tind_max < 0: no limit): X_SHIFT, Y_SHIFT, FSHIFT_X and
 *             FSHIFT_Y all move by delta_r a; SCORE = 100 S_r at the arg-max grid point; LOGP and SIGMA stay
 *   groups in first..last outside tind_min..tind_max are scored only: SCORE = 100 S_r(0), nothing else changes
 *   rows with OCCUPANCY <= 0, and rows of other groups, are returned unchanged and enter no pool
 * rows / rows_out: n_rows x PPM_NCOL doubles (host), image i belongs to row i; the rows may come in any order and a call may hold any
 * subset of the groups: a group's result depends on its own rows alone.  own_maps / pooled_maps (NULL: not wanted): n_rows x (2W + 1)^2
 * floats on the host, zeros for rows without a map.  Refused with -22: a FIND that occurs twice in a group, step_px < 0, range_px <= 0,
 * half_width < 0. */
#define PPM_FRAME_MAX_STEPS 8
typedef struct ppm_frame_cfg { float range_px, step_px; int half_width, tind_min, tind_max, first, last; } ppm_frame_cfg;
/* groups with a usable row; slices gathered (one per set of frames of a group with bit-identical PSI, THETA, PHI, DEFOCUS_1, DEFOCUS_2,
 * DEFOCUS_ANGLE, PHASE_SHIFT); rows whose shifts moved; rows scored only; rows returned unchanged; W; h; W h; whether the range was cut */
typedef struct ppm_frame_info { long groups, models, rows_refined, rows_scored, rows_skipped; int n_steps; float step_px, range_px; int clipped; } ppm_frame_info;
int ppm_frame_refine(ppm_ref_t *ref, const ppm_refine_cfg *cfg, const ppm_frame_cfg *fcfg, const void *images, int images_on_device,
                     const double *rows, int n_rows, double *rows_out, float *own_maps, float *pooled_maps, ppm_frame_info *info);
/* The grid ppm_frame_refine would use (pure host; any output may be NULL); the same refusals. */
int ppm_frame_plan(const ppm_frame_cfg *fcfg, float *step_px, int *n_steps, int *clipped);

/* Sub-tomogram alignment (3DAVG, `external/TOMO/MPI_Classification`, driven by src/pyp/refine/tomo_avg/sub_tomo_avg.py:318-555
 * with the XML protocols of src/pyp/refine/3DAVG/): every sub-volume is aligned to the reference by a rotation + 3-D shift that
 * maximise the band-passed, missing-wedge-weighted normalised cross-correlation of its 3-D transform with the rotated
 * reference transform.  Pose convention = the particle block of constrained refinement: the sub-volume's transform at k
 * matches the reference's at N k, times e^{+2 pi i k.p / box} (N = E(-ppsi, -ptheta, -pphi), p = particle shift), so a refined
 * pose can be written straight into a particle's (ppsi, ptheta, pphi, shift) and vice versa. */
typedef struct ppm_sva_cfg {
    int box; float pixel_size;
    float window[3];        /* <mode>_image_window_x/y/z: half-axes of the real-space window, pixels (0 = none) */
    float window_sigma;     /* <mode>_image_window_sigma: Gaussian fall-off outside the window, pixels */
    float highpass_cutoff, highpass_decay, lowpass_cutoff, lowpass_decay;   /* <mode>_high/low_pass_cutoff/decay, cycles per pixel (Nyquist = 0.5) */
    int use_missing_wedge;  /* metric/use_missing_wedge: samples outside the tilt range lwedge..uwedge do not count */
    float tol_angle;        /* <mode>_out_of_plane_search_range: search bound either side of the start, degrees (all three rotations) */
    float tol_shift;        /* <mode>_shifts_tolerance, pixels */
    float step_tolerance;   /* smallest compass step (default 0.05 degrees / pixels) */
    int max_iterations;     /* 0 = until the step falls below step_tolerance, at most 12 */
    float band_factor;      /* frequency marching like the band_factor field of the refinement settings (0 = default 3, < 0 = off) */
    int search_mode;        /* metric/alignment_mode of the protocol (iteration_002_mode_3.xml:29-38).  0 = rotation and translation REFINEMENT
                               within the tolerances (the protocol's mode 1); 1 = GLOBAL rotation and translation search (the protocol's
                               mode 0): the start rotation times every rotation of a grid of step `global_step` over the whole of SO(3)
                               (theta_i = 180 i / (n - 1), n_phi = round(360 sin theta / step), n_psi = round(360 / step)) is ranked by the
                               correlation of the AMPLITUDES |F(k)| and |Ref(N k)| - a shift only moves phases, so the ranking does not
                               depend on how well the sub-volume is centred - on the coarse band the step allows (frequency marching with
                               probe Delta / 2); the `n_candidates` best rotations get two compass iterations each from the start shift
                               (first steps Delta / 2 and tol_shift / 2; bounds +-step about the grid rotation, +-tol_shift about the start
                               shift), and the best of them at the full band is refined again from Delta / 4 and tol_shift / 4 down to
                               step_tolerance; 2 = translation only (the protocol's mode 2).
                               Build-defined: the absent program ranks peaks of a spherical-harmonics correlation instead */
    float global_step;      /* degrees; 0 = 15 */
    int n_candidates;       /* metric/number_of_candidate_peaks_to_search; 0 = 25, at most 64 */
    char symmetry[8];       /* point group of the reference, read by search_mode 1 only: "" (= "C1"), "Cn", "Dn", "T", "O", "I" - the symbols of
                               ppm_refine_cfg.symmetry (<mode>_use_symmetrization n of the protocol -> "Cn"); an unknown symbol or one of more
                               than 60 operators returns -22.  With more than one operator the grid is cut to the group's asymmetric unit
                               (phi < phi_max, theta <= theta_max as for ppm_refine_cfg: theta_i = theta_max i / (n - 1), n_phi =
                               round(phi_max sin theta / step), phi_j = phi_max j / n_phi, psi unchanged) and the candidates are G N0 instead
                               of N0 G: pose N is equivalent to S N for every operator S (F_v(k) = Ref(N k), Ref(S x) = Ref(x)), so the cut
                               has to act on the left; the grid holds one copy of every peak instead of n, and ppm_refine_last_counts
                               reports its size.  "" / "C1": the full grid and N0 G, bit for bit as before.  The reference is used as
                               given (it is not symmetrised here); the average is symmetrised by the ACCUMULATOR's symbol (ppm_sva_insert).
                               Build-defined: the absent MPI_Classification's own rule is not visible */
} ppm_sva_cfg;
/* volumes: n_vol * box^3 floats (x fastest); wedges: n_vol x {lwedge, uwedge} tilt limits in degrees (tilt axis = y);
 * poses: n_vol x 12 doubles {N row-major (9), shift x y z (pixels)}, start values in, refined values out; scores: n_vol. */
int ppm_sva_align(ppm_ref_t *ref, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol, const float *wedges,
                  double *poses, double *scores);

/* symmetry: "C1", "Cn", "Dn", "T", "O", "I".  ext_device_buffer: NULL, or a device buffer of
 * ppm_accum_floats(box) floats the caller allocated (e.g. a torch tensor, so that RCCL can
 * reduce it in place); it must be zeroed by the caller. */
size_t ppm_accum_floats(int box);
ppm_accum_t *ppm_accum_create(int box, float pixel_size, const char *symmetry,
                              void *ext_device_buffer);
void ppm_accum_destroy(ppm_accum_t *acc);
int ppm_insert_batch(ppm_accum_t *acc, const ppm_recon_cfg *cfg, const void *images,
                     int images_on_device, int n_img, const double *rows);
/* host copies of the accumulators: ppm_accum_floats(box) floats laid out
 * [half 0..1][kz][ky][kx 0..box/2]{re, im, weight} */
int ppm_accum_download(ppm_accum_t *acc, float *host);
/* `count` floats from float index `first` of the same layout (one half map = ppm_accum_floats(box) / 2 floats): lets a caller
 * download each half into a page-locked buffer of its own and write the two dump files (frealign.py:1820-1822) from there */
int ppm_accum_download_range(ppm_accum_t *acc, float *host, size_t first, size_t count);
int ppm_accum_add(ppm_accum_t *acc, const float *host);
long ppm_accum_count(ppm_accum_t *acc, int half); /* particles inserted so far */
void ppm_accum_set_count(ppm_accum_t *acc, int half, long count);

/* Multi-GPU reconstruction: every rank (one process per GPU) inserts its particle shard into its own accumulator;
 * ONE sum over the ranks replaces the dump files + local_merge3d + the summation of merge3d (frealign.py:1838-1903, :2075-2093).
 * ppm_accum_reduce sums the accumulator (ppm_accum_floats(box) floats, in place on the device) and the two particle counters over
 * the communicator with RCCL on the library's stream: root >= 0 -> ncclReduce to that rank, root < 0 -> ncclAllReduce.  `comm` is
 * an ncclComm_t: the caller's own, or one made by ppm_comm_create (rank 0 calls ppm_comm_unique_id and hands the 128 bytes to the
 * other ranks by any means - MPI, a file, torch.distributed - then every rank calls ppm_comm_create; collective, blocks until all
 * ranks have joined).  librccl is opened on first use; if it cannot be, these calls fail with a message (no other transport). */
typedef struct ppm_comm_id { char bytes[128]; } ppm_comm_id; /* = ncclUniqueId */
int ppm_comm_unique_id(ppm_comm_id *id);
void *ppm_comm_create(int n_ranks, int rank, const ppm_comm_id *id);
int ppm_comm_count(void *comm); /* ranks of the communicator as RCCL reports them (ncclCommCount); < 0 on error */
void ppm_comm_destroy(void *comm);
int ppm_accum_reduce(ppm_accum_t *acc, void *comm, int root);

/* Sub-tomogram AVERAGE (BASELINE config 5 is "sub-tomogram averaging": a 3DAVG iteration ends in averaged maps,
 * `<dataset>_iteration_%03d_refined_selected_average_0.mrc` + `..._filtered.mrc`, src/pyp/refine/tomo_avg/sub_tomo_avg.py:79-94,
 * src/pyp_main.py:3076-3100; the next iteration aligns to them): the 3-D analogue of ppm_insert_batch.  Every sub-volume's transform
 * ((v - mean) / sigma, the whole box: no window, no band-pass) is brought into the reference frame by its aligned pose - the
 * convention of ppm_sva_align: F_v(k) = Ref(N k) e^{+2 pi i k.p / box} - and added to the accumulator of the half-map it belongs to
 * (parity of index[v], or of v when index is NULL; odd -> half 1), with its missing-wedge mask as the weight:
 *     num_h(q) += m_v(k) F_v(k) e^{-2 pi i k.p / box} / box,    den_h(q) += m_v(k),    k = N^T q  (trilinear interpolation of F_v)
 * for |q| < box/2 - 1, m_v = 1 where the tilt angle of (k_x, k_z) lies in the sub-volume's lwedge .. uwedge (cfg->use_missing_wedge)
 * and everywhere otherwise.  `acc` = ppm_accum_create(box, pixel, symmetry, ...), and the ACCUMULATOR's symbol decides the average
 * (cfg->symmetry is not read here): with operators S_1 = 1, S_2 .. S_n every sub-volume enters once per operator at the pose
 * (S N, p), i.e. at k = N^T S^T q with the shift phase and the wedge mask taken at that k - operators in order, the batch inside,
 * den_h(q) grows by one per (sub-volume, operator) inside the wedge - which makes the sums invariant under the group (build-defined:
 * the absent MPI_Classification's own rule is not visible); "C1" is the plain average.  ppm_accum_count counts sub-volumes ONCE each,
 * whatever the group; shards on several
 * GPUs are summed with ppm_accum_reduce; ppm_finalize turns the sums into the two half-maps, the FSC-weighted average and the
 * statistics table exactly as for a reconstruction.  Of cfg only box and use_missing_wedge are read.  Build-defined (the absent
 * MPI_Classification's weighting is not visible).  Sub-volumes enter the sums in batches of up to 32 and the counters follow every
 * completed batch: after an error return ppm_accum_count says how many are in the sums (the caller can go on from there or start
 * the accumulator again).  With index == NULL the half-map parity is that of the POSITION IN THIS CALL (plus the call's base in
 * ppm_sva_align_average): callers that split a table into several calls pass the table numbers in `index`. */
int ppm_sva_insert(ppm_accum_t *acc, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol, const float *wedges,
                   const double *poses, const long *index);

/* One pass of a 3DAVG iteration: ppm_sva_align, and every chunk of sub-volumes is added to the average (ppm_sva_insert into `acc`) at
 * its refined pose while it is still in device memory - sub-volumes that live on the host (config 5: 10 k x 192^3 = 283 GB) cross PCIe
 * once per iteration instead of twice.  The calls on `acc` made inside run on the reference's stream: do not use `acc` from another
 * thread meanwhile. */
int ppm_sva_align_average(ppm_ref_t *ref, ppm_accum_t *acc, const ppm_sva_cfg *cfg, const void *volumes, int volumes_on_device, int n_vol,
                          const float *wedges, double *poses, double *scores, const long *index);

/* half1/half2/filtered: box^3 floats each (host).  stats: (box/2) * PPM_STATS_COLS doubles. */
int ppm_finalize(ppm_accum_t *acc, const ppm_final_cfg *cfg, float *half1, float *half2,
                 float *filtered, double *stats);

/* Shape masking of a reference map: the work of frealign_v9.11/bin/apply_mask.exe, which PYP runs on last iteration's map at the
 * top of every refinement iteration (src/pyp/align/core.py:783-856, answers in the order of :788-799).  Build-defined (the binary
 * is absent from the reference checkout):
 *   core = {mask >= 0.5}; d = Euclidean distance in voxels to the nearest core voxel, no wrap-around at the faces of the box;
 *   s    = max(clamp(mask, 0, 1), (1 + cos(pi d / edge_width)) / 2 for d < edge_width, else 0)     (edge_width 0: the clamp alone)
 *   O    = map (filter 0), or the map low-passed in Fourier space (filter 2): 1 up to r_c - e/2 Fourier pixels, a raised cosine to 0
 *          at r_c + e/2, with r_c = n pixel_size / filter_radius_A and e = filter_edge_px (e = 0: a step at r_c)
 *   out  = s map + (1 - s) outside_weight O
 * map, mask, out: n^3 floats, x fastest; on_device != 0: all three are device pointers; out may equal map.  n: 8..512; filter 2
 * needs a box the transforms take (even, 32..512, prime factors 2, 3, 5, 7); edge_width: 0..64.  Anything else returns -22. */
typedef struct ppm_mask_cfg { double pixel_size; int edge_width; double outside_weight;
                              int filter; double filter_radius_A; double filter_edge_px; } ppm_mask_cfg;
int ppm_mask_volume(const void *map, const void *mask, int on_device, int n, const ppm_mask_cfg *cfg, void *out);

/* Binary mask of a map's largest body: the work of frealignx/create_mask, which PYP's masking block runs on the reference before
 * apply_mask.exe (src/pyp/inout/image/core.py:1538-1605, answers in the order of :1548-1555).  Build-defined (the binary is absent
 * from the reference checkout), with c = n / 2 (integer division):
 *   sphere = voxels with integer (x - c)^2 + (y - c)^2 + (z - c)^2 <= (outer_radius_A / pixel_size)^2, the right side in double
 *   L      = map (lowpass_A 0), or the map low-passed in Fourier space: the cosine-edge filter of ppm_mask_volume around
 *            r_c = n pixel_size / lowpass_A Fourier pixels, lowpass_edge_px wide
 *   B0     = sphere and {L >= threshold}, compared in float32; an empty B0 returns -22 and the message holds min / max of L over the sphere
 *   C      = the connected body of B0 under 26-connectivity (faces, edges, corners; no wrap-around) with the most voxels; among equals
 *            the one that holds the smallest linear index (z n + y) n + x
 *   mask   = C (lowpass_A 0), or sphere and {low-passed indicator of C >= rebin}, compared in float32; no second labelling
 * map, mask_out: n^3 floats, x fastest; on_device != 0: both are device pointers; mask_out may equal map; every value written is 0 or 1,
 * and nothing is written when the call is refused.  n: 8..512; lowpass_A != 0 needs a box the transforms take (even, 32..512, prime
 * factors 2, 3, 5, 7) and rebin strictly inside 0..1; pixel_size, outer_radius_A > 0; lowpass_A, lowpass_edge_px >= 0.  Anything else
 * returns -22.  info (may be null): range of L over the sphere, voxels of B0, its bodies, voxels of C, voxels of the mask. */
typedef struct ppm_create_mask_cfg { double pixel_size, outer_radius_A, threshold, lowpass_A, lowpass_edge_px, rebin; } ppm_create_mask_cfg;
typedef struct ppm_create_mask_info { double density_min, density_max; long above, components, largest, mask_voxels; } ppm_create_mask_info;
int ppm_create_mask(const void *map, int on_device, int n, const ppm_create_mask_cfg *cfg, void *mask_out, ppm_create_mask_info *info);

/* Post-processing of the two half maps of the last iteration: the work of PYP's external/postprocessing/postprocessing.py, which the
 * Post-processing block starts (src/pyp_main.py:6601-6865, command line at :6638-6737).  Build-defined (the program is absent from the
 * reference checkout), after Rosenthal & Henderson 2003 and Chen et al. 2013:
 *   mask     none (1 everywhere), external (as given, clamped to 0..1) or automatic: the largest body of (half1 + half2) / 2 at or above
 *            a threshold (ppm_create_mask: outer radius n pixel_size / 2, low-pass automask_lp, re-bin 1/2) with a cosine edge of 6 voxels
 *            (ppm_mask_volume); the threshold is the given value (0), mean + value x standard deviation of the low-passed map over the
 *            sphere (1), or the ceil(value x voxels of the sphere)-th largest low-passed value there (2)
 *   curves   per shell s = floor(|k| + 1/2) = 0 .. n/2: FSC of the halves (U), of the masked halves (Mk), of the masked halves whose phases
 *            were randomised from shell s_r on (Rd), and C = Mk below s_r + 2, (Mk - Rd) / (1 - Rd) from there (0 where 1 - Rd < 1e-6)
 *   s_r      round(n pixel_size / randomize_value) (method 0), or the first shell >= 1 with U < randomize_value (method 1); 1 .. n/2
 *   resolution  where C first falls below 0.143, interpolated linearly in frequency; Nyquist if it never does
 *   filter   W(s) = w(s) exp(-B f^2 / 4) L(s): w = sqrt(2C / (1 + C)) (1 with skip_fsc_weighting, max(C, 0)^2 with apply_fsc2); B none,
 *            ad hoc, or 4 x the slope of ln(sqrt(P) w) against f^2 over 1/fit_low <= f <= 1/fit_high (fit_high 0: the resolution), P the
 *            shell mean of |F1 + F2|^2 / 4 of the masked halves; L a cosine edge two shells wide about the low-pass cutoff (lowpass in A,
 *            0 = none, lowpass_auto: the resolution) and a mirrored one for highpass (<= 0: none), or Gaussians with half amplitude there
 *   outputs  unmasked = Re IFFT(W FFT((half1 + half2) / 2)), masked = mask x unmasked; flip_x/y/z reverse that axis of both
 * half1, half2, mask (NULL unless mask_mode 1), unmasked_out, masked_out, mask_out (or NULL): n^3 floats, x fastest; on_device != 0: all
 * of them are device pointers.  curves: 4 x (n/2 + 1) doubles on the host (U, Mk, Rd, C); shell_count (or NULL): n/2 + 1 longs on the host.
 * n: a box the transforms take (even, 32..512, prime factors 2, 3, 5, 7).  Refused with -22: any other box, both FSC flags, fewer than
 * three shells in the B-factor fit, values out of range; nothing is written then.  Two calls on the same data agree bit for bit. */
typedef struct ppm_post_cfg {
    double pixel_size;
    int mask_mode;                  /* 0 none, 1 external, 2 automatic */
    double automask_lp;             /* A; 0 = no low-pass */
    int threshold_method;           /* 0 intensity, 1 sigma, 2 volume */
    double threshold_value;
    int randomize_method;           /* 0 resolution (A), 1 fsc */
    double randomize_value;
    unsigned seed;
    int bfactor_method;             /* 0 none, 1 ad hoc, 2 automatic */
    double adhoc_bfac, fit_low, fit_high;
    int lowpass_auto;
    double lowpass, highpass;
    int gaussian, skip_fsc_weighting, apply_fsc2, flip_x, flip_y, flip_z;
} ppm_post_cfg;
/* s_r; the first shell with C < 0.143 (0: none); shells of the B-factor fit; complex 3-D transforms run (5 without the automatic mask);
 * resolution in A; B in A^2; threshold of the automatic mask; voxels of the mask at or above 0.5 (automatic: of its body) */
typedef struct ppm_post_info { int s_r, res_shell, fit_shells, transforms; double resolution, bfactor, threshold; long mask_voxels; } ppm_post_info;
int ppm_postprocess(const void *half1, const void *half2, const void *mask, int on_device, int n, const ppm_post_cfg *cfg,
                    void *unmasked_out, void *masked_out, void *mask_out, double *curves, long *shell_count, ppm_post_info *info);

/* Local resolution of two half maps: the work of ResMap (--noguiSplit), which PYP's Post-processing block starts on the half maps once
 * <out>_data.fsc is read (src/pyp_main.py:6815-6844; tabs.sharpen.resmap defaults to true).  Build-defined: the reference checkout holds
 * neither that program nor any output of it, so nothing pins its arithmetic.  After the published idea (Kucukelbir, Sigworth & Tagare
 * 2014): voxel by voxel and resolution by resolution, test whether the local signal at that wavelength stands out of the noise, the
 * noise taken from the difference of the half maps, at the caller's p-value.  DESIGN.md 2e.
 *   inside   voxels with mask > 0.5; without a mask those with |x - c| < n/2, c = (n/2, n/2, n/2); their number n_inside = 0 is refused
 *   levels   lambda_i = lambda_min + i step for all i with lambda_i <= lambda_max, in float64; the device and the map hold them as float32.
 *            step < 0.25 is refused.  lambda_min = min_res, raised to 2.5 pixel_size when below it (0 included; info.notes says so): the
 *            band centre plus two widths stays inside Nyquist.  lambda_max = max_res; 0 means n pixel_size / 6 (band centre six Fourier
 *            pixels out); above n pixel_size / 4 is refused.  No level, or more than 64, is refused.
 *   per level, with s = n pixel_size / lambda Fourier pixels and l = lambda / pixel_size voxels:
 *     band    b(k) = exp(-(|k| - s)^2 / (2 sb^2)), sb = max(s / 8, 1.5), b(0) = 0
 *     window  W(k) = exp(-2 pi^2 sw^2 |k|^2 / n^2), sw = max(l, 2) / 2
 *             k: signed indices in [-n/2, n/2) per axis; both are tables over the integer |k|^2 (3 (n/2)^2 + 1 entries), made in float64
 *             with the transforms' 1 / n^3 folded in and rounded once to float32
 *     A = (half1 + half2) / 2, D = (half1 - half2) / 2 in float32; A_l = IFFT(b FFT A), D_l likewise;
 *     E_A = Re IFFT(W FFT(A_l^2)), E_D likewise from D_l^2 (cyclic convolutions)
 *     tau     the r-th smallest E_D over the inside voxels, r = ceil((1 - p) n_inside) clipped to 1 .. n_inside: an exact order statistic
 *             (non-negative float32 bits order like unsigned integers; a negative value counts as 0)
 *     a voxel passes the level when it is inside and E_A > tau
 *   map      levels run from the coarsest to the finest; a voxel is alive at first when it is inside, stays alive while it passes, and
 *            takes the lambda of the last level at which it was alive; every other voxel keeps 100.0 (outside, or failed the coarsest
 *            level).  No multiple-testing correction: the continuity rule keeps the chance hits of a fine level off the solvent.
 * Both maps ride one complex array Z = A + i D (a real radial filter acts on both, squaring after the inverse transform keeps them
 * apart): 1 + 3 L complex transforms for L levels.  Integer atomics only: two calls on the same data agree bit for bit.
 * half1, half2, mask (or NULL), out_res: n^3 floats, x fastest; on_device != 0: device pointers, level_maps included.
 * keep_levels (a debug output, 0 = off): the number of levels level_maps has room for, n^3 pairs (E_A, E_D) of floats each, finest level
 * first; fewer than the grid holds is refused.  n: a box the transforms take (even, 32..512, prime factors 2, 3, 5, 7).  Refusals return
 * -22 and write nothing. */
#define PPM_LOCRES_MAX_LEVELS 64
#define PPM_LOCRES_UNASSIGNED 100.0f
typedef struct ppm_locres_cfg { double pixel_size, p_value, min_res, max_res, step; int keep_levels; } ppm_locres_cfg;
/* levels (ascending, as float32), tau per level, voxels whose value is that level, inside voxels, those left at 100, the median of the
 * map over the inside voxels (the ceil(n_inside / 2)-th smallest), complex 3-D transforms run, notes (what was adjusted; may be empty) */
typedef struct ppm_locres_info {
    int n_levels, transforms;
    long n_inside, unassigned;
    double median;
    float levels[PPM_LOCRES_MAX_LEVELS], tau[PPM_LOCRES_MAX_LEVELS];
    long counts[PPM_LOCRES_MAX_LEVELS];
    char notes[256];
} ppm_locres_info;
int ppm_local_resolution(const ppm_locres_cfg *cfg, const void *half1, const void *half2, const void *mask, int on_device, int n,
                         void *out_res, void *level_maps, ppm_locres_info *info);

/* Fourier resampling and real-space resizing of maps and image stacks: the work of cistem2's `resample` and `resize`, which PYP runs on the
 * initial model (src/pyp/preprocess/core.py:762-793 through src/pyp/system/wrapper_functions.py:14-122), and of frealign_v9.11's
 * resample_mp.exe, which Fourier-bins particle stacks (src/pyp/analysis/image.py:71-147, :209-248).  DESIGN.md section 2f defines both:
 *   resample  per axis, with X the unnormalised DFT of a line of n_in samples, K = min(n_in, n_out), h = K / 2: Y[k mod n_out] = X[k mod n_in]
 *             for |k| < h; the Nyquist term of the smaller grid Y[h] = X[h] + X[n_in - h] (n_out < n_in) or Y[h] = Y[n_out - h] = X[h] / 2
 *             (n_out > n_in); all else 0; y = (1 / n_in) IDFT(Y).  Sample 0 stays sample 0, the mean is kept.  Both sizes must be ones the
 *             transforms take (even, 32..512, prime factors 2, 3, 5, 7); the refusal names the nearest such sizes.
 *   resize    out[i] = in[i - n_out / 2 + n_in / 2] per axis where that lies inside the input, elsewhere the pad value: the mean of the voxels
 *             on the six faces of a volume (the four edges of an image, per image), every voxel once, summed in double in a fixed order
 *             (no floating-point atomics: two calls agree bit for bit).  normalize != 0: the mean of the item is subtracted and the result
 *             divided by its standard deviation first (both in double, over all voxels); a deviation of 0 is refused.  Sizes 8..512.
 *             pad_values (host memory, may be NULL): the pad value of every item as written.
 * dims: 2 = n_items square images, 3 = n_items cubic volumes, x fastest, items one after the other.  on_device != 0: src and dst are
 * device pointers.  Host stacks of any length pass through the device in chunks sized from its total memory.  Refusals return -22 and
 * write nothing to dst. */
int ppm_resample(const void *src, int on_device, int dims, long n_items, int n_in, int n_out, void *dst);
int ppm_resize(const void *src, int on_device, int dims, long n_items, int n_in, int n_out, int normalize, void *dst, float *pad_values);
/* Fitting a reference of n_in voxels at pixel_in to a box of box_out voxels at pixel_out: s = pixel_in / pixel_out,
 * n_c = min(n_in, 2 ceil(box_out / (2 s)) + 2) is what the output box can show; among the sizes P >= n_c and M the transforms take the
 * pair with the smallest rel_error = |M / (P s) - 1| is chosen (ties: the smaller P M, then the smaller P); the map is resized n_in -> P,
 * resampled P -> M and resized M -> box_out.  pixel_achieved = pixel_in P / M is what the output header should carry.  A rel_error above
 * 0.01 (the caller's own tolerance, preprocess/core.py:810-812) is refused with the best pair in the message; `out` of the plan is filled
 * in either case.  The plan needs no device and no initialised library; the volume call fills pad_value_1 / pad_value_2 (the pad values of the two resizes) too. */
typedef struct ppm_fit_info {
    int n_in, box_out, n_c, P, M;
    double scale, pixel_achieved, rel_error, pad_value_1, pad_value_2;
} ppm_fit_info;
int ppm_fit_plan(int n_in, double pixel_in, double pixel_out, int box_out, ppm_fit_info *out);
int ppm_fit_volume(const void *vol, int on_device, int n_in, double pixel_in, double pixel_out, int box_out, void *out, ppm_fit_info *info);

/* The averaged periodogram of a micrograph or a movie: the spectrum stage of cistem2's `ctffind`, which PYP runs per micrograph, per
 * tilt and per particle (src/pyp/ctf/core.py:130-468, :471-600, :715-787).  DESIGN.md section 2g defines it; it is pinned to the
 * reference's own plain-numpy `periodogram_averaging` (ctf/core.py:1216-1337, power 2, binning 1):
 *   tiles     T x T, origins 0, T/2, 2 T/2, ... along each axis (n / (T/2) of them, integer division), an origin whose tile would leave
 *             the image pulled back to n - T; where T/2 divides n the last tile therefore repeats the one before it and counts twice,
 *             as it does there.  The image need not be square; an axis shorter than T is refused.
 *   movie     nframes > 1: frames are averaged in groups of `group` (in order; the last group holds what is left) and every group's
 *             mean image is tiled; the average runs over the tiles of all groups.
 *   power     |rfft2(tile)|^2 (unnormalised transform), averaged over the tiles: T rows (ky = 0 .. T-1 in transform order) of T/2 + 1
 *             values (kx = 0 .. T/2), floats, kx fastest.
 *   normalise != 0: the reference's own scaling - element [0, 0] set to 0, then everything divided by the maximum (an image whose
 *             tiles are all constant gives 0 / 0 there and here).
 *   order     tiles are summed in walk order (group, tile row, tile column) in chunks of 16, the chunks' partial sums in order: the
 *             order depends on the sizes alone, no floating-point atomics, two calls agree bit for bit.
 * T must be a size the transforms take (even, 32..512, prime factors 2, 3, 5, 7); the refusal names the nearest such sizes.  The handle
 * owns the workspaces, sized by the plan before the first launch (ppm_ctf_spectrum_plan reports them; it needs no device and no
 * initialised library); a workspace that cannot be had refuses the call.  on_device != 0: img is a device pointer; out_on_device
 * likewise for out_power, which may be NULL: the result also stays in the handle, where ppm_ctf_last_power finds it (a device pointer,
 * valid until the handle's next call), so that a later stage can read it without a trip through the host.  Refusals return -22 and
 * write nothing. */
typedef struct ppm_ctf ppm_ctf_t;
typedef struct ppm_ctf_spectrum_info {
    int tile, half_w, tiles_x, tiles_y, groups, vec;       /* vec: the sizes allow 16-byte loads (the image's address must too) */
    long tiles, chunks, pass_tiles;                        /* tiles averaged, partial sums, tiles per trip through the two passes */
    long half_bytes, part_bytes, out_floats;               /* the two workspaces and the size of the result */
} ppm_ctf_spectrum_info;
ppm_ctf_t *ppm_ctf_create(void);
void ppm_ctf_destroy(ppm_ctf_t *h);
int ppm_ctf_spectrum_plan(int nx, int ny, int nframes, int group, int tile, ppm_ctf_spectrum_info *out);
int ppm_ctf_spectrum(ppm_ctf_t *h, const void *img, int on_device, int nx, int ny, int nframes, int group, int tile, int normalise,
                     void *out_power, int out_on_device);
const void *ppm_ctf_last_power(ppm_ctf_t *h);

/* Defocus and astigmatism from power spectra: the estimator of DESIGN.md section 2g (build-defined: the program it stands in for is
 * absent; tests/f64_ctf.py is its executable form).  Per spectrum [T][T/2 + 1] as ppm_ctf_spectrum leaves it (normalised or not: the
 * score does not see the scale):
 *   crop      a pixel below 1.4 A: the spectrum is centre-cropped in Fourier space to B = 2 floor(T pixel / 1.4 / 2), a = pixel T / B;
 *             else B = T, a = pixel
 *   condition A = sqrt(P); mean of A over integer rings r = floor(|k| + 1/2) <= B/2 of the half plane; background = that profile
 *             box-averaged over +- ceil(B a / min_res) rings (ring 0, the image's mean, left out); samples = half-plane pixels with min_res >= 1/s >= max_res inside ring
 *             B/2, kx = 0 with ky < 0 dropped; v = A - background(ring) - mean over the samples (sums in double)
 *   score     sum v |c| / sqrt(sum v^2 sum c^2) - (D / tol)^2 / (2 n) (the last term with tol > 0 only), c the CTF of ppm_refine_batch
 *             (same wavelength, Cs and amplitude-contrast phase) at mean defocus d, astigmatism D = df1 - df2 >= 0 and angle t
 *   grid      d = lo, lo + step, ... <= hi; D = 0, step, ... up to tol (or 1000 A without a restraint); 12 angles of 15 degrees for
 *             every D > 0; candidate index = i_d (1 + 12 n_D) + c, c = 0 for D = 0, else 1 + 12 (j_D - 1) + k_t; ties to the lowest index
 *   search    from the grid winner: steps (step, step, 15 degrees); per level at most 8 sweeps over the six neighbours (D kept >= 0, t
 *             fixed while D = 0), a move only to a strictly better score (ties to the first neighbour in the order +d -d +D -D +t -t);
 *             the steps are halved 10 times
 * out_rows: n x 8 doubles {df1 >= df2, angle in (-90, 90] degrees, score, grid winner's index, its score, samples fitted, fit resolution
 * in A}.  avrot (host, may be NULL): n x 6 x (B/2 + 1) doubles, per ring r: frequency r / (B a) in 1/A; rotational average of A -
 * background; the same averaged along equiphase lines (a pixel counts for ring floor(|k| sqrt(df(phi) / d) + 1/2)); the fitted 1-D |CTF|
 * at mean defocus; quality = correlation of the last two over the rings r +- ceil(B a / min_res) inside 1 .. B/2; noise level = 1 /
 * sqrt(pixels of that window).  The fit resolution is 1 / s of the first ring beyond min_res whose quality is below 0.5 (of the last
 * ring when none is).  diag (host, may be NULL): n x B x B floats, centred: the conditioned spectrum where kx >= 0, the fitted |CTF|
 * (with astigmatism) where kx < 0.  All of it in double on the device (k_ctf_profile).  def_lo / def_hi (host, both or neither): a window [lo, hi] per spectrum in place of cfg's; when all are the
 * same a block scores one |c| against four spectra, which changes no spectrum's bits.  grid_scores (host, may be NULL): the whole
 * score map, grid_ld floats per spectrum (a debug output; NaN past the candidates of a spectrum whose window is shorter than the longest).  spectra: n spectra one after the other; on_device != 0: a device pointer
 * (ppm_ctf_last_power's, for one).  ppm_ctf_estimate runs both stages on one image without a trip through the host.  No floating-point
 * atomics: a spectrum's result is bit-identical whatever the batch around it.  Refusals return -22 and write nothing. */
typedef struct ppm_ctf_cfg { double pixel, kv, cs, wgh, min_res, max_res, min_def, max_def, step, tol; } ppm_ctf_cfg;
typedef struct ppm_ctf_fit_info {
    int tile, B, k2lo, k2hi, bg_w, nj, nc;       /* B_fit; samples have k2lo <= |k|^2 <= k2hi; background half width; D steps; candidates per d */
    double a;                                    /* a_fit */
    long ni, candidates, samples;                /* d steps of cfg's range, ni * nc, samples fitted */
} ppm_ctf_fit_info;
int ppm_ctf_fit_plan(int tile, const ppm_ctf_cfg *cfg, ppm_ctf_fit_info *out);
int ppm_ctf_fit(ppm_ctf_t *h, const void *spectra, int on_device, int n, int tile, const ppm_ctf_cfg *cfg, const double *def_lo,
                const double *def_hi, double *out_rows, float *grid_scores, long grid_ld, double *avrot, float *diag);
int ppm_ctf_estimate(ppm_ctf_t *h, const void *img, int on_device, int nx, int ny, int nframes, int group, int tile,
                     const ppm_ctf_cfg *cfg, double *out_row, double *avrot, float *diag);

/* Particle extraction straight into a (resident) stack — the step before the path:
 * crop `box` x `box` windows around the picked coordinates, fill what falls outside the micrograph with the mean
 * of the inside part, replace empty boxes by white noise, subtract the background mean and divide by the background
 * sigma (pixels farther than radius_px from the box centre).  Restates extract_particles_non_mpi
 * (src/pyp/extract/core.py:447-506) and normalize_image / extract_background / fix_empty_particles_in_place
 * (src/pyp/analysis/image.py:320-340, :406-417, :461-471).
 * image: rows x cols floats (row-major); coords: m x 2 doubles {box[0] (column coordinate), box[1] (row coordinate)}
 * in unbinned pixels; out: m * box * box floats.  Refused with -22 before anything is enqueued: a coordinate that is not finite
 * or whose floor(coordinate / coordinate_binning) leaves no room for the box in an int (the message names its index), and a
 * radius_px that is negative or not a number.  The rules are written out in DESIGN.md section 8a. */
int ppm_extract_boxes(const void *image, int image_on_device, int rows, int cols, const double *coords, int m,
                      int box, double coordinate_binning, double radius_px, int normalize, int fix_empty,
                      void *out, int out_on_device);

/* device-time accounting with HIP events on the library's stream */
void ppm_profile_enable(int on);
void ppm_profile_reset(void);
int ppm_profile_get(int kernel_id, double *total_ms, long *launches);

/* device memory helpers for callers that keep the particle stack resident in HBM */
void *ppm_device_alloc(size_t bytes);
void ppm_device_free(void *p);
int ppm_device_upload(void *dst, const void *src, size_t bytes);
int ppm_device_sync(void);
/* page-locked host staging memory: uploads from it overlap the kernels of the previous chunk (pageable memory makes them
 * synchronous); the drop-in executables read their particle ranges from the stack file through two such buffers */
void *ppm_host_alloc(size_t bytes);
void ppm_host_free(void *p);
/* Fill `dst` with `bytes` bytes of the open file `fd` from `offset`, read by `n_threads` (1..16) concurrent pread loops of a
 * thread pool the library keeps (no device call; returns when all parts are in).  The particle stack of a refine3d /
 * reconstruct3d range (src/pyp/refine/frealign/frealign.py:3918-3994, answer 1 "input particle images") comes out of the page
 * cache at ~60 GB/s this way, against ~8 GB/s for one thread.  Returns 0, -5 on a short read, -errno on a read error. */
int ppm_host_read(int fd, long long offset, void *dst, size_t bytes, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* PPM_H */
