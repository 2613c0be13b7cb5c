"""ctypes mirror of the structs in include/ppm.h (field order and types must match exactly)."""
import ctypes as C

NCOL = 32
STATS_COLS = 7
K_NAMES = ("prep", "bank", "global", "topk", "local", "insert", "final", "extract", "norms")


class RefineCfg(C.Structure):
    _fields_ = [
        ("box", C.c_int), ("pixel_size", C.c_float), ("molecular_mass_kda", C.c_float),
        ("mask_radius", C.c_float), ("res_low", C.c_float), ("res_high", C.c_float),
        ("res_signed_cc", C.c_float), ("search_mask_radius", C.c_float), ("res_search", C.c_float),
        ("angular_step", C.c_float), ("top_hits", C.c_int), ("search_range_x", C.c_float),
        ("search_range_y", C.c_float), ("global_search", C.c_int), ("local_refine", C.c_int),
        ("refine_psi", C.c_int), ("refine_theta", C.c_int), ("refine_phi", C.c_int),
        ("refine_x", C.c_int), ("refine_y", C.c_int), ("normalize", C.c_int), ("invert", C.c_int),
        ("mask_falloff", C.c_float), ("iters_hit", C.c_int), ("iters_final", C.c_int),
        ("local_angle_step", C.c_float), ("local_shift_step", C.c_float), ("symmetry", C.c_char * 8), ("band_factor", C.c_float),
        ("refine_defocus", C.c_int), ("defocus_range", C.c_float), ("defocus_step", C.c_float),
        ("focus", C.c_float * 4),
        ("use_priors", C.c_int), ("prior_mean", C.c_float * 5), ("prior_var", C.c_float * 5),
        ("res_classification", C.c_float),
    ]

    @classmethod
    def make(cls, **kw):
        focus = kw.pop("focus", None)
        priors = kw.pop("priors", None)          # (mean[5], var[5]) of psi, theta, phi (degrees), x, y (Angstrom)
        d = dict(molecular_mass_kda=0.0, res_low=0.0, res_signed_cc=0.0, search_mask_radius=0.0, res_search=0.0,
                 angular_step=15.0, top_hits=20, search_range_x=0.0, search_range_y=0.0, global_search=1,
                 local_refine=1, refine_psi=1, refine_theta=1, refine_phi=1, refine_x=1, refine_y=1, normalize=1,
                 invert=0, mask_falloff=0.0, iters_hit=0, iters_final=0, local_angle_step=0.0, local_shift_step=0.0,
                 band_factor=0.0, symmetry=b"C1", refine_defocus=0, defocus_range=500.0, defocus_step=50.0, res_classification=0.0)
        d.update(kw)
        for req in ("box", "pixel_size", "mask_radius", "res_high"):
            if req not in d:
                raise ValueError(f"ERROR: RefineCfg needs {req}")
        if not d["res_search"]:
            d["res_search"] = d["res_high"]
        if isinstance(d["symmetry"], str):
            d["symmetry"] = d["symmetry"].encode()
        c = cls(**d)
        if focus is not None:
            c.focus[:] = [float(v) for v in focus]
        if priors is not None:
            c.use_priors = 1
            c.prior_mean[:] = [float(v) for v in priors[0]]
            c.prior_var[:] = [float(v) for v in priors[1]]
        return c


class ReconCfg(C.Structure):
    _fields_ = [
        ("box", C.c_int), ("pixel_size", C.c_float), ("res_limit", C.c_float),
        ("score_weight_bfactor", C.c_float), ("score_average", C.c_float), ("score_threshold", C.c_float),
        ("normalize", C.c_int), ("invert", C.c_int), ("split_by_pind", C.c_int), ("mask_radius", C.c_float),
        ("dose_weights", C.c_void_p), ("n_dose_weights", C.c_int), ("dose_exponent", C.c_float), ("dose_transition", C.c_float),
    ]

    def set_dose_weights(self, q, exponent, transition=1.0):
        """q[t] in (0, 1] per exposure (TIND); the array is kept alive on the struct."""
        import numpy as np
        self._dose = np.ascontiguousarray(q, dtype=np.float32)
        self.dose_weights = self._dose.ctypes.data_as(C.c_void_p)
        self.n_dose_weights = int(self._dose.size)
        self.dose_exponent = float(exponent)
        self.dose_transition = float(transition)
        return self


NPCOL, NTCOL = 12, 6
CSP_PARTICLES, CSP_MICROGRAPHS = 1, 2


class CspCfg(C.Structure):
    """ppm_csp_cfg (include/ppm.h)."""
    _fields_ = [("unit", C.c_int), ("refine_rotation", C.c_int), ("refine_translation", C.c_int), ("tol_angle", C.c_float * 3),
                ("tol_shift", C.c_float), ("step_tolerance", C.c_float), ("max_iterations", C.c_int), ("tind_min", C.c_int),
                ("tind_max", C.c_int), ("first", C.c_int), ("last", C.c_int), ("refine_defocus", C.c_int),
                ("defocus_range", C.c_float), ("defocus_step", C.c_float), ("search_points", C.c_int), ("search_candidates", C.c_int)]

    @classmethod
    def make(cls, unit, refine_rotation=1, refine_translation=1, tol_angle=(30.0, 30.0, 30.0), tol_shift=20.0, step_tolerance=0.01,
             max_iterations=0, tind_min=0, tind_max=-1, first=0, last=-1, refine_defocus=0, defocus_range=750.0, defocus_step=50.0,
             search_points=0, search_candidates=0):
        """search_points: budget of the exhaustive particle search (csp_NumberOfRandomIterations; 0 = none), search_candidates: rotations
        per particle that go on to the compass passes (0 = 8)."""
        return cls(unit=int(unit), refine_rotation=int(refine_rotation), refine_translation=int(refine_translation),
                   tol_angle=(C.c_float * 3)(*[float(x) for x in tol_angle]), tol_shift=float(tol_shift),
                   step_tolerance=float(step_tolerance), max_iterations=int(max_iterations), tind_min=int(tind_min),
                   tind_max=int(tind_max), first=int(first), last=int(last), refine_defocus=int(refine_defocus),
                   defocus_range=float(defocus_range), defocus_step=float(defocus_step), search_points=int(search_points),
                   search_candidates=int(search_candidates))


class CspSearchInfo(C.Structure):
    """ppm_csp_search_info (include/ppm.h)."""
    _fields_ = [("active", C.c_int), ("shift_grid", C.c_int), ("step", C.c_double), ("r_g", C.c_double), ("h_s", C.c_double),
                ("tol_shift", C.c_double), ("n_angle", C.c_int * 3), ("full_turn", C.c_int * 3), ("n_shift_axis", C.c_int),
                ("n_rot", C.c_long), ("n_shift", C.c_long), ("n_candidates", C.c_int)]


FRAME_MAX_STEPS = 8


class FrameCfg(C.Structure):
    """ppm_frame_cfg (include/ppm.h)."""
    _fields_ = [("range_px", C.c_float), ("step_px", C.c_float), ("half_width", C.c_int), ("tind_min", C.c_int), ("tind_max", C.c_int),
                ("first", C.c_int), ("last", C.c_int)]

    @classmethod
    def make(cls, range_px, step_px=0.0, half_width=2, tind_min=0, tind_max=-1, first=0, last=-1):
        """range_px: shifts searched either side of a row's own, pixels; step_px: grid step (0 = half a pixel); half_width: frames pooled
        either side (csp_running_average_frames); tind_min / tind_max: tilts whose shifts are written back, the others are scored only
        (csp_UseImagesForRefinementMin / Max; max < 0 = no limit); first / last: tilts the call works on (last < 0 = to the end)."""
        return cls(range_px=float(range_px), step_px=float(step_px), half_width=int(half_width), tind_min=int(tind_min), tind_max=int(tind_max),
                   first=int(first), last=int(last))


class FrameInfo(C.Structure):
    """ppm_frame_info (include/ppm.h): groups with a usable row, slices gathered, rows whose shifts moved, rows scored only, rows returned
    unchanged, grid steps either side, grid step and reach in pixels, whether the range was cut."""
    _fields_ = [("groups", C.c_long), ("models", C.c_long), ("rows_refined", C.c_long), ("rows_scored", C.c_long), ("rows_skipped", C.c_long),
                ("n_steps", C.c_int), ("step_px", C.c_float), ("range_px", C.c_float), ("clipped", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SvaCfg(C.Structure):
    """ppm_sva_cfg (include/ppm.h)."""
    _fields_ = [("box", C.c_int), ("pixel_size", C.c_float), ("window", C.c_float * 3), ("window_sigma", C.c_float),
                ("highpass_cutoff", C.c_float), ("highpass_decay", C.c_float), ("lowpass_cutoff", C.c_float), ("lowpass_decay", C.c_float),
                ("use_missing_wedge", C.c_int), ("tol_angle", C.c_float), ("tol_shift", C.c_float), ("step_tolerance", C.c_float),
                ("max_iterations", C.c_int), ("band_factor", C.c_float), ("search_mode", C.c_int), ("global_step", C.c_float), ("n_candidates", C.c_int),
                ("symmetry", C.c_char * 8)]

    @classmethod
    def make(cls, box, pixel_size=1.0, window=(0, 0, 0), window_sigma=0.0, highpass=(0.0, 0.0), lowpass=(0.25, 0.05), use_missing_wedge=1,
             tol_angle=10.0, tol_shift=5.0, step_tolerance=0.05, max_iterations=0, band_factor=0.0, search_mode=0, global_step=0.0, n_candidates=0,
             symmetry=""):
        """symmetry: point group of the reference for the global search ("" = C1; the symbols of RefineCfg.symmetry)."""
        sym = symmetry.encode() if isinstance(symmetry, str) else bytes(symmetry)
        if len(sym) > 7:
            raise ValueError("ERROR: SvaCfg: symmetry symbol longer than 7 characters")
        return cls(box=int(box), pixel_size=float(pixel_size), window=(C.c_float * 3)(*[float(x) for x in window]), window_sigma=float(window_sigma),
                   highpass_cutoff=float(highpass[0]), highpass_decay=float(highpass[1]), lowpass_cutoff=float(lowpass[0]),
                   lowpass_decay=float(lowpass[1]), use_missing_wedge=int(use_missing_wedge), tol_angle=float(tol_angle),
                   tol_shift=float(tol_shift), step_tolerance=float(step_tolerance), max_iterations=int(max_iterations), band_factor=float(band_factor),
                   search_mode=int(search_mode), global_step=float(global_step), n_candidates=int(n_candidates), symmetry=sym)


class FinalCfg(C.Structure):
    _fields_ = [("molecular_mass_kda", C.c_float), ("inner_radius", C.c_float), ("outer_radius", C.c_float),
                ("mask_falloff", C.c_float)]


class MaskCfg(C.Structure):
    """ppm_mask_cfg (include/ppm.h)."""
    _fields_ = [("pixel_size", C.c_double), ("edge_width", C.c_int), ("outside_weight", C.c_double), ("filter", C.c_int),
                ("filter_radius_A", C.c_double), ("filter_edge_px", C.c_double)]

    @classmethod
    def make(cls, pixel_size, edge_width=3, outside_weight=0.0, filter=0, filter_radius_A=10.0, filter_edge_px=10.0):
        """edge_width: cosine edge added to the mask (voxels, 0 = none); outside_weight: weight of the density outside the mask;
        filter: low-pass of that density (0 = none, 2 = cosine edge at filter_radius_A Angstrom, filter_edge_px Fourier pixels wide)."""
        return cls(pixel_size=float(pixel_size), edge_width=int(edge_width), outside_weight=float(outside_weight), filter=int(filter),
                   filter_radius_A=float(filter_radius_A), filter_edge_px=float(filter_edge_px))


class CreateMaskCfg(C.Structure):
    """ppm_create_mask_cfg (include/ppm.h)."""
    _fields_ = [("pixel_size", C.c_double), ("outer_radius_A", C.c_double), ("threshold", C.c_double), ("lowpass_A", C.c_double),
                ("lowpass_edge_px", C.c_double), ("rebin", C.c_double)]

    @classmethod
    def make(cls, pixel_size, outer_radius_A, threshold, lowpass_A=0.0, lowpass_edge_px=4.0, rebin=0.35):
        """outer_radius_A: sphere outside of which nothing is kept; threshold: density at or above which a voxel counts; lowpass_A: the
        map is low-passed to this resolution first and the largest body once more afterwards (0 = neither); lowpass_edge_px: width of
        the filter's cosine edge in Fourier pixels; rebin: level at which the low-passed body becomes the mask (strictly inside 0..1)."""
        return cls(pixel_size=float(pixel_size), outer_radius_A=float(outer_radius_A), threshold=float(threshold), lowpass_A=float(lowpass_A),
                   lowpass_edge_px=float(lowpass_edge_px), rebin=float(rebin))


class CreateMaskInfo(C.Structure):
    """ppm_create_mask_info (include/ppm.h): range of the (low-passed) density inside the sphere, voxels at or above the threshold there,
    their connected bodies, voxels of the largest, voxels of the mask."""
    _fields_ = [("density_min", C.c_double), ("density_max", C.c_double), ("above", C.c_long), ("components", C.c_long),
                ("largest", C.c_long), ("mask_voxels", C.c_long)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FitInfo(C.Structure):
    """ppm_fit_info (include/ppm.h): the plan that fits a reference of n_in voxels to box_out - what the output box can show (n_c), the
    padded / cropped input P, its resampled size M, scale = pixel_in / pixel_out, the pixel size the pair achieves and how far M / (P scale)
    is from 1 - and the pad values of the two resizes (ppm_fit_volume only)."""
    _fields_ = [("n_in", C.c_int), ("box_out", C.c_int), ("n_c", C.c_int), ("P", C.c_int), ("M", C.c_int), ("scale", C.c_double),
                ("pixel_achieved", C.c_double), ("rel_error", C.c_double), ("pad_value_1", C.c_double), ("pad_value_2", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CtfSpectrumInfo(C.Structure):
    """ppm_ctf_spectrum_info (include/ppm.h): the plan of an averaged periodogram - tile T and T / 2 + 1, tiles along x and y, frame
    groups, whether the sizes allow 16-byte loads, tiles averaged, partial sums, tiles per trip, the two workspaces in bytes and the
    floats of the result."""
    _fields_ = [("tile", C.c_int), ("half_w", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("groups", C.c_int), ("vec", C.c_int),
                ("tiles", C.c_long), ("chunks", C.c_long), ("pass_tiles", C.c_long), ("half_bytes", C.c_long), ("part_bytes", C.c_long),
                ("out_floats", C.c_long)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CtfCfg(C.Structure):
    """ppm_ctf_cfg (include/ppm.h): pixel size in A, voltage in kV, spherical aberration in mm, amplitude contrast, the resolutions between
    which the spectrum is fitted, the range and step of the mean-defocus grid in A, the astigmatism restraint in A (0: none)."""
    _fields_ = [("pixel", C.c_double), ("kv", C.c_double), ("cs", C.c_double), ("wgh", C.c_double), ("min_res", C.c_double),
                ("max_res", C.c_double), ("min_def", C.c_double), ("max_def", C.c_double), ("step", C.c_double), ("tol", C.c_double)]

    @classmethod
    def make(cls, pixel, kv=300.0, cs=2.7, wgh=0.07, min_res=30.0, max_res=5.0, min_def=5000.0, max_def=50000.0, step=500.0, tol=0.0):
        return cls(float(pixel), float(kv), float(cs), float(wgh), float(min_res), float(max_res), float(min_def), float(max_def),
                   float(step), float(tol))


class CtfFitInfo(C.Structure):
    """ppm_ctf_fit_info (include/ppm.h): the plan of a fit - B_fit, the |k|^2 range of the fitted samples, the background's half width,
    astigmatism steps, candidates per mean defocus, a_fit, mean-defocus steps, candidates and samples."""
    _fields_ = [("tile", C.c_int), ("B", C.c_int), ("k2lo", C.c_int), ("k2hi", C.c_int), ("bg_w", C.c_int), ("nj", C.c_int), ("nc", C.c_int),
                ("a", C.c_double), ("ni", C.c_long), ("candidates", C.c_long), ("samples", C.c_long)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PostCfg(C.Structure):
    """ppm_post_cfg (include/ppm.h)."""
    MASK = {"none": 0, "external": 1, "auto": 2}
    THRESHOLD = {"intensity": 0, "sigma": 1, "volume": 2}
    RANDOMIZE = {"resolution": 0, "fsc": 1}
    BFACTOR = {"none": 0, "adhoc": 1, "auto": 2}
    _fields_ = [("pixel_size", C.c_double), ("mask_mode", C.c_int), ("automask_lp", C.c_double), ("threshold_method", C.c_int),
                ("threshold_value", C.c_double), ("randomize_method", C.c_int), ("randomize_value", C.c_double), ("seed", C.c_uint),
                ("bfactor_method", C.c_int), ("adhoc_bfac", C.c_double), ("fit_low", C.c_double), ("fit_high", C.c_double),
                ("lowpass_auto", C.c_int), ("lowpass", C.c_double), ("highpass", C.c_double), ("gaussian", C.c_int),
                ("skip_fsc_weighting", C.c_int), ("apply_fsc2", C.c_int), ("flip_x", C.c_int), ("flip_y", C.c_int), ("flip_z", C.c_int)]

    @classmethod
    def make(cls, pixel_size, mask="none", automask_lp=0.0, threshold_method="intensity", threshold_value=0.0, randomize="fsc",
             randomize_value=0.8, seed=0, bfactor="none", adhoc_bfac=0.0, fit_low=10.0, fit_high=0.0, lowpass="auto", highpass=0.0,
             gaussian=False, skip_fsc_weighting=False, apply_fsc2=False, flip_x=False, flip_y=False, flip_z=False):
        """mask: "none", "external" (host.postprocess is given one) or "auto" (made from the mean of the halves: low-pass automask_lp in A,
        threshold_method "intensity" / "sigma" / "volume" with threshold_value); randomize: "fsc" (from the first shell whose unmasked FSC
        is below randomize_value) or "resolution" (from randomize_value A); bfactor: "none", "adhoc" (adhoc_bfac, negative sharpens) or
        "auto" (fit between fit_low and fit_high A, fit_high 0 = the resolution); lowpass: A, 0 = none, "auto" = the resolution;
        highpass: A, <= 0 = none."""
        auto = isinstance(lowpass, str)
        if auto and lowpass != "auto":
            raise ValueError(f"ERROR: PostCfg: lowpass must be a number or 'auto', got '{lowpass}'")
        return cls(pixel_size=float(pixel_size), mask_mode=cls.MASK[mask], automask_lp=float(automask_lp),
                   threshold_method=cls.THRESHOLD[threshold_method], threshold_value=float(threshold_value),
                   randomize_method=cls.RANDOMIZE[randomize], randomize_value=float(randomize_value), seed=int(seed) & 0xFFFFFFFF,
                   bfactor_method=cls.BFACTOR[bfactor], adhoc_bfac=float(adhoc_bfac), fit_low=float(fit_low), fit_high=float(fit_high),
                   lowpass_auto=1 if auto else 0, lowpass=0.0 if auto else float(lowpass), highpass=float(highpass), gaussian=int(bool(gaussian)),
                   skip_fsc_weighting=int(bool(skip_fsc_weighting)), apply_fsc2=int(bool(apply_fsc2)), flip_x=int(bool(flip_x)),
                   flip_y=int(bool(flip_y)), flip_z=int(bool(flip_z)))


class PostInfo(C.Structure):
    """ppm_post_info (include/ppm.h): first randomised shell, first shell with a corrected FSC below 0.143 (0: none), shells of the
    B-factor fit, complex transforms run, resolution in A, B in A^2, threshold of the automatic mask, voxels of the mask."""
    _fields_ = [("s_r", C.c_int), ("res_shell", C.c_int), ("fit_shells", C.c_int), ("transforms", C.c_int), ("resolution", C.c_double),
                ("bfactor", C.c_double), ("threshold", C.c_double), ("mask_voxels", C.c_long)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


LOCRES_MAX_LEVELS = 64
LOCRES_UNASSIGNED = 100.0
LOCRES_MIN_STEP = 0.25
LOCRES_MIN_LEVEL_PX = 2.5


def locres_levels(n, pixel_size, min_res=0.0, max_res=0.0, step=1.0):
    """The level grid of ppm_local_resolution as the library builds it, in float64: lambda_min + i step for all i with
    lambda_i <= lambda_max.  min_res below 2.5 pixels (0 included) is raised to that; max_res 0 = n pixel_size / 6.  Returns
    (levels, notes); raises ValueError for what the library refuses (step < 0.25, max_res above n pixel_size / 4, no level, more than 64)."""
    a, lo, hi, step = float(pixel_size), float(min_res), float(max_res), float(step)
    if not a > 0:
        raise ValueError("ERROR: local_resolution: the pixel size must be positive")
    if not step >= LOCRES_MIN_STEP or step == float("inf"):
        raise ValueError("ERROR: local_resolution: the resolution step must be at least 0.25 A")
    if not (0 <= lo < float("inf")) or not (0 <= hi < float("inf")):
        raise ValueError("ERROR: local_resolution: the minimum and maximum resolution must not be negative (0 = the default)")
    notes = []
    if lo < LOCRES_MIN_LEVEL_PX * a:
        notes.append("minimum resolution %g A raised to %g A (2.5 pixels)" % (lo, LOCRES_MIN_LEVEL_PX * a))
        lo = LOCRES_MIN_LEVEL_PX * a
    if hi == 0:
        hi = n * a / 6.0
        notes.append("maximum resolution set to %g A (box / 6)" % hi)
    elif hi > n * a / 4.0:
        raise ValueError("ERROR: local_resolution: the maximum resolution %g A is above a quarter of the box (%g A)" % (hi, n * a / 4.0))
    levels = []
    i = 0
    while lo + i * step <= hi:
        if i >= LOCRES_MAX_LEVELS:
            raise ValueError("ERROR: local_resolution: more than 64 resolution levels; raise the step or narrow the range")
        levels.append(lo + i * step)
        i += 1
    if not levels:
        raise ValueError("ERROR: local_resolution: no resolution level between %g A and %g A" % (lo, hi))
    return levels, notes


def locres_rank(p_value, n_inside):
    """r of ppm_local_resolution: the threshold of a level is the r-th smallest noise energy over the n_inside voxels of the mask,
    r = ceil((1 - p) n_inside) clipped to 1 .. n_inside."""
    import math
    return int(min(max(math.ceil((1.0 - float(p_value)) * float(n_inside)), 1), n_inside))


class LocresCfg(C.Structure):
    """ppm_locres_cfg (include/ppm.h)."""
    _fields_ = [("pixel_size", C.c_double), ("p_value", C.c_double), ("min_res", C.c_double), ("max_res", C.c_double), ("step", C.c_double),
                ("keep_levels", C.c_int)]

    @classmethod
    def make(cls, pixel_size, p_value=0.05, min_res=0.0, max_res=0.0, step=1.0, keep_levels=False):
        """p_value: of the test of a level's signal energy against the noise energies inside the mask; min_res, max_res, step: the level
        grid in A (abi.locres_levels; 0 = 2.5 pixels / a sixth of the box); keep_levels: a debug output - host.local_resolution also
        returns the energy maps (E_A, E_D) of every level."""
        if not 0 < float(p_value) < 1:
            raise ValueError(f"ERROR: LocresCfg: the p-value must lie strictly between 0 and 1, got {p_value}")
        return cls(pixel_size=float(pixel_size), p_value=float(p_value), min_res=float(min_res), max_res=float(max_res), step=float(step),
                   keep_levels=1 if keep_levels else 0)


class LocresInfo(C.Structure):
    """ppm_locres_info (include/ppm.h): levels (ascending), tau and voxels per level, inside voxels, those left at 100, the median of the
    map over the inside voxels, complex transforms run, notes."""
    _fields_ = [("n_levels", C.c_int), ("transforms", C.c_int), ("n_inside", C.c_long), ("unassigned", C.c_long), ("median", C.c_double),
                ("levels", C.c_float * LOCRES_MAX_LEVELS), ("tau", C.c_float * LOCRES_MAX_LEVELS), ("counts", C.c_long * LOCRES_MAX_LEVELS),
                ("notes", C.c_char * 256)]

    def as_dict(self):
        L = self.n_levels
        return dict(n_levels=L, transforms=self.transforms, n_inside=self.n_inside, unassigned=self.unassigned, median=self.median,
                    levels=list(self.levels[:L]), tau=list(self.tau[:L]), counts=list(self.counts[:L]), notes=self.notes.decode())
