"""Positional stdin answer scripts of the drop-in executables.

The caller never parses prompts; it pipes a here-doc of answers, one per line, `yes`/`no` for
booleans (src/pyp/refine/frealign/frealign.py:3918-3994 refine3d, :1780-1824 reconstruct3d,
:1878-1888 local_merge3d, :2075-2093 merge3d; src/pyp/align/core.py:811-850 apply_mask.exe; src/pyp/inout/image/core.py:1583-1596
create_mask; the `.par`-surface refine3d script
is preserved at src/pyp/system/wrapper_functions.py:512-561).  Answer order: SURVEY.md §9.1-§9.3.
cistem2's resample / resize and frealign_v9.11's resample_mp.exe: src/pyp/system/wrapper_functions.py:57-67, :109-118 and
src/pyp/analysis/image.py:97-118, :226-241 (parse_resample, parse_resize, parse_resample_mp).
postprocessing.py and ResMap take command lines (src/pyp_main.py:6638-6737, :6826): parse_postprocessing, parse_resmap.
"""


class PromptError(ValueError):
    pass


def read_answers(stream):
    """All lines of the here-doc, stripped; stops at a line reading 'eot' if the shell left it in."""
    out = []
    for line in stream.read().splitlines():
        s = line.strip()
        if s == "eot":
            break
        out.append(s)
    while out and out[-1] == "":
        out.pop()
    return out


def split_heredoc(command):
    """A command string exactly as PYP builds it — '<dir>/<program> << eot >> <logfile> 2>&1\n<answer>\n...eot\n'
    (frealign.py:3918-3994, :1780-1824, :1878-1888, :2075-2093) — taken apart into (program, logfile, answers)."""
    head, _, rest = command.lstrip("\n").partition("\n")
    prog, sep, tail = head.partition("<<")
    if not sep:
        raise PromptError(f"ERROR: not a here-doc command: '{head}'")
    log = tail.split(">>", 1)[1].replace("2>&1", "").strip() if ">>" in tail else ""
    import io
    return prog.strip(), log, read_answers(io.StringIO(rest))


def _bool(s, what):
    t = s.strip().lower()
    if t in ("yes", "y", "true", "1"):
        return True
    if t in ("no", "n", "false", "0"):
        return False
    raise PromptError(f"ERROR: answer for '{what}' must be yes or no, got '{s}'")


def _num(s, what, typ=float):
    try:
        return typ(float(s)) if typ is int else typ(s)
    except ValueError:
        raise PromptError(f"ERROR: answer for '{what}' must be a number, got '{s}'")


REFINE3D_CISTEM = [  # (key, kind) in script order, 50 answers
    ("stack", str), ("input_params", str), ("global_stats", str), ("reference", str), ("statistics", str),
    ("use_statistics", bool), ("use_priors", bool), ("match_out", str), ("output_params", str), ("output_changes", str),
    ("symmetry", str), ("first", int), ("last", int), ("fraction", float), ("pixel_size", float), ("molecular_mass", float),
    ("inner_radius", float), ("outer_radius", float), ("res_low", float), ("res_high", float), ("res_signed_cc", float),
    ("res_classification", float), ("search_mask_radius", float), ("res_search", float), ("angular_step", float),
    ("top_hits", int), ("search_range_x", float), ("search_range_y", float), ("focus_x", float), ("focus_y", float),
    ("focus_z", float), ("focus_r", float), ("defocus_range", float), ("defocus_step", float), ("padding", float),
    ("global_search", bool), ("local_refine", bool), ("refine_psi", bool), ("refine_theta", bool), ("refine_phi", bool),
    ("refine_x", bool), ("refine_y", bool), ("calc_match", bool), ("mask_2d", bool), ("refine_defocus", bool),
    ("normalize", bool), ("invert", bool), ("exclude_edges", bool), ("normalize_reference", bool), ("threshold_reference", bool),
]

REFINE3D_PAR = [  # frealign_v9.11 surface, 45 answers
    ("stack", str), ("input_params", str), ("reference", str), ("statistics", str), ("use_statistics", bool),
    ("match_out", str), ("output_params", str), ("output_changes", str), ("symmetry", str), ("first", int), ("last", int),
    ("pixel_size", float), ("voltage", float), ("cs", float), ("amplitude_contrast", float), ("molecular_mass", float),
    ("outer_radius", float), ("res_low", float), ("res_high", float), ("res_signed_cc", float), ("res_classification", float),
    ("search_mask_radius", float), ("res_search", float), ("angular_step", float), ("top_hits", int),
    ("search_range_x", float), ("search_range_y", float), ("focus_x", float), ("focus_y", float), ("focus_z", float),
    ("focus_r", float), ("defocus_range", float), ("defocus_step", float), ("padding", float), ("global_search", bool),
    ("local_refine", bool), ("refine_psi", bool), ("refine_theta", bool), ("refine_phi", bool), ("refine_x", bool),
    ("refine_y", bool), ("calc_match", bool), ("mask_2d", bool), ("refine_defocus", bool), ("invert", bool),
]

MERGE3D = [("half1", str), ("half2", str), ("filtered", str), ("statistics", str), ("molecular_mass", float),
           ("inner_radius", float), ("outer_radius", float), ("dump_seed_1", str), ("dump_seed_2", str), ("n_dumps", int)]

LOCAL_MERGE3D = [("out_dump_1", str), ("out_dump_2", str), ("dump_seed_1", str), ("dump_seed_2", str), ("n_dumps", int)]


def _take(answers, spec, prog):
    if len(answers) < len(spec):
        raise PromptError(f"ERROR: {prog}: expected {len(spec)} answers, got {len(answers)}")
    out = {}
    for (key, kind), s in zip(spec, answers):
        if kind is bool:
            out[key] = _bool(s, key)
        elif kind is str:
            if s == "":
                raise PromptError(f"ERROR: {prog}: empty answer for '{key}'")
            out[key] = s
        else:
            out[key] = _num(s, key, kind)
    return out


def parse_refine3d(answers):
    """Selects the .par surface when the input parameter file is not a .cistem file."""
    if len(answers) >= 2 and not answers[1].endswith(".cistem"):
        d = _take(answers, REFINE3D_PAR, "refine3d")
        d["surface"] = "par"
        d.update(global_stats="null", use_priors=False, fraction=1.0, inner_radius=0.0, normalize=True,
                 exclude_edges=False, normalize_reference=False, threshold_reference=False)
    else:
        d = _take(answers, REFINE3D_CISTEM, "refine3d")
        d["surface"] = "cistem"
    if d["first"] < 1 or d["last"] < d["first"]:
        raise PromptError(f"ERROR: refine3d: bad particle range {d['first']}..{d['last']}")
    return d


def parse_reconstruct3d(answers):
    """39 answers, or 43 when dose weighting is switched on (its answer expands to five lines,
    frealign.py:1731-1753)."""
    a = list(answers)
    head = [("stack", str), ("input_params", str), ("global_stats", str), ("reference", str), ("map1", str), ("map2", str),
            ("output", str), ("res_file", str), ("symmetry", str), ("first", int), ("last", int), ("pixel_size", float),
            ("molecular_mass", float), ("inner_radius", float), ("outer_radius", float), ("res_limit", float),
            ("res_reference", float), ("score_bfactor", float), ("score_weighting", bool), ("min_tilt_score", float),
            ("max_tilt_score", float), ("dose_weighting", bool)]
    tail = [("score_threshold", float), ("smoothing", float), ("padding", float), ("normalize", bool), ("adjust_scores", bool),
            ("invert", bool), ("exclude_edges", bool), ("crop", bool), ("split_even_odd", bool), ("per_particle_splitting", bool),
            ("center_mass", bool), ("likelihood_blurring", bool), ("threshold_reference", bool), ("dump", bool),
            ("dump_1", str), ("dump_2", str), ("threads", int)]
    d = _take(a, head, "reconstruct3d")
    rest = a[len(head):]
    if d["dose_weighting"]:
        dw = _take(rest, [("dose_weights_file", str), ("dose_multiply", bool), ("dose_fraction", float), ("dose_transition", float)],
                   "reconstruct3d")
        d.update(dw)
        rest = rest[4:]
    d.update(_take(rest, tail, "reconstruct3d"))
    if d["first"] < 1 or d["last"] < d["first"]:
        raise PromptError(f"ERROR: reconstruct3d: bad particle range {d['first']}..{d['last']}")
    return d


def parse_merge3d(answers):
    return _take(answers, MERGE3D, "merge3d")


def parse_local_merge3d(answers):
    return _take(answers, LOCAL_MERGE3D, "local_merge3d")


def parse_apply_mask(answers):
    """apply_mask.exe (frealign_v9.11), answers in the order of the questions at src/pyp/align/core.py:788-799: image format, input
    map, pixel size, input mask, width of the cosine edge, weight outside, outside filter, [filter radius in A, filter edge in pixels,]
    output map.  Two layouts: 10 answers, or the 8 PYP sends with filter `0` / `0.0` (:833-850: no radius, no filter edge).  The
    filter answer is a number (`0` and `0.0` both mean none).  pixel_size None: `*`, the map header's value.  Refused here: what
    can be told from the answers alone (format other than M, the Gaussian filter 1, ranges ppm_mask_volume refuses, include/ppm.h)."""
    prog = "apply_mask"
    a = list(answers)
    if len(a) < 8:
        raise PromptError(f"ERROR: {prog}: expected 8 or 10 answers, got {len(a)}")
    d = _take(a, [("format", str), ("map", str), ("pixel", str), ("mask", str), ("edge_width", float), ("outside_weight", float),
                  ("filter", float)], prog)
    if d["format"].upper() != "M":
        raise PromptError(f"ERROR: {prog}: image format '{d['format']}' is not supported by this build (only M, MRC)")
    d["pixel_size"] = None if d.pop("pixel") == "*" else _num(a[2], "pixel_size")
    if d["pixel_size"] is not None and not d["pixel_size"] > 0:
        raise PromptError(f"ERROR: {prog}: pixel size must be positive or *, got '{a[2]}'")
    if d["edge_width"] != int(d["edge_width"]) or not 0 <= d["edge_width"] <= 64:
        raise PromptError(f"ERROR: {prog}: width of the cosine edge must be a whole number of pixels, 0..64, got '{a[4]}'")
    d["edge_width"] = int(d["edge_width"])
    if d["filter"] == 1:
        raise PromptError(f"ERROR: {prog}: the Gaussian low-pass filter outside (1) is not supported by this build (0 = none, 2 = cosine edge)")
    if d["filter"] not in (0, 2):
        raise PromptError(f"ERROR: {prog}: low-pass filter outside must be 0 or 2, got '{a[6]}'")
    d["filter"] = int(d["filter"])
    if d["filter"] == 0 and len(a) == 8:
        d.update(filter_radius=0.0, filter_edge=0.0)
        rest = a[7:]
    else:
        if len(a) < 10:
            raise PromptError(f"ERROR: {prog}: expected 10 answers (filter radius and filter edge before the output), got {len(a)}")
        d.update(_take(a[7:], [("filter_radius", float), ("filter_edge", float)], prog))
        rest = a[9:]
    if len(rest) != 1:
        raise PromptError(f"ERROR: {prog}: expected 8 or 10 answers, got {len(a)}")
    d.update(_take(rest, [("output", str)], prog))
    if d["filter"] == 2 and not d["filter_radius"] > 0:
        raise PromptError(f"ERROR: {prog}: cosine edge filter radius must be positive, got '{a[7]}'")
    if d["filter"] == 2 and not d["filter_edge"] >= 0:
        raise PromptError(f"ERROR: {prog}: width of the filter edge must not be negative, got '{a[8]}'")
    return d


CREATE_MASK = [("input", str), ("output", str), ("pixel_size", float), ("outer_radius", float), ("auto_threshold", bool),
               ("threshold", float), ("lowpass", float), ("rebin", float)]
# The script has no answer for the width of the low-pass edge: this many Fourier pixels, at most 2 r_c
CREATE_MASK_EDGE_PX = 4.0


def parse_create_mask(answers):
    """create_mask (frealignx), the eight answers in the order of the questions at src/pyp/inout/image/core.py:1548-1555 and of the
    script at :1583-1596: input map, output mask, pixel size, outer radius in A, auto-estimate the threshold (PYP always sends No),
    threshold, low-pass resolution in A (0 = none), re-bin value.  Refused here: what can be told from the answers alone (the
    automatic threshold, ranges ppm_create_mask refuses, include/ppm.h)."""
    prog = "create_mask"
    a = list(answers)
    if len(a) != len(CREATE_MASK):
        raise PromptError(f"ERROR: {prog}: expected {len(CREATE_MASK)} answers, got {len(a)}")
    d = _take(a, CREATE_MASK, prog)
    if d["auto_threshold"]:
        raise PromptError(f"ERROR: {prog}: the automatic estimate of the binarization threshold is not supported by this build (answer No and give a threshold)")
    if not d["pixel_size"] > 0:
        raise PromptError(f"ERROR: {prog}: pixel size must be positive, got '{a[2]}'")
    if not d["outer_radius"] > 0:
        raise PromptError(f"ERROR: {prog}: outer radius of the mask must be positive, got '{a[3]}'")
    if not d["threshold"] == d["threshold"] or d["threshold"] in (float("inf"), float("-inf")):
        raise PromptError(f"ERROR: {prog}: binarization threshold must be a finite number, got '{a[5]}'")
    if not d["lowpass"] >= 0:
        raise PromptError(f"ERROR: {prog}: low-pass filter resolution must not be negative (0 = none), got '{a[6]}'")
    if d["lowpass"] != 0 and not 0 < d["rebin"] < 1:
        raise PromptError(f"ERROR: {prog}: re-bin value must lie strictly between 0 and 1, got '{a[7]}'")
    return d


# ------------------------------------------------------------------------------------------ resample / resize / resample_mp.exe
def resample_len_ok(n):
    """Lengths the transforms take (box_ok of ppm_geom.h): even, 32..512, prime factors 2, 3, 5, 7 only."""
    if n < 32 or n > 512 or n % 2:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def resample_nearest_ok(n):
    """The supported lengths next to n, below and above (either may be missing)."""
    lo = next((k for k in range(min(n, 512), 31, -1) if resample_len_ok(k)), None)
    hi = next((k for k in range(max(n, 32), 513) if resample_len_ok(k)), None)
    return [k for k in dict.fromkeys((lo, hi)) if k is not None]


def _size_answers(prog, names, answers):
    """Size answers are numbers (resample_and_resize sends a float, preprocess/core.py:776-782); a fractional part is rounded to the nearest
    integer and the rounding is reported.  Returns (the one size all of them name, notes for the log)."""
    sizes, notes = [], []
    for name, s in zip(names, answers):
        v = _num(s, name)
        if not v == v or v in (float("inf"), float("-inf")):
            raise PromptError(f"ERROR: {prog}: answer for '{name}' must be a finite number, got '{s}'")
        r = int(round(v))
        if r != v:
            notes.append(f"{name}: {s} is not a whole number of pixels, rounded to {r}")
        sizes.append(r)
    if len(set(sizes)) != 1:
        raise PromptError(f"ERROR: {prog}: only equal sizes along every axis are supported by this build (square images, cubic volumes), got "
                          + " x ".join(str(v) for v in sizes))
    if sizes[0] < 1:
        raise PromptError(f"ERROR: {prog}: the new size must be positive, got {sizes[0]}")
    return sizes[0], notes


def _resample_like(prog, answers, real_space=False, normalize=False):
    a = list(answers)
    if a and a[-1].strip().upper() == "EOF":              # a here-doc closed by EOF, taken apart by split_heredoc (which knows `eot`)
        a.pop()
    head = [("input", str), ("output", str), ("volume", bool)] + ([("real_space_binning", bool)] if real_space else [])
    d = _take(a, head, prog)
    names = ["new_x", "new_y"] + (["new_z"] if d["volume"] else [])
    want = len(head) + len(names) + (1 if normalize else 0)
    if len(a) < want:
        raise PromptError(f"ERROR: {prog}: expected {want} answers ({'a volume' if d['volume'] else 'a stack of images'}), got {len(a)}")
    if len(a) > want and any(s != "" for s in a[want:]):
        raise PromptError(f"ERROR: {prog}: expected {want} answers ({'a volume' if d['volume'] else 'a stack of images'}), got {len(a)}")
    d["size"], d["notes"] = _size_answers(prog, names, a[len(head):len(head) + len(names)])
    if normalize:
        d["normalize"] = _bool(a[want - 1], "normalize")
    if real_space and d["real_space_binning"]:
        raise PromptError(f"ERROR: {prog}: real-space binning is not supported by this build (answer no: Fourier resampling)")
    return d


def parse_resample(answers):
    """cistem2's resample, the answers of src/pyp/system/wrapper_functions.py:109-118: input, output, is the input a volume, new X, new Y,
    and new Z only for a volume."""
    return _resample_like("resample", answers)


def parse_resize(answers):
    """cistem2's resize (wrapper_functions.py:57-67): the answers of resample plus 'normalize and zero-float the input'."""
    return _resample_like("resize", answers, normalize=True)


def parse_resample_mp(answers):
    """frealign_v9.11's resample_mp.exe (src/pyp/analysis/image.py:97-118, :226-241): input, output, volume, real-space binning (refused;
    PYP sends no), new X, new Y, and new Z only for a volume."""
    return _resample_like("resample_mp", answers, real_space=True)


POSTPROCESSING_FLAGS = ("flip_x", "flip_y", "flip_z", "gaussian", "skip_fsc_weighting", "apply_fsc2", "automask", "xml")
POSTPROCESSING_VALUES = ("mask", "angpix", "out", "auto_bfac", "adhoc_bfac", "lowpass", "highpass", "automask_input", "automask_lp",
                         "automask_threshold", "automask_fraction", "automask_sigma", "randomize_below_fsc", "randomize_beyond",
                         "refine_res_lim", "mtf")
POSTPROCESSING_RANDOMIZE_FSC = 0.8       # neither --randomize_below_fsc nor --randomize_beyond: from the first shell with an FSC below this


def postprocessing_box_ok(n):
    """A box the library's transforms take: even, 32..512, prime factors 2, 3, 5, 7."""
    if n % 2 or not 32 <= n <= 512:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def parse_postprocessing(argv):
    """postprocessing.py, the command line PYP's Post-processing block puts together at src/pyp_main.py:6638-6737 (it is a command line,
    not a here-doc): `half1 half2 [--mask F] --angpix A --out NAME [--flip_x] [--flip_y] [--flip_z] [--refine_res_lim V] --xml
    [--auto_bfac LOW,HIGH | --adhoc_bfac I] [--gaussian] --lowpass V|auto --highpass V [--skip_fsc_weighting] [--apply_fsc2]
    [--automask --automask_input 0 --automask_lp V (--automask_threshold V | --automask_fraction V | --automask_sigma V)]
    [--randomize_below_fsc V | --randomize_beyond V]`.  Options may also be written `--name=value`.  Refused here: what can be told from
    the command line alone (--mtf, --automask_input other than 0, both FSC flags, unknown options, values out of range)."""
    prog = "postprocessing"
    d = {k: False for k in POSTPROCESSING_FLAGS}
    d.update({k: None for k in POSTPROCESSING_VALUES})
    pos = []
    a = list(argv)
    i = 0
    while i < len(a):
        tok = a[i]
        i += 1
        if not tok.startswith("--"):
            pos.append(tok)
            continue
        name, eq, val = tok[2:].partition("=")
        if name in POSTPROCESSING_FLAGS:
            if eq:
                raise PromptError(f"ERROR: {prog}: option --{name} takes no value")
            d[name] = True
        elif name in POSTPROCESSING_VALUES:
            if not eq:
                if i >= len(a):
                    raise PromptError(f"ERROR: {prog}: option --{name} needs a value")
                val = a[i]
                i += 1
            if d[name] is not None:
                raise PromptError(f"ERROR: {prog}: option --{name} given twice")
            d[name] = val
        else:
            raise PromptError(f"ERROR: {prog}: unknown option '{tok}'")
    if len(pos) != 2:
        raise PromptError(f"ERROR: {prog}: expected the two half maps, got {len(pos)} positional arguments")
    d["half1"], d["half2"] = pos
    if d["mtf"] is not None:
        raise PromptError(f"ERROR: {prog}: the MTF correction (--mtf) is not supported by this build")
    if d["angpix"] is None or d["out"] is None:
        raise PromptError(f"ERROR: {prog}: --angpix and --out are required")
    d["angpix"] = _num(d["angpix"], "angpix")
    if not d["angpix"] > 0:
        raise PromptError(f"ERROR: {prog}: pixel size must be positive, got '{d['angpix']:g}'")
    if d["skip_fsc_weighting"] and d["apply_fsc2"]:
        raise PromptError(f"ERROR: {prog}: --skip_fsc_weighting and --apply_fsc2 exclude each other")
    # B-factor
    if d["auto_bfac"] is not None and d["adhoc_bfac"] is not None:
        raise PromptError(f"ERROR: {prog}: --auto_bfac and --adhoc_bfac exclude each other")
    d["bfactor"], d["fit_low"], d["fit_high"] = "none", 10.0, 0.0
    if d["adhoc_bfac"] is not None:
        d["bfactor"], d["adhoc_bfac"] = "adhoc", _num(d["adhoc_bfac"], "adhoc_bfac")
    elif d["auto_bfac"] is not None:
        parts = d["auto_bfac"].split(",")
        if len(parts) != 2:
            raise PromptError(f"ERROR: {prog}: --auto_bfac takes LOW,HIGH (resolutions in A), got '{d['auto_bfac']}'")
        d["bfactor"], d["fit_low"], d["fit_high"] = "auto", _num(parts[0], "auto_bfac low"), _num(parts[1], "auto_bfac high")
        if not d["fit_low"] > 0 or not d["fit_high"] >= 0 or d["fit_high"] > d["fit_low"]:
            raise PromptError(f"ERROR: {prog}: --auto_bfac needs LOW > 0 and 0 <= HIGH <= LOW (in A; HIGH 0 = the resolution), got '{d['auto_bfac']}'")
    d["adhoc_bfac"] = d["adhoc_bfac"] if d["bfactor"] == "adhoc" else 0.0
    # filter
    if d["lowpass"] is None or d["lowpass"] == "auto":
        d["lowpass"] = "auto"
    else:
        d["lowpass"] = _num(d["lowpass"], "lowpass")
        if not d["lowpass"] >= 0:
            raise PromptError(f"ERROR: {prog}: --lowpass must be a resolution in A (0 = none) or auto, got '{d['lowpass']:g}'")
    d["highpass"] = 0.0 if d["highpass"] is None else _num(d["highpass"], "highpass")
    # mask
    thr = [(k, m) for k, m in (("automask_threshold", "intensity"), ("automask_fraction", "volume"), ("automask_sigma", "sigma")) if d[k] is not None]
    d["threshold_method"], d["threshold_value"] = "intensity", 0.0
    if d["automask"]:
        if d["mask"] is not None:
            raise PromptError(f"ERROR: {prog}: --mask and --automask exclude each other")
        if d["automask_input"] is not None and _num(d["automask_input"], "automask_input") != 0:
            raise PromptError(f"ERROR: {prog}: --automask_input {d['automask_input']} is not supported by this build (only 0, the mean of the half maps)")
        if len(thr) != 1:
            raise PromptError(f"ERROR: {prog}: --automask needs one of --automask_threshold, --automask_fraction, --automask_sigma, got {len(thr)}")
        d["threshold_method"], d["threshold_value"] = thr[0][1], _num(d[thr[0][0]], thr[0][0])
        if d["threshold_method"] == "volume" and not 0 < d["threshold_value"] <= 1:
            raise PromptError(f"ERROR: {prog}: --automask_fraction must lie in (0, 1], got '{d['threshold_value']:g}'")
        d["automask_lp"] = 0.0 if d["automask_lp"] is None else _num(d["automask_lp"], "automask_lp")
        if not d["automask_lp"] >= 0:
            raise PromptError(f"ERROR: {prog}: --automask_lp must not be negative (0 = none), got '{d['automask_lp']:g}'")
    else:
        if thr or d["automask_lp"] is not None or d["automask_input"] is not None:
            raise PromptError(f"ERROR: {prog}: --automask_* options need --automask")
        d["automask_lp"] = 0.0
    d["mask_mode"] = "auto" if d["automask"] else "external" if d["mask"] is not None else "none"
    # phase randomisation
    if d["randomize_below_fsc"] is not None and d["randomize_beyond"] is not None:
        raise PromptError(f"ERROR: {prog}: --randomize_below_fsc and --randomize_beyond exclude each other")
    if d["randomize_beyond"] is not None:
        d["randomize"], d["randomize_value"] = "resolution", _num(d["randomize_beyond"], "randomize_beyond")
        if not d["randomize_value"] > 0:
            raise PromptError(f"ERROR: {prog}: --randomize_beyond must be a positive resolution in A, got '{d['randomize_value']:g}'")
    else:
        d["randomize"] = "fsc"
        d["randomize_value"] = POSTPROCESSING_RANDOMIZE_FSC if d["randomize_below_fsc"] is None else _num(d["randomize_below_fsc"], "randomize_below_fsc")
    if d["refine_res_lim"] is not None:
        d["refine_res_lim"] = _num(d["refine_res_lim"], "refine_res_lim")
    return d


RESMAP_FLAGS = ("noguiSplit", "noguiSingle", "doBenchMarking")
RESMAP_VALUES = ("vxSize", "pVal", "minRes", "maxRes", "stepRes", "maskVol")
RESMAP_DEFAULTS = dict(pVal=0.05, minRes=0.0, maxRes=0.0, stepRes=1.0)      # tabs.sharpen.resmap_* (config/pyp_config.toml:9222-9248)
RESMAP_MIN_STEP = 0.25


def parse_resmap(argv):
    """ResMap as PYP's Post-processing block starts it (src/pyp_main.py:6826): `--noguiSplit --vxSize A --doBenchMarking --pVal P
    --minRes=V --maxRes=V --stepRes=V [--maskVol F] half1 half2`.  A value may follow its option or be joined to it by `=` (that line
    mixes both).  --noguiSplit is required, --noguiSingle (one map, no halves) is refused, --doBenchMarking is accepted and ignored;
    --vxSize may be left out (the header's pixel size is used then).  Refused here: what can be told from the command line alone."""
    prog = "resmap"
    d = {k: False for k in RESMAP_FLAGS}
    d.update({k: None for k in RESMAP_VALUES})
    pos = []
    a = list(argv)
    i = 0
    while i < len(a):
        tok = a[i]
        i += 1
        if not tok.startswith("--"):
            pos.append(tok)
            continue
        name, eq, val = tok[2:].partition("=")
        if name in RESMAP_FLAGS:
            if eq:
                raise PromptError(f"ERROR: {prog}: option --{name} takes no value")
            d[name] = True
        elif name in RESMAP_VALUES:
            if not eq:
                if i >= len(a):
                    raise PromptError(f"ERROR: {prog}: option --{name} needs a value")
                val = a[i]
                i += 1
            if d[name] is not None:
                raise PromptError(f"ERROR: {prog}: option --{name} given twice")
            d[name] = val
        else:
            raise PromptError(f"ERROR: {prog}: unknown option '{tok}'")
    if d["noguiSingle"]:
        raise PromptError(f"ERROR: {prog}: --noguiSingle (one map) is not supported by this build; the noise is taken from two half maps (--noguiSplit)")
    if not d["noguiSplit"]:
        raise PromptError(f"ERROR: {prog}: --noguiSplit is required (this build has no graphical mode)")
    if len(pos) != 2:
        raise PromptError(f"ERROR: {prog}: expected the two half maps, got {len(pos)} positional arguments")
    d["half1"], d["half2"] = pos
    if d["vxSize"] is not None:
        d["vxSize"] = _num(d["vxSize"], "vxSize")
        if not d["vxSize"] > 0:
            raise PromptError(f"ERROR: {prog}: --vxSize must be positive, got '{d['vxSize']:g}'")
    for k, v in RESMAP_DEFAULTS.items():
        d[k] = v if d[k] is None else _num(d[k], k)
    if not 0 < d["pVal"] < 1:
        raise PromptError(f"ERROR: {prog}: --pVal must lie strictly between 0 and 1, got '{d['pVal']:g}'")
    if not d["minRes"] >= 0 or not d["maxRes"] >= 0:
        raise PromptError(f"ERROR: {prog}: --minRes and --maxRes must not be negative (0 = the default)")
    if not d["stepRes"] >= RESMAP_MIN_STEP:
        raise PromptError(f"ERROR: {prog}: --stepRes must be at least {RESMAP_MIN_STEP:g} A, got '{d['stepRes']:g}'")
    return d


def resmap_output_names(half1):
    """(<half1 without suffix>_ori_resmap<suffix>, <half1 without suffix>_ori_resmap_chimera.cmd): where src/pyp_main.py:6831-6843 looks."""
    import os
    stem, suffix = os.path.splitext(half1)
    return stem + "_ori_resmap" + suffix, stem + "_ori_resmap_chimera.cmd"


def dump_name(seed, k):
    """'…_map1_n.mrc', 3 -> '…_map1_n3.mrc' (the index goes before '.mrc', frealign.py:1870-1876)."""
    if seed.endswith(".mrc"):
        return seed[:-4] + str(k) + ".mrc"
    return seed + str(k)
