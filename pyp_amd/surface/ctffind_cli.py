"""bin/ctffind: cistem2's ctffind 4.1 as PYP runs it (src/pyp/ctf/core.py:100-468 `ctffind4_movie`, :471-600 `ctffind4_power`), on the
GPU estimator of DESIGN.md 2g.  Three stdin scripts are honoured:

  image      input, diagnostic output, pixel, kV, Cs, amplitude contrast, tile, min res, max res, min defocus, max defocus, step,
             know the astigmatism (no), exhaustive search (ignored), restraint (yes + tolerated astigmatism | no), phase shift (no),
             [tilt (no)], expert options (no)
  movie      input, "yes", frames to average, then as above from the output name
  spectrum   with --amplitude-spectrum-input: the image form; the input is a centred full-plane AMPLITUDE spectrum (tile x tile), so
             the tile stage is skipped

For an output X.mrc it writes X.mrc (diagnostic image), X.txt (one row: 1.0 df1 df2 angle 0.0 cc res) and X_avrot.txt (six rows), each
complete or not at all.  Everything else is refused with ERROR, a non-zero exit and no output file (DESIGN.md 2g lists the refusals).
"""
import os
import sys
import time

import numpy as np

from . import prompts
from .prompts import PromptError

YES, NO = ("yes", "y"), ("no", "n")


def split_command(command):
    """A command string as PYP builds it -> (argv of the program, answers): the lines between '<< EOF' and 'EOF'."""
    lines = command.strip("\n").split("\n")
    k = next((i for i, ln in enumerate(lines) if "<<" in ln), None)
    if k is None:
        raise PromptError("ERROR: ctffind: not a here-doc command")
    head = lines[k].split(">")[0].split()
    argv = [w for w in head[head.index(next(w for w in head if w.endswith("ctffind") or w.endswith("ctffind5"))) + 1:]]
    end = lines[k].split("<<")[1].split()[0]
    body = lines[k + 1:]
    if end in body:
        body = body[:body.index(end)]
    return argv, [b.strip() for b in body]


def parse_args(argv):
    """Command-line flags: --amplitude-spectrum-input switches to the spectrum form, --omp-num-threads N is accepted and ignored,
    --old-school-input and anything else is refused."""
    spectrum, i = False, 0
    while i < len(argv):
        a = argv[i]
        if a == "--amplitude-spectrum-input":
            spectrum = True
        elif a == "--omp-num-threads":
            i += 1
        elif a.startswith("--omp-num-threads="):
            pass
        elif a == "--old-school-input":
            raise PromptError("ERROR: ctffind: --old-school-input (the ctffind3 card format) is not supported")
        else:
            raise PromptError(f"ERROR: ctffind: option '{a}' is not supported")
        i += 1
    return spectrum


def _yes(s, what):
    t = s.strip().lower()
    if t in YES:
        return True
    if t in NO:
        return False
    raise PromptError(f"ERROR: ctffind: answer for '{what}' must be yes or no, got '{s}'")


def parse_script(answers, spectrum=False, frames=None):
    """The answers of one script -> dict(input, output, movie, average, pixel, kv, cs, wgh, tile, min_res, max_res, min_def, max_def, step,
    tol, spectrum).  frames: sections of the input file where the caller has read its header - the program asks "Input is a movie" only of
    a file with several, so with one section the second answer is the output name whatever it reads.  Raises PromptError for every
    answer this build refuses."""
    a = [s for s in answers]
    while a and a[-1] == "":
        a.pop()
    if len(a) < 16:
        raise PromptError(f"ERROR: ctffind: {len(a)} answers, a ctffind 4.1 script has at least 16")
    d = dict(input=a[0], movie=False, average=1, spectrum=bool(spectrum))
    i = 1
    if a[1].strip().lower() in YES + NO and (frames is None or frames > 1):      # "Input is a movie": asked only of a file with several frames
        d["movie"] = _yes(a[1], "Input is a movie")
        i = 2
        if d["movie"]:
            d["average"] = prompts._num(a[2], "Number of frames to average together", int)
            i = 3
    if spectrum and d["movie"]:
        raise PromptError("ERROR: ctffind: an amplitude spectrum cannot be a movie")
    d["output"] = a[i]
    names = ("pixel", "kv", "cs", "wgh", "tile", "min_res", "max_res", "min_def", "max_def", "step")
    if len(a) < i + 1 + len(names) + 4:
        raise PromptError("ERROR: ctffind: the script ends before its last question")
    for k, name in enumerate(names):
        d[name] = prompts._num(a[i + 1 + k], name, int if name == "tile" else float)
    i += 1 + len(names)
    if _yes(a[i], "Do you know what astigmatism is present"):
        raise PromptError("ERROR: ctffind: 'do you know what astigmatism is present = yes' is not supported (the astigmatism is always searched)")
    _yes(a[i + 1], "Slower, more exhaustive search")           # honoured by construction: the grid is always exhaustive
    i += 2
    d["tol"] = 0.0
    if _yes(a[i], "Use a restraint on astigmatism"):
        d["tol"] = prompts._num(a[i + 1], "Expected (tolerated) astigmatism", float)        # 0 (ctf_use_ast off) = no restraint
        i += 2
    else:
        i += 1
    rest = a[i:]
    if rest and _yes(rest[0], "Find additional phase shift"):      # before the count: its follow-up answers lengthen the script
        raise PromptError("ERROR: ctffind: the phase-shift search is not supported")
    if len(rest) > 3:
        raise PromptError("ERROR: ctffind: the ctffind5 prompt sequence (or expert options) is not supported: %d answers follow the astigmatism "
                          "questions, ctffind 4.1 asks 2 or 3" % len(rest))
    if len(rest) < 2:
        raise PromptError("ERROR: ctffind: the script ends before its last question")
    if len(rest) == 3 and _yes(rest[1], "Determine sample tilt"):
        raise PromptError("ERROR: ctffind: tilt / thickness determination is not supported")
    if _yes(rest[-1], "Do you want to set expert options"):
        raise PromptError("ERROR: ctffind: expert options are not supported")
    if not prompts.resample_len_ok(d["tile"]):
        near = " and ".join(str(k) for k in prompts.resample_nearest_ok(d["tile"]) if k)
        raise PromptError(f"ERROR: ctffind: a spectrum of {d['tile']} is not a size the transforms take (even, 32..512, prime factors 2, 3, 5, 7); "
                          f"nearest: {near}")
    if d["tol"] < 0:
        raise PromptError("ERROR: ctffind: the tolerated astigmatism must not be negative")
    return d


def half_power_from_amplitude(full):
    """A centred full-plane amplitude spectrum [T, T] (as ctffind4_power builds it: row T/2 = ky 0, column T/2 = kx 0) -> the half-plane
    POWER spectrum [T, T/2 + 1] in transform order; the column kx = T/2, which the full plane does not hold, repeats kx = T/2 - 1."""
    t = full.shape[0]
    amp = np.fft.ifftshift(np.asarray(full, dtype=np.float64), axes=0)[:, t // 2:]
    amp = np.concatenate([amp, amp[:, -1:]], axis=1)
    return (amp * amp).astype(np.float32)


def output_names(output):
    stem = output[:-4] if output.lower().endswith(".mrc") else output
    return output, stem + ".txt", stem + "_avrot.txt"


def format_txt(d, row):
    """X.txt: np.loadtxt(X.txt, comments="#")[[1, 2, 3, 5, 6]] is df1, df2, angle, cc, resolution."""
    head = ["# Output from CTFFind version 4.1 (MI355X / libpypmatch), run on %s" % time.strftime("%Y-%m-%d %H:%M:%S"),
            "# Input file: %s ; Number of micrographs: 1" % d["input"],
            "# Pixel size: %.3f Angstroms ; acceleration voltage: %.1f keV ; spherical aberration: %.2f mm ; amplitude contrast: %.2f"
            % (d["pixel"], d["kv"], d["cs"], d["wgh"]),
            "# Box size: %d pixels ; min. res.: %.1f Angstroms ; max. res.: %.1f Angstroms ; min. def.: %.1f um; max. def. %.1f um"
            % (d["tile"], d["min_res"], d["max_res"], d["min_def"], d["max_def"]),
            "# Columns: #1 - micrograph number; #2 - defocus 1 [Angstroms]; #3 - defocus 2; #4 - azimuth of astigmatism; #5 - additional phase "
            "shift [radians]; #6 - cross correlation; #7 - spacing (in Angstroms) up to which CTF rings were fit successfully"]
    return "\n".join(head) + "\n%.6f %.6f %.6f %.6f %.6f %.6f %.6f\n" % (1.0, row[0], row[1], row[2], 0.0, row[3], row[7])


def format_avrot(d, avrot):
    """X_avrot.txt: np.loadtxt(..., comments="#") is [6, rings]; row 0 in 1/A."""
    head = ["# Output from CTFFind version 4.1 (MI355X / libpypmatch)", "# Input file: %s ; Number of micrographs: 1" % d["input"],
            "# 6 lines per micrograph: #1 - spatial frequency (1/Angstroms); #2 - 1D rotational average of spectrum (assuming no astigmatism); "
            "#3 - 1D rotational average of spectrum; #4 - CTF fit; #5 - cross-correlation between spectrum and CTF fit; #6 - 2sigma of expected "
            "cross correlation of noise"]
    return "\n".join(head) + "\n" + "\n".join(" ".join("%.6f" % v for v in r) for r in np.asarray(avrot)) + "\n"


def write_outputs(d, row, avrot, diag):
    """The three files, each under a temporary name until all are complete; X.txt, whose values PYP reads, takes its name last."""
    from ..formats import mrc
    out, txt, avr = output_names(d["output"])
    files = [(out, None), (avr, format_avrot(d, avrot)), (txt, format_txt(d, row))]
    tmps = [p + ".tmp%d" % os.getpid() for p, _ in files]
    try:
        mrc.write(np.asarray(diag, dtype=np.float32), tmps[0], pixel_size=d["pixel"])
        for (p, text), tmp in zip(files[1:], tmps[1:]):
            with open(tmp, "w") as f:
                f.write(text)
        for (p, _), tmp in zip(files, tmps):
            os.replace(tmp, p)
    except OSError as e:
        for tmp in tmps:
            if os.path.exists(tmp):
                os.remove(tmp)
        raise PromptError(f"ERROR: ctffind: cannot write the output files: {e}")


def _device_backend(d, data):
    """(row [8], avrot [6, rings], diag [B, B]) from the GPU, under the per-GPU lock."""
    from .. import host
    from ..abi import CtfCfg
    from .cli import gpu_lock
    dev = int(os.environ.get("PPM_DEVICE", "0"))
    cfg = CtfCfg.make(d["pixel"], kv=d["kv"], cs=d["cs"], wgh=d["wgh"], min_res=d["min_res"], max_res=d["max_res"], min_def=d["min_def"],
                      max_def=d["max_def"], step=d["step"], tol=d["tol"])
    with gpu_lock(dev):
        if d["spectrum"]:
            rows, avrot, diag = host.estimate_ctf(half_power_from_amplitude(data), cfg, profile=True, device=dev)
        else:
            rows, avrot, diag = host.estimate_ctf(data, cfg, tile=d["tile"], group=d["average"], profile=True, device=dev)
    return rows[0], avrot[0], diag[0]


def main(argv=None, stdin=None, backend=None):
    """backend(d, data) -> (row, avrot, diag) replaces the GPU (the CPU tests give the float64 model)."""
    from ..formats import mrc
    t0 = time.time()
    try:
        spectrum = parse_args(sys.argv[1:] if argv is None else argv)
        answers = prompts.read_answers(sys.stdin if stdin is None else stdin)
        if not answers or not os.path.exists(answers[0]):
            raise PromptError(f"ERROR: ctffind: input file {answers[0] if answers else ''} does not exist")
        d = parse_script(answers, spectrum, frames=int(mrc.read_header(answers[0])["nz"]))
        data = np.asarray(mrc.read(d["input"]), dtype=np.float32)
        if data.ndim == 3 and data.shape[0] == 1:
            data = data[0]
        if spectrum:
            if data.ndim != 2 or data.shape != (d["tile"], d["tile"]):
                raise PromptError(f"ERROR: ctffind: the amplitude spectrum must be {d['tile']} x {d['tile']}, got {data.shape}")
        else:
            if data.ndim == 3 and not d["movie"]:
                d["movie"], d["average"] = True, 1            # the program asks; a script without the answer treats every frame alone
            if d["movie"] and (d["average"] < 1 or d["average"] > (data.shape[0] if data.ndim == 3 else 1)):
                raise PromptError(f"ERROR: ctffind: frames to average must be 1 .. the number of frames, got {d['average']}")
            if data.shape[-1] < d["tile"] or data.shape[-2] < d["tile"]:
                raise PromptError(f"ERROR: ctffind: the image ({data.shape[-1]} x {data.shape[-2]}) is smaller than one tile of {d['tile']}")
        print("\n        **   Welcome to Ctffind (MI355X / libpypmatch)   **\n")
        for k, v in d.items():
            print(f"{k:12s}: {v}")
        row, avrot, diag = (backend or _device_backend)(d, data)
        write_outputs(d, row, avrot, diag)
    except (PromptError, ValueError, IOError, RuntimeError) as e:
        msg = str(e)
        print(msg if "ERROR" in msg else "ERROR: ctffind: " + msg, flush=True)
        return 1
    print("\nEstimated defocus values        : %.2f , %.2f Angstroms\nEstimated azimuth of astigmatism: %.2f degrees\nScore                           : %.5f"
          % (row[0], row[1], row[2], row[3]))
    print("Thon rings with good fit up to  : %.1f Angstroms" % row[7])
    print("Timing: %.2f s\n\nSummary of results                          : %s\nCtffind: Normal termination" % (time.time() - t0, output_names(d["output"])[1]))
    return 0
