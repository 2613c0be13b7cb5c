"""Inputs, reference and plans of the defocus refinement (k_defocus, pyp_amd/csrc/ppm_kernels2.h), shared by
tests/test_defocus_plan_cpu.py, tests/test_defocus_table_cpu.py, tests/test_gpu_defocus.py and tests/test_gpu_csp.py.

The yardstick is the oracle's own score in double: a score-only pass (global_search=0, local_refine=0) at a row whose DF1 / DF2 were
moved by (t - nt) step IS the score of offset t (`table`).  The inputs are ladders: particle i starts k_i steps off its true defocus, so
its optimum is offset index nt - k_i and, with k = -nt .. nt, every index is the optimum of exactly one particle (`ladder`).

`steps`, `chunk` and `plan` mirror pyp_amd/csrc/ppm_defocus_plan.h (held to the compiled header by tests/test_defocus_plan_cpu.py), so
that a GPU case can assert the path it claims to take."""
import functools

import numpy as np

from pyp_amd import synth
from pyp_amd.abi import RefineCfg

MAX_STEPS = 20                  # PPM_MAX_DEFOCUS_STEPS (include/ppm.h)
TABLE_BYTES = 60000             # ppm::kDefocusTableBytes
DF1, DF2, SCORE = 6, 7, 14
EPS32 = float(np.finfo(np.float32).eps)


# ----------------------------------------------------------------------------------------------- the two host rules
def steps(range_, step, wide=False, cap=MAX_STEPS):
    """ppm::defocus_steps.  The configs hold floats; the refinement divides float by float, csp (wide) float by double."""
    r, s = np.float32(range_), np.float32(step)
    if not (s > 0) or not (r >= s):
        return 0
    q = float(r) / float(s) if wide else float(r / s)
    return min(int(np.floor(q + 1e-6)), cap)


def csp_steps(range_, step):
    """host_csp.h: a step that is not positive means 50 A."""
    return steps(range_, step if np.float32(step) > 0 else 50.0, wide=True)


def chunk(nt, nrings, knob=0):
    """ppm::defocus_chunk: offsets per pass over the samples; `knob` is PPM_DEFOCUS_CHUNK."""
    T = 2 * nt + 1
    tc = min(T, TABLE_BYTES // (16 * nrings)) if nrings > 0 else T
    if 0 < knob < tc:
        tc = knob
    return max(tc, 1)


def plan(nt, nrings, knob=0):
    """(T, offsets per chunk, chunks, trips of the final ring reduction in a full chunk: 32 offsets a trip)"""
    T, tc = 2 * nt + 1, chunk(nt, nrings, knob)
    return (T, tc, -(-T // tc), -(-tc // 32))


def tol(n):
    """Score bound of leg B of tests/test_gpu_box_sweep.py: float32 round-off of a normalised sum over the in-band samples."""
    return 2e-5 * max(1.0, n / 64)


# ----------------------------------------------------------------------------------------------- inputs
def cfg_for(n, px, rhi, **kw):
    """Band to rhi Fourier pixels (B = ceil(rhi) - 1, nrings = B + 2); pose and shifts stay the row's."""
    base = dict(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / rhi, res_signed_cc=30.0, global_search=0, local_refine=0)
    base.update(kw)
    return RefineCfg.make(**base)


def nrings_of(rhi):
    return int(np.ceil(rhi)) - 1 + 2


@functools.lru_cache(maxsize=None)
def volume(n):
    """synth.phantom up to box 64; above, the box-64 phantom in the middle of an empty box (a small particle in a large box: the same
    fine detail per pixel, and none of the 9 .. 17 s a phantom of 192 .. 240 voxels takes to make)."""
    if n <= 64:
        return synth.phantom(n)
    v = np.zeros((n, n, n), dtype=np.float32)
    o = n // 2 - 32
    v[o:o + 64, o:o + 64, o:o + 64] = synth.phantom(64)
    return v


@functools.lru_cache(maxsize=None)
def _dataset(n, m, px, snr):
    vol, stack, rows = synth.make_dataset(n, m, pixel=px, snr=snr, vol=volume(n))
    imgs = stack.numpy()
    imgs.setflags(write=False); rows.setflags(write=False)
    return vol, imgs, rows


def ladder(n, px, nt, step, snr, indices=None, pool=None):
    """(vol, imgs, rows, optima): rows start k_i step away from the true defocus (DF1 and DF2 alike), so the optimum of particle i is
    offset index nt - k_i = optima[i].  Default: m = 2 nt + 1 particles, optima 2 nt .. 0.  With `pool` the particles are the first m
    of a dataset of that many (the shorter ladders at box 64 are cut from the longest one's images)."""
    optima = np.arange(2 * nt, -1, -1) if indices is None else np.asarray(indices, dtype=int)
    assert optima.min() >= 0 and optima.max() <= 2 * nt
    m = len(optima)
    vol, imgs, truth = _dataset(n, max(m, pool or 0), px, snr)
    imgs, rows = imgs[:m], truth[:m].copy()
    rows[:, DF1] += (nt - optima) * float(step); rows[:, DF2] += (nt - optima) * float(step)
    return vol, imgs, rows, optima


def table(O, o, cfg0, imgs, rows, nt, step):
    """(m, 2 nt + 1) float64: the oracle's score of every row at every offset, one score_batch call per offset.  cfg0: no defocus
    refinement.  The offset is t times the step as the config's float holds it (what the oracle adds)."""
    s = float(np.float32(step))
    out = np.empty((len(rows), 2 * nt + 1))
    for t in range(2 * nt + 1):
        r = rows.copy()
        r[:, DF1] += (t - nt) * s; r[:, DF2] += (t - nt) * s
        out[:, t] = O.score_batch(o, cfg0, imgs, r)
    return out


def choose(tab, nt):
    """The oracle's choice per row of `tab`: highest score, the unshifted offset on ties, then the lower index."""
    out = np.empty(len(tab), dtype=int)
    for i, sc in enumerate(tab):
        bt, bf = nt, sc[nt]
        for t in range(len(sc)):
            if t != nt and sc[t] > bf:
                bt, bf = t, sc[t]
        out[i] = bt
    return out


def margins(tab):
    """best minus runner-up per row"""
    s = np.sort(tab, axis=1)
    return s[:, -1] - s[:, -2]


def edge_optima(nt, tc):
    """8 distinct optima at the edges of a chunked plan: t = 0, nt, 31, 32, TC - 1, TC, T - 2, T - 1, those that exist; filled up with
    their neighbours."""
    T = 2 * nt + 1
    out = []
    for t in [0, nt, 31, 32, tc - 1, tc, T - 2, T - 1, 1, nt - 1, nt + 1, tc - 2]:
        if 0 <= t < T and t not in out:
            out.append(t)
    return out[:8]


# ----------------------------------------------------------------------------------------------- cases
# Decisive inputs (tests/test_defocus_table_cpu.py holds every particle's best - runner-up above 4 tol): 1 A pixels, 100 A steps, snr 4
PX, STEP, SNR = 1.0, 100.0, 4.0
RHI64 = 0.48 * 64               # B = 30, 32 rings: every count of offsets fits one chunk

# offset counts at box 64: id -> (nt, plan).  T = 31: one trip of the reduction with idle lanes; 33: a second trip for one offset; 41: the cap
COUNTS = {f"nt{nt}": (nt, (2 * nt + 1, 2 * nt + 1, 1, 1 if 2 * nt + 1 <= 32 else 2)) for nt in (1, 8, 10, 15, 16, 17, 20)}

# chunk cuts through PPM_DEFOCUS_CHUNK at box 64, nt = 20: knob -> plan
KNOBS = {1: (41, 1, 41, 1), 2: (41, 2, 21, 1), 7: (41, 7, 6, 1), 32: (41, 32, 2, 1), 33: (41, 33, 2, 2), 40: (41, 40, 2, 2)}

# the production chunk rule, no knob: id -> (box, rhi, nt, step, plan); 8 particles at edge_optima
LARGE = {
    "box192-nt20": (192, 0.499 * 192, 20, 100.0, (41, 38, 2, 2)),           # 38 + 3
    "box240-nt15": (240, 119.5, 15, 100.0, (31, 30, 2, 1)),                 # 30 + 1: the last offset alone in its chunk
    "box240-nt20": (240, 119.5, 20, 100.0, (41, 30, 2, 1)),                 # 30 + 11
}

# PYP's own ranges on noisy data (not decisive: regret, not exact choice): id -> (range, step, nt)
PYP = {"500/50": (500.0, 50.0, 10), "750/50": (750.0, 50.0, 15)}
PYP_BOX, PYP_PX, PYP_SNR, PYP_M = 64, 2.0, 0.5, 24


def count_case(name):
    nt, pl = COUNTS[name]
    return (64, RHI64, nt, STEP, pl) + ladder(64, PX, nt, STEP, SNR, pool=2 * MAX_STEPS + 1)


def large_case(name):
    n, rhi, nt, step, pl = LARGE[name]
    return (n, rhi, nt, step, pl) + ladder(n, PX, nt, step, SNR, edge_optima(nt, pl[1]))


def pyp_case(name):
    rng_, step, nt = PYP[name]
    optima = [(i * 2 * nt) // (PYP_M - 1) for i in range(PYP_M)]
    return (PYP_BOX, RHI64, nt, step, plan(nt, nrings_of(RHI64))) + ladder(PYP_BOX, PYP_PX, nt, step, PYP_SNR, optima)


# the rule from (range, step) to offsets, end to end on 4 particles of the box-64 data: id -> (range, step, nt, optima).  Without optima
# the rows start 50 A either side of the truth: no offset in reach (nt = 0), or the end of the range wins (0.3 / 0.1, see rule_case)
RULES = {"1050/100": (1050.0, 100.0, 10, [0, 7, 14, 20]), "5000/100-cap": (5000.0, 100.0, 20, [0, 13, 27, 40]),
         "49.999/50-off": (49.999, 50.0, 0, None), "0.3/0.1": (0.3, 0.1, 3, None)}
# a step float32 cannot hold: (range, step, nt), the full ladder of nt = 10
STEP33 = (340.0, 33.3, 10)


def rule_case(name):
    """(range, step, nt, imgs, rows, optima or None)"""
    rng_, step, nt, optima = RULES[name]
    if optima is not None:
        vol, imgs, rows, optima = ladder(64, PX, nt, step, SNR, optima, pool=2 * MAX_STEPS + 1)
    else:
        vol, imgs, rows, _ = ladder(64, PX, 1, 50.0, SNR, [1, 1, 1, 1], pool=2 * MAX_STEPS + 1)        # at the truth ...
        rows[:, DF1:DF2 + 1] += np.array([50.0, -50.0, 50.0, -50.0])[:, None]                         # ... +- 50 A
    return rng_, step, nt, imgs, rows, optima


def step33_case():
    rng_, step, nt = STEP33
    return (rng_, step, nt) + ladder(64, PX, nt, step, SNR, pool=2 * MAX_STEPS + 1)[1:]


EXACT = [("count", k) for k in COUNTS] + [("large", k) for k in LARGE]


def exact_case(kind, name):
    return count_case(name) if kind == "count" else large_case(name)
