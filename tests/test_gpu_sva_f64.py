"""The sub-tomogram path (ppm_sva_insert, and ppm_sva_align at a given pose) against the float64 restatement tests/f64_sva.py, one
case per box and launch plan: the two-step transforms (k_sva_x16 / k_sva_yz16) with 16 lines per block at 32, 48, 112 (M = 2, 3, 7),
192 (fft16m<12> / <-12>) and 256 (nl M = 256 exactly) and with 8 lines at 288 and 512 (M = 32, the window and twiddle tables full);
the staged transforms (k_sva_xpass + k_fft_lines) with L = 16, 14, 10, 12 lines at 40, 42, 50, 54, with L = 15 at 270 and with
k_sva_xpass's largest LDS request at 490; PPM_SVA_GENERIC_FFT=1 and PPM_SVA_FOLD=0 at 48 and 288; C3, D2 and two batches of the gather.

Average: `Accumulator.sva_insert` on 4 seeded sub-volumes (two kinds of pose x two wedges, the last one 40 sigma off zero, index
3 v + 1) against f64_sva.insert with f64_ref.compare_by_shell - worst shell below SHELL_K x, worst voxel below VOXEL_K x
floor_model_sva; weights equal; exactly zero outside the band and on the non-canonical half of qx = 0.  Voxels within 1e-3 px of a
wedge-limit plane are left out (at most 0.5 %, tests/test_f64_sva_cpu.py).  At 490 and 512: 2 sub-volumes, compared on a seeded sample
of 2e5 in-band voxels plus the planes qx = 0 and qx = 1.

Scores: `Reference.sva_align` with tol_angle = tol_shift = 0 under three settings (f64_sva.score_settings): the poses come back bit
for bit, every score within MAP_K x floor_model_sva of f64_sva.score.  At 490 and 512 a float64 score costs ~5 s, so the default band
and the no-wedge setting are compared on sub-volume 0 and the windowed setting on both (sub-volume 1 is the one 40 sigma off zero,
whose bound carries the model's offset term; sub-volume 0 holds that setting to the bound without it); the GPU scores all of them.

Error model (f64_sva.floor_model_sva): float32 line transforms, positions, shift phase in revolutions, hardware sine; on the two-step
path, which transforms the RAW volume and normalises afterwards, the term offset_sigmas x 3 log2 N for a sub-volume whose mean is that
many standard deviations off zero (the staged path and PPM_SVA_GENERIC_FFT normalise before the transform: no such term).  The
headroom constants are those of the box sweep (f64_ref.SHELL_K, VOXEL_K, MAP_K).  Measured floors: CHANGELOG.md.
"""
import functools
import json
import time

import numpy as np
import pytest

import f64_ref as R
import f64_sva as S
from pyp_amd.abi import SvaCfg

pytestmark = pytest.mark.gpu

VARIANT_BOXES = (48, 288)
CASES = []
for _n in S.GPU_BOXES:
    CASES.append((_n, "default"))
    if _n in VARIANT_BOXES:                      # next to the box's own case: they share its float64 results
        CASES += [(_n, "generic"), (_n, "nofold")]


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


def report(kind, N, **kw):
    print("FLOOR " + json.dumps(dict(kind=kind, box=N, **kw)))


def two_step(N, variant="default"):
    return N % 16 == 0 and variant != "generic"


class F64:
    """The float64 side of a case: transforms, average, excluded voxels; scores on demand."""

    def __init__(self, N, nv=None, sym="C1"):
        self.c = c = S.gpu_case(N, nv)
        self.N, self.sym = N, sym
        self.T = [S.transform(v) for v in c["vols"]]
        self.vox = S.voxel_sample(N, S.N_SAMPLE, N) if N in S.SAMPLED else None
        self.want, self.counts, self.near, self.n_in = S.insert(N, None, c["wedges"], c["poses"], c["index"], R.symmetry_ops(sym),
                                                                voxels=self.vox, transforms=self.T)
        self.cube = None
        self.scores = {}

    def score(self, k, cfg, v):
        if (k, v) not in self.scores:
            if self.cube is None:
                self.cube = S.reference_cube(self.c["ref"])
                self.samples = {}
            if k not in self.samples:
                self.samples = {k: S.band_samples(cfg)}          # one list at a time (35 M samples at 512), cut from one half-space grid per box
            c = self.c
            T = self.T[v] if not any(cfg.window) else S.transform(c["vols"][v], cfg)
            self.scores[(k, v)] = S.score(self.cube, cfg, T, c["wedges"][v], c["poses"][v], self.samples[k])
        return self.scores[(k, v)]


@functools.lru_cache(maxsize=1)
def f64_of(N):
    return F64(N)


def check_average(H, f, offset_sigmas, tag):
    """Accumulator.sva_insert of the case against f.want; returns the figures."""
    c, N = f.c, f.N
    NX = N // 2 + 1
    model = S.floor_model_sva(N, S.P_MAX, offset_sigmas)
    acc = H.Accumulator(N, 1.0, f.sym)
    acc.sva_insert(SvaCfg.make(N, use_missing_wedge=1), c["vols"], c["wedges"], c["poses"], c["index"])
    got = acc.download().reshape(2, N, N, NX, 3)
    counts = acc.counts()
    acc.close()
    assert counts == f.counts
    mask = S.inband_mask(N)
    for z in range(N):                                   # nothing outside |q| < N/2 - 1 or on the non-canonical half of qx = 0
        assert not got[:, z][:, ~mask[z]].any(), (N, z - N // 2)
    if f.vox is None:
        g, w = S.without(got, f.near), S.without(f.want, f.near)
        del got
        weights_equal = np.array_equal(g[..., 2], w[..., 2])
        rep = R.compare_by_shell(g, w, N)
        n_cmp = f.n_in
    else:
        g = got.reshape(2, -1, 3)[:, f.vox, :].astype(np.float64)
        del got
        g, w = S.without(g, f.near), S.without(f.want, f.near)
        weights_equal = np.array_equal(g[..., 2], w[..., 2])
        rep = S.compare_at(g, w, N, f.vox)
        n_cmp = len(f.vox)
    share = float(f.near.sum() / n_cmp)
    out = dict(model=model, shell=rep.max_shell_rel / model, voxel=rep.max_voxel_rel / model, excluded=share, where=str(rep), case=tag)
    report("average", N, **out)
    assert share <= S.EXCLUDED_CAP
    assert weights_equal, (N, tag, int((g[..., 2] != w[..., 2]).sum()))
    assert rep.max_shell_rel <= R.SHELL_K * model, f"box {N} {tag}: {rep}"
    assert rep.max_voxel_rel <= R.VOXEL_K * model, f"box {N} {tag}: {rep}"
    return out


def check_scores(H, f, raw_transform, tag):
    """Reference.sva_align at the given poses under the three settings against f.score."""
    c, N = f.c, f.N
    ref = H.Reference(c["ref"], N / 2)
    worst, fails, largest = 0.0, [], {0.0: 0.0, 1.0: 0.0}          # largest |GPU - float64| without / with the density offset
    for k, cfg in enumerate(S.score_settings(N)):
        poses, got = ref.sva_align(cfg, c["vols"], c["wedges"], c["poses"])
        assert np.array_equal(poses, c["poses"]), (N, tag, k)
        which = range(c["nv"]) if N not in S.SAMPLED else ((0, 1) if k == 1 else (0,))
        for v in which:
            bound = R.MAP_K * S.floor_model_sva(N, S.P_MAX, S.OFFSET_SIGMAS * c["offset"][v] if raw_transform else 0.0)
            err = abs(float(got[v]) - f.score(k, cfg, v))
            worst = max(worst, err / bound)
            largest[float(c["offset"][v])] = max(largest[float(c["offset"][v])], err)
            if err > bound:
                fails.append((k, v, float(got[v]), f.score(k, cfg, v), err, bound))
    ref.close()
    report("scores", N, worst_of_bound=worst, largest_plain=largest[0.0], largest_offset=largest[1.0],
           model_plain=S.floor_model_sva(N, S.P_MAX, 0.0), case=tag)
    assert not fails, (N, tag, fails)


@pytest.mark.parametrize("N,variant", CASES, ids=[f"{n}-{v}" for n, v in CASES])
def test_average_and_scores_vs_float64(H, N, variant, monkeypatch):
    t0 = time.perf_counter()
    f = f64_of(N)
    if variant == "generic":
        monkeypatch.setenv("PPM_SVA_GENERIC_FFT", "1")
    if variant == "nofold":
        monkeypatch.setenv("PPM_SVA_FOLD", "0")
    raw = two_step(N, variant)
    t1 = time.perf_counter()
    if variant != "nofold":                                     # PPM_SVA_FOLD is read by the alignment only
        check_average(H, f, S.OFFSET_SIGMAS if raw else 0.0, variant)
    t2 = time.perf_counter()
    check_scores(H, f, raw, variant)
    report("time", N, case=variant, float64_average=t1 - t0, average=t2 - t1, scores=time.perf_counter() - t2)


@pytest.mark.parametrize("N,sym,nv", [(n, s, v) for n, s, v, g in S.MORE_AVERAGES if not g])
def test_more_averages_vs_float64(H, N, sym, nv):
    """C3 at 48 and D2 at 42 (k_sva_insert<true> with 3 and 4 operators; two-step and staged transforms); 35 sub-volumes at 32: two
    batches of the gather, 32 + 3."""
    check_average(H, F64(N, nv, sym), S.OFFSET_SIGMAS if two_step(N) else 0.0, f"{sym} x {nv}")
