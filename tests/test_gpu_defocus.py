"""k_defocus (pyp_amd/csrc/ppm_kernels2.h) against the oracle's double-precision score of every offset: every count of offsets up to
the cap, both trips of the final ring reduction, every shape of chunk, the classification band with chunks, and the host rule that
turns (range, step) into offsets.  Inputs, reference table and plans: tests/defocus_cases.py; that the table is the oracle's own
defocus stage and that the exact-choice inputs are decisive (best - runner-up > 4 tol for every particle) is checked without a GPU
by tests/test_defocus_table_cpu.py.

All runs use global_search=0, local_refine=0, refine_defocus=1: the pose is the row's in both implementations, and nothing but
k_defocus, with k_prep in front of it, is under test.

tol is the score bound of leg B of tests/test_gpu_box_sweep.py, 2e-5 max(1, N / 64): float32 round-off of a normalised sum over the
in-band samples.  k_defocus adds one operation to that path, `dsum += 2 k step` in float: one more rounding of dsum, eps32 / 2
relative, where ctf_from_row has already rounded dsum to float once; the CTF phase of every score of the plain path carries that
error already, so no term is added to tol for it.  Measured: 1.1e-7 .. 1.4e-7 in every case, two orders below tol (CHANGELOG.md)."""
import json

import numpy as np
import pytest

import defocus_cases as D
from defocus_cases import DF1, DF2, SCORE

pytestmark = pytest.mark.gpu
SIGMA, LOGP = 13, 12


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def refs(H, O):
    """(HIP reference, oracle reference) per box, built once"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = (H.Reference(D.volume(n), n / 2), O.Reference(D.volume(n), n / 2))
        return made[n]
    yield get
    made.clear()


@pytest.fixture(scope="module")
def yardstick(O, refs):
    """(reference table, oracle rows, oracle counts) of a case, computed once and left unchanged"""
    made = {}

    def get(key, n, px, rhi, nt, step, imgs, rows, **kw):
        if key not in made:
            o = refs(n)[1]
            tab = D.table(O, o, D.cfg_for(n, px, rhi), imgs, rows, nt, step)
            want, cw = O.refine_batch(o, D.cfg_for(n, px, rhi, refine_defocus=1, defocus_range=nt * step, defocus_step=step, **kw), imgs, rows)
            for a in (tab, want, cw):
                a.setflags(write=False)
            made[key] = (tab, want, cw)
        return made[key]
    return get


def report(case, **kw):
    print("FLOOR " + json.dumps(dict(leg="defocus", case=case, **kw)))


def run(g, O, n, px, rhi, nt, step, pl, imgs, rows, knob=0, **kw):
    """One refinement; the plan the case claims is the plan the rules give for this config."""
    cfg = D.cfg_for(n, px, rhi, refine_defocus=1, defocus_range=nt * step, defocus_step=step, **kw)
    assert D.plan(D.steps(cfg.defocus_range, cfg.defocus_step), O.band_dims(cfg)["B"] + 2, knob) == tuple(pl)
    got = g.refine(cfg, imgs, rows)
    return got, g.last_counts()


def check(case, O, o, n, px, rhi, nt, step, pl, imgs, rows, tab, cw, got, lc, exact=True):
    """Assertions 1 - 5 of a case (1, the choice, only where the inputs are decisive); returns the offset indices the GPU chose."""
    bt = D.choose(tab, nt)
    k = np.rint((got[:, DF1] - rows[:, DF1]) / step).astype(int)
    assert np.abs(k).max() <= nt
    at = np.arange(len(tab))
    err = float(np.abs(got[:, SCORE] / 100.0 - tab[at, k + nt]).max())
    back = float(np.abs(O.score_batch(o, D.cfg_for(n, px, rhi), imgs, got) - got[:, SCORE] / 100.0).max())
    regret = float((tab.max(axis=1) - tab[at, k + nt]).max())
    report(case, box=n, plan=list(pl), score=err, round_trip=back, regret=regret, tol=D.tol(n), min_margin=float(D.margins(tab).min()))
    # 1. the written defocus is the row's plus the offset: the oracle's offset where the inputs are decisive
    assert np.array_equal(got[:, DF1], rows[:, DF1] + k * float(step)) and np.array_equal(got[:, DF2], rows[:, DF2] + k * float(step))
    if exact:
        assert np.array_equal(k + nt, bt), (k + nt, bt)
    else:
        assert regret <= 2 * D.tol(n)
    assert err < D.tol(n)                                   # 2. the score is the reference score of that offset
    assert back < D.tol(n)                                  # 3. the written defocus is the scored one
    assert (lc["n_local"], lc["samples_local"]) == (cw[1], cw[2])          # 4.
    return k + nt


@pytest.mark.parametrize("name", list(D.COUNTS))
def test_every_count_of_offsets_chooses_and_scores_like_the_table(H, O, refs, yardstick, name):
    """T = 3 .. 41 at box 64, every offset the optimum of one particle: T = 31 fills one trip of the final reduction but for one
    offset's lanes, T = 33 takes a second trip for a single offset, T = 41 is the cap."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.count_case(name)
    g, o = refs(n)
    tab, want, cw = yardstick(name, n, D.PX, rhi, nt, step, imgs, rows)
    got, lc = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows)
    bt = check(name, O, o, n, D.PX, rhi, nt, step, pl, imgs, rows, tab, cw, got, lc)
    assert sorted(bt) == list(range(2 * nt + 1))            # every offset index won once
    assert np.array_equal(got[:, [DF1, DF2]], want[:, [DF1, DF2]])


@pytest.mark.parametrize("knob", list(D.KNOBS))
def test_chunk_cuts_give_the_rows_of_one_chunk(H, O, refs, yardstick, monkeypatch, knob):
    """PPM_DEFOCUS_CHUNK cuts the 41 offsets into chunks of 1 .. 40: a last chunk shorter than the others, tables zeroed between
    chunks, sumB behind the full-length tables.  Every offset has its own per-wave tables, filled by the same waves in the same
    order of samples whatever the chunking, and combined in a fixed order: the rows are the unchunked rows bit for bit."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.count_case("nt20")
    g, o = refs(n)
    tab, want, cw = yardstick("nt20", n, D.PX, rhi, nt, step, imgs, rows)
    one, _ = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows)
    monkeypatch.setenv("PPM_DEFOCUS_CHUNK", str(knob))
    got, lc = run(g, O, n, D.PX, rhi, nt, step, D.KNOBS[knob], imgs, rows, knob=knob)
    check(f"knob{knob}", O, o, n, D.PX, rhi, nt, step, D.KNOBS[knob], imgs, rows, tab, cw, got, lc)
    assert np.array_equal(got, one)


@pytest.mark.parametrize("name", list(D.LARGE))
def test_production_chunk_rule(H, O, refs, yardstick, name):
    """No knob: the chunks the 60 000-byte rule cuts at boxes 192 (38 + 3) and 240 (30 + 1, 30 + 11), with the dynamic LDS request
    that goes with them; optima at t = 0, nt, 31, 32, TC - 1, TC, T - 2, T - 1."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.large_case(name)
    g, o = refs(n)
    tab, want, cw = yardstick(name, n, D.PX, rhi, nt, step, imgs, rows)
    got, lc = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows)
    bt = check(name, O, o, n, D.PX, rhi, nt, step, pl, imgs, rows, tab, cw, got, lc)
    T, tc = pl[0], pl[1]
    assert {t for t in (0, nt, 31, 32, tc - 1, tc, T - 2, T - 1) if t < T} <= set(bt)
    assert np.array_equal(got[:, [DF1, DF2]], want[:, [DF1, DF2]])


def test_classification_band_with_chunks(H, O, refs, yardstick):
    """Box 192, 38 + 3: the chosen offset is scored once more over the classification band, also where it lies in the last chunk
    (t >= 38).  SIGMA and LOGP under the bounds of test_classification_limit_moves_logp_and_sigma_like_the_oracle; every other column
    as without the limit."""
    name = "box192-nt20"
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.large_case(name)
    g, o = refs(n)
    g0, _ = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows)
    tab, w1, cw = yardstick(name + "-cls", n, D.PX, rhi, nt, step, imgs, rows, res_classification=D.PX * n / 40.0)
    g1, lc = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows, res_classification=D.PX * n / 40.0)
    bt = check(name + "-cls", O, o, n, D.PX, rhi, nt, step, pl, imgs, rows, tab, cw, g1, lc)
    assert (bt >= pl[1]).sum() >= 3                          # optima in the last chunk
    keep = [c for c in range(32) if c not in (LOGP, SIGMA)]
    assert np.array_equal(g0[:, keep], g1[:, keep]) and not np.allclose(g0[:, LOGP], g1[:, LOGP])
    assert np.abs(w1[:, SIGMA] - g1[:, SIGMA]).max() < 2e-4 and np.abs(w1[:, LOGP] - g1[:, LOGP]).max() < 2e-3 * np.abs(w1[:, LOGP]).max()


@pytest.mark.parametrize("name", list(D.RULES))
def test_range_and_step_give_the_oracles_offsets(H, O, refs, name):
    """The rule from (range, step) to offsets, end to end on 4 particles: DF and the evaluation counts are the oracle's.  A range
    below one step leaves the rows and counts of a run without defocus refinement; 5000 / 100 stops at the cap of 20; 0.3 / 0.1 is
    3 through the 1e-6 (rows 50 A off their optimum: the reference score moves by 1.6e-6 .. 1.5e-5 per 0.1 A towards it,
    tests/test_defocus_table_cpu.py, and the float error of neighbouring offsets is shared, so the end of the range wins in both;
    the offset itself is the float product k step, within eps32 |k step| of the oracle's double product)."""
    n, rhi = 64, D.RHI64
    g, o = refs(n)
    rng_, step, nt, imgs, rows, optima = D.rule_case(name)
    assert D.steps(rng_, step) == nt
    cfg = D.cfg_for(n, D.PX, rhi, refine_defocus=1, defocus_range=rng_, defocus_step=step)
    want, cw = O.refine_batch(o, cfg, imgs, rows)
    got = g.refine(cfg, imgs, rows)
    lc = g.last_counts()
    assert cw[1] == 1 + 2 * nt and (lc["n_local"], lc["samples_local"]) == (cw[1], cw[2])
    kw, kg = np.rint((want[:, DF1] - rows[:, DF1]) / step), np.rint((got[:, DF1] - rows[:, DF1]) / step)
    report(name, box=n, nt=nt, oracle=kw.tolist(), gpu=kg.tolist(), score=float(np.abs(want[:, SCORE] - got[:, SCORE]).max() / 100.0))
    assert np.array_equal(kw, kg)
    if nt == 0:
        off = g.refine(D.cfg_for(n, D.PX, rhi), imgs, rows)
        assert np.array_equal(got, off) and g.last_counts() == lc and np.array_equal(got[:, [DF1, DF2]], rows[:, [DF1, DF2]])
    elif step >= 1.0:
        assert np.array_equal(got[:, [DF1, DF2]], want[:, [DF1, DF2]]) and set(kg + nt) == set(optima)
    else:
        s = float(np.float32(step))
        assert np.abs(kg).max() == nt
        assert np.abs((got[:, DF1] - rows[:, DF1]) - kw * s).max() <= D.EPS32 * nt * s + 1e-11       # 1e-11: the double sum row + offset
        assert np.abs((got[:, DF2] - got[:, DF1]) - (rows[:, DF2] - rows[:, DF1])).max() <= 1e-11
    assert np.abs(want[:, SCORE] - got[:, SCORE]).max() / 100.0 < D.tol(n)


def test_a_step_float32_cannot_hold(H, O, refs, yardstick):
    """33.3 A: the kernel writes the float product k step that it scored, the oracle the double product of k and the config's float
    step; they differ by at most eps32 |k step|.  The choice is the oracle's, DF2 - DF1 is unchanged and the written defocus is
    the scored one."""
    n, rhi = 64, D.RHI64
    rng_, step, nt, imgs, rows, _ = D.step33_case()
    g, o = refs(n)
    s = float(np.float32(step))
    cfg = D.cfg_for(n, D.PX, rhi, refine_defocus=1, defocus_range=rng_, defocus_step=step)
    assert D.steps(rng_, step) == nt
    tab = D.table(O, o, D.cfg_for(n, D.PX, rhi), imgs, rows, nt, step)
    want, cw = O.refine_batch(o, cfg, imgs, rows)
    got = g.refine(cfg, imgs, rows)
    lc = g.last_counts()
    bt = D.choose(tab, nt)
    assert np.array_equal(want[:, DF1], rows[:, DF1] + (bt - nt) * s)
    k = np.rint((got[:, DF1] - rows[:, DF1]) / s).astype(int)
    at = np.arange(len(tab))
    err = float(np.abs(got[:, SCORE] / 100.0 - tab[at, k + nt]).max())
    back = float(np.abs(O.score_batch(o, D.cfg_for(n, D.PX, rhi), imgs, got) - got[:, SCORE] / 100.0).max())
    report("step33.3", box=n, plan=list(D.plan(nt, D.nrings_of(rhi))), score=err, round_trip=back, min_margin=float(D.margins(tab).min()), tol=D.tol(n))
    assert np.array_equal(k + nt, bt)
    assert (np.abs(got[:, DF1] - want[:, DF1]) <= D.EPS32 * np.abs(k * s) + 1e-11).all()           # 1e-11: the double sum row + offset
    assert np.abs((got[:, DF2] - got[:, DF1]) - (rows[:, DF2] - rows[:, DF1])).max() <= 1e-11
    assert err < D.tol(n) and back < D.tol(n)
    assert (lc["n_local"], lc["samples_local"]) == (cw[1], cw[2])


def test_an_image_of_zeros_keeps_its_defocus(H, O, refs, yardstick):
    """Every offset of an empty image scores 0: the tie goes to the unshifted offset.  Its neighbours in the batch are unaffected."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.count_case("nt8")
    g, o = refs(n)
    got0, _ = run(g, O, n, D.PX, rhi, nt, step, pl, imgs, rows)
    z = 5
    blank = imgs.copy(); blank[z] = 0.0
    got, _ = run(g, O, n, D.PX, rhi, nt, step, pl, blank, rows)
    assert np.array_equal(got[z, [DF1, DF2]], rows[z, [DF1, DF2]]) and got[z, SCORE] == 0.0
    others = [i for i in range(len(rows)) if i != z]
    assert np.array_equal(got[others], got0[others]) and not np.array_equal(got0[z, [DF1, DF2]], rows[z, [DF1, DF2]])


@pytest.mark.parametrize("name", list(D.PYP))
def test_pyp_ranges_on_noisy_data(H, O, refs, yardstick, name):
    """PYP's 500 / 50 and 750 / 50 at 2 A pixels, snr 0.5: neighbouring offsets lie closer than tol in the reference table, so the
    choice may differ from the oracle's; the score of the chosen offset, the round trip and the counts hold as everywhere, and the
    regret is bounded: reference score at the GPU's offset >= reference maximum - 2 tol, for every particle."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.pyp_case(name)
    assert D.steps(D.PYP[name][0], step) == nt
    g, o = refs(n)
    tab, want, cw = yardstick("pyp" + name, n, D.PYP_PX, rhi, nt, step, imgs, rows)
    got, lc = run(g, O, n, D.PYP_PX, rhi, nt, step, pl, imgs, rows)
    check("pyp" + name, O, o, n, D.PYP_PX, rhi, nt, step, pl, imgs, rows, tab, cw, got, lc, exact=False)
