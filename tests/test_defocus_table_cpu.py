"""The yardstick and the inputs of tests/test_gpu_defocus.py, checked without a GPU.

The yardstick: a table of oracle scores, one score-only pass per defocus offset (defocus_cases.table), is the oracle's own defocus
stage: same choice per particle (ties as the oracle resolves them), the reported SCORE to 1e-12, 1 + 2 nt evaluations.

The inputs: every particle of every exact-choice case has its best offset ahead of the runner-up by more than 4 tol in the reference
table (tol: the score bound of leg B of tests/test_gpu_box_sweep.py), so a kernel within tol of the reference at every offset must
choose as the oracle does; nobody is left out."""
import numpy as np
import pytest

import defocus_cases as D
from oracle import oracle as O


def _check(n, rhi, nt, step, pl, vol, imgs, rows, optima):
    o = O.Reference(vol, n / 2)
    cfg0 = D.cfg_for(n, D.PX, rhi)
    cfg = D.cfg_for(n, D.PX, rhi, refine_defocus=1, defocus_range=nt * step, defocus_step=step)
    assert D.plan(nt, O.band_dims(cfg0)["B"] + 2) == pl                   # the band gives the rings the plan was stated for
    tab = D.table(O, o, cfg0, imgs, rows, nt, step)
    want, cw = O.refine_batch(o, cfg, imgs, rows)
    bt = D.choose(tab, nt)
    assert np.array_equal(want[:, D.DF1] - rows[:, D.DF1], (bt - nt) * step) and np.array_equal(want[:, D.DF2] - rows[:, D.DF2], (bt - nt) * step)
    assert np.abs(want[:, D.SCORE] / 100.0 - tab[np.arange(len(tab)), bt]).max() < 1e-12
    assert cw[1] == 1 + 2 * nt
    mg = D.margins(tab)
    print("MARGIN " + repr(dict(box=n, nt=nt, step=step, min_margin=float(mg.min()), four_tol=4 * D.tol(n))))
    assert np.array_equal(bt, optima)                         # the ladder puts every optimum where it says
    assert (mg > 4 * D.tol(n)).all(), (mg.min(), 4 * D.tol(n))


@pytest.mark.parametrize("kind,name", D.EXACT, ids=[k for _, k in D.EXACT])
def test_table_is_the_oracles_defocus_stage_and_the_ladder_is_decisive(kind, name):
    _check(*D.exact_case(kind, name))


def test_the_other_exact_choice_inputs_are_decisive_too():
    """The 4-particle ladders of the (range, step) cases, the 33.3 A ladder (whose optima need not sit where a 100 A ladder puts them:
    the GPU test compares with the table's choice) and, for 0.3 / 0.1, the premise of its docstring: from 50 A off the optimum the
    reference score moves monotonically over the seven offsets, by more than 1.5e-6 per 0.1 A, so the end of the range wins."""
    o = O.Reference(D.volume(64), 32)
    cfg0 = D.cfg_for(64, D.PX, D.RHI64)
    for name in D.RULES:
        rng_, step, nt, imgs, rows, optima = D.rule_case(name)
        assert D.steps(rng_, step) == nt
        if nt == 0:
            continue
        tab = D.table(O, o, cfg0, imgs, rows, nt, step)
        want, cw = O.refine_batch(o, D.cfg_for(64, D.PX, D.RHI64, refine_defocus=1, defocus_range=rng_, defocus_step=step), imgs, rows)
        bt = D.choose(tab, nt)
        assert cw[1] == 1 + 2 * nt and np.array_equal(np.rint((want[:, D.DF1] - rows[:, D.DF1]) / step), bt - nt)
        if optima is not None:
            assert np.array_equal(bt, optima) and (D.margins(tab) > 4 * D.tol(64)).all()
        else:
            d = np.diff(tab, axis=1)
            assert ((d > 1.5e-6).all(axis=1) | (d < -1.5e-6).all(axis=1)).all() and set(bt) == {0, 2 * nt}
    rng_, step, nt, imgs, rows, optima = D.step33_case()
    assert D.steps(rng_, step) == nt
    tab = D.table(O, o, cfg0, imgs, rows, nt, step)
    assert (D.margins(tab) > 4 * D.tol(64)).all(), D.margins(tab).min()


@pytest.mark.parametrize("name", list(D.PYP))
def test_table_is_the_oracles_defocus_stage_on_noisy_data(name):
    """PYP's own 50 A steps at 2 A pixels: the margins fall below tol (the GPU test bounds the regret there), the table is still the
    oracle's stage."""
    n, rhi, nt, step, pl, vol, imgs, rows, optima = D.pyp_case(name)
    o = O.Reference(vol, n / 2)
    cfg0 = D.cfg_for(n, D.PYP_PX, rhi)
    cfg = D.cfg_for(n, D.PYP_PX, rhi, refine_defocus=1, defocus_range=D.PYP[name][0], defocus_step=step)
    tab = D.table(O, o, cfg0, imgs, rows, nt, step)
    want, cw = O.refine_batch(o, cfg, imgs, rows)
    bt = D.choose(tab, nt)
    assert np.array_equal(want[:, D.DF1] - rows[:, D.DF1], (bt - nt) * step) and cw[1] == 1 + 2 * nt
    assert np.abs(want[:, D.SCORE] / 100.0 - tab[np.arange(len(tab)), bt]).max() < 1e-12


def test_ties_take_the_unshifted_offset_then_the_lower_index():
    tab = np.array([[1.0, 1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 1.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 3.0, 1.0, 3.0, 0.0]])
    assert list(D.choose(tab, 2)) == [2, 0, 2, 1]
