"""k_global with the columns kx and kx + 32 folded ahead of the window reduction (pyp_amd/csrc/ppm_window.h) against the CPU oracle, never
against another path of the library, with the assertions of tests/test_gpu_global_fold.py: the hits stay on the grid (iters_hit = -1);
same grid point (angular error below 1e-4 deg), same integer shift, |dSCORE| < 0.01.  The cases (tests/global_xfold_cases.py) make every
row and every column of the 7 x 7 window the winner of some particle — the test asserts that coverage on the oracle's own answers —
and run the narrower windows (R = 1, 2), a window with RSx != RSy and odd particle counts.  tests/test_global_xfold_margins_cpu.py shows
on the CPU that no particle's best two grid scores are closer than 1e-5, so that the equalities cannot hinge on rounding.  No particle
is excluded."""
import numpy as np
import pytest

import global_fold_cases as G
import global_xfold_cases as X
from pyp_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(X.CASES))
def test_xfolded_grid_search_matches_oracle_exactly(case, monkeypatch):
    from oracle import oracle as O
    from pyp_amd import host as H
    box, band, astep, (rx, ry), what = X.CASES[case]
    vol, imgs, rows = X.data_for(case)
    c = X.cfg_for(case)
    d = O.band_dims(c)
    assert d["Ns"] == G.NS and (d["RSx"], d["RSy"]) == (rx, ry), d
    assert len(imgs) % 2 == 1                                                            # the last block of k_global holds one particle
    monkeypatch.delenv("PPM_GLOBAL_PATH", raising=False)
    want, counts = O.refine_batch(O.Reference(vol, box / 2), c, imgs, rows)
    step = G.grid_step_px(box) * G.PX
    if what != "five":
        # every row and every column of the window wins somewhere (asserted, never skipped)
        won = {(int(a), int(b)) for a, b in np.round(want[:, 4:6] / step)}
        assert won == {(sx, sy) for sx in range(-rx, rx + 1) for sy in range(-ry, ry + 1)}, sorted(won)
    g = H.Reference(vol, box / 2, device=0)
    got = g.refine(c, imgs, rows)
    assert g.last_counts()["n_global"] == counts[0]
    ang = synth.angular_error_deg(want, got)
    dsc = np.abs(want[:, 14] - got[:, 14])
    print("XFOLD %s: max angular difference %.3g deg, max |dSCORE| %.3g" % (case, ang.max(), dsc.max()))
    assert ang.max() < 1e-4                                                              # same grid point
    assert np.array_equal(np.round(want[:, 4:6] / step), np.round(got[:, 4:6] / step))   # same integer shift
    assert dsc.max() < 0.01                                                              # SCORE is 100 x cc
