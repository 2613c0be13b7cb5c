"""k_global with the folded row order (quads of the row pairs t and Ns/2 - t, pyp_amd/csrc/ppm_rows.h) against the CPU oracle, never
against another path of the library, as test_gpu_parity.test_global_grid_search_matches_oracle_exactly does: the hits stay on the
grid (iters_hit = -1); same grid point (angular error below 1e-4 deg), same integer shift, |dSCORE| < 0.01.  The cases
(tests/global_fold_cases.py) are the smallest at which the fold can go wrong; tests/test_global_fold_margins_cpu.py shows on the CPU
that no particle's best two grid scores are closer than 1e-5, so that the equalities cannot hinge on rounding.  No particle is
excluded."""
import numpy as np
import pytest

import global_fold_cases as G
from pyp_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(G.CASES))
def test_folded_grid_search_matches_oracle_exactly(case, monkeypatch):
    from oracle import oracle as O
    from pyp_amd import host as H
    box, band, astep, R, path = G.CASES[case]
    vol, imgs, rows = G.dataset(box)
    c = G.cfg_for(box, band, astep, R)
    d = O.band_dims(c)
    assert d["Ns"] == G.NS and d["RSx"] == d["RSy"] == R, d
    if path:
        monkeypatch.setenv("PPM_GLOBAL_PATH", path)
    else:
        monkeypatch.delenv("PPM_GLOBAL_PATH", raising=False)
    want, counts = O.refine_batch(O.Reference(vol, box / 2), c, imgs, rows)
    g = H.Reference(vol, box / 2, device=0)
    got = g.refine(c, imgs, rows)
    assert g.last_counts()["n_global"] == counts[0]
    step = G.grid_step_px(box) * G.PX
    ang = synth.angular_error_deg(want, got)
    dsc = np.abs(want[:, 14] - got[:, 14])
    print("FOLD %s: max angular difference %.3g deg, max |dSCORE| %.3g" % (case, ang.max(), dsc.max()))
    assert ang.max() < 1e-4                                                              # same grid point
    assert np.array_equal(np.round(want[:, 4:6] / step), np.round(got[:, 4:6] / step))   # same integer shift
    assert dsc.max() < 0.01                                                              # SCORE is 100 x cc
