"""The GPU tests of the folded kx sum (tests/test_gpu_global_xfold.py) assert that k_global picks the oracle's grid point and integer
shift.  As tests/test_global_fold_margins_cpu.py does for the row fold, the grid scores of every particle of every case are restated
here in float64 from the oracle's own pieces, with the oracle alone on the CPU: the best and the second-best orientation must lie more
than 1e-5 apart in cc, and so must the best shift and the runner-up inside the winning orientation's window (+-RSx by +-RSy).  The
restatement is held to the oracle: its arg-max is the pose refine_batch returns."""
import numpy as np
import pytest

import f64_ref
import global_fold_cases as G
import global_xfold_cases as X
import test_global_fold_margins_cpu as M
from pyp_amd import synth

MARGIN = M.MARGIN


@pytest.mark.parametrize("case", list(X.CASES))
def test_best_two_grid_scores_are_further_apart_than_rounding(case):
    from oracle import oracle as O
    box, band, astep, (rx, ry), _ = X.CASES[case]
    vol, imgs, rows = X.data_for(case)
    c = X.cfg_for(case)
    d = O.band_dims(c)
    B, Ns = d["B"], d["Ns"]
    assert Ns == G.NS and (d["RSx"], d["RSy"]) == (rx, ry)
    o, bank = M.oracle_bank(box, band, astep)
    assert np.array_equal(vol, G.dataset(box)[0])                                     # the bank's reference is this case's
    want, _ = O.refine_batch(o, c, imgs, rows)
    dirs, n_psi = M.grid_orientations(astep)
    assert len(dirs) * n_psi == d["n_orient"]
    half = n_psi % 2 == 0
    npsi_store = n_psi // 2 if half else n_psi
    dpsi = 360.0 / n_psi
    kx, ky = np.meshgrid(np.arange(B + 1), np.arange(-B, B + 1))
    k2 = (kx * kx + ky * ky).astype(np.float64)
    r_s = box * G.PX / c.res_search
    inband = (k2 < r_s * r_s) & (k2 > 0)
    ring = np.floor(np.sqrt(k2)).astype(int)
    al = np.where(kx == 0, 1.0, 2.0)
    Ey = np.exp(2j * np.pi * np.outer(np.arange(-ry, ry + 1), np.arange(-B, B + 1)) / Ns)      # [sy][ky]
    Ex = np.exp(2j * np.pi * np.outer(np.arange(B + 1), np.arange(-rx, rx + 1)) / Ns)          # [kx][sx]
    step = G.grid_step_px(box) * G.PX
    m_or, m_sh = np.inf, np.inf
    for p in range(len(imgs)):
        I, wr = O.preprocess(c, imgs[p], c.mask_radius)
        cv = f64_ref.ctf(rows[p], box, G.PX, kx, ky) * wr[np.minimum(ring, B + 1)]
        W = np.where(inband, (al * cv * I).astype(np.complex64), 0).astype(np.complex128)
        C2 = np.where(inband, (al * cv * cv).astype(np.float32), 0).astype(np.float64)
        nI = float((al * np.abs(I.astype(np.complex128)) ** 2)[inband].sum())
        nP = (C2[None] * np.abs(bank) ** 2).sum(axis=(1, 2))
        win = np.empty((len(dirs), n_psi, 2 * ry + 1, 2 * rx + 1))
        for conj in range(2 if half else 1):
            Q = W[None] * (bank if conj else np.conj(bank))                          # psi + 180 deg: the conjugate slice
            cc = np.real(np.einsum("yk,okx,xs->oys", Ey, Q, Ex, optimize=True)) / np.sqrt(nP * nI)[:, None, None]
            win[:, conj * npsi_store:(conj + 1) * npsi_store] = cc.reshape(len(dirs), npsi_store, 2 * ry + 1, 2 * rx + 1)
        win = win.reshape(-1, 2 * ry + 1, 2 * rx + 1)
        best = win.max(axis=(1, 2))
        order = np.argsort(-best)
        b0, b1 = order[0], order[1]
        th, ph = dirs[b0 // n_psi]
        mine = want[p:p + 1].copy()
        mine[0, 1:4] = ((b0 % n_psi) * dpsi, th, ph)
        assert synth.angular_error_deg(want[p:p + 1], mine)[0] < 1e-4, (case, p)      # the restatement finds the oracle's grid point
        iy, ix = np.unravel_index(np.argmax(win[b0]), win[b0].shape)
        assert np.array_equal(np.round(want[p, 4:6] / step), [ix - rx, iy - ry]), (case, p)     # ... and its shift
        w = np.sort(win[b0].ravel())
        m_or, m_sh = min(m_or, best[b0] - best[b1]), min(m_sh, w[-1] - w[-2])
        assert best[b0] - best[b1] > MARGIN, (case, p, best[b0] - best[b1])
        assert w[-1] - w[-2] > MARGIN, (case, p, w[-1] - w[-2])
    print("MARGIN %s, %d particles: orientations >= %.3g, shifts >= %.3g" % (case, len(imgs), m_or, m_sh))
