"""The GPU tests of the folded row order (tests/test_gpu_global_fold.py) assert that k_global picks the oracle's grid point and integer
shift.  That can only be asked where the oracle's own choice does not hinge on rounding: here, with the oracle alone on the CPU, the
grid scores of every particle of every case are restated in float64 from the oracle's own pieces (its pre-processed spectra, ring
weights and slices) and the best and the second-best orientation must lie more than 1e-5 apart; so must the best shift and the
runner-up of the winning orientation's window.  The restatement is held to the oracle: its arg-max is the pose refine_batch returns."""
import functools
import math

import numpy as np
import pytest

import f64_ref
import global_fold_cases as G
from pyp_amd import synth

MARGIN = 1e-5


def grid_orientations(astep):
    """(psi, theta, phi) of the C1 grid in orientation order: directions, then in-plane angles"""
    n_theta = max(2, int(math.floor(180.0 / astep + 0.5)) + 1)
    n_psi = max(1, int(math.floor(360.0 / astep + 0.5)))
    out = []
    for i in range(n_theta):
        th = 180.0 * i / (n_theta - 1)
        n_phi = max(1, int(math.floor(360.0 * math.sin(math.radians(th)) / astep + 0.5)))
        for j in range(n_phi):
            out.append((th, 360.0 * j / n_phi))
    return out, n_psi


@functools.lru_cache(maxsize=None)
def oracle_bank(box, band, astep):
    """the oracle's reference and its stored slices of one grid (shared by the cases that differ in the window alone), left unchanged"""
    from oracle import oracle as O
    vol = G.dataset(box)[0]
    c = G.cfg_for(box, band, astep, 3)
    o = O.Reference(vol, box / 2)
    dirs, n_psi = grid_orientations(astep)
    npsi_store = n_psi // 2 if n_psi % 2 == 0 else n_psi
    bank = np.stack([O.extract_slice(o, c, k * 360.0 / n_psi, th, ph) for th, ph in dirs for k in range(npsi_store)]).astype(np.complex128)
    bank.setflags(write=False)
    return o, bank


@pytest.mark.parametrize("case", list(G.CASES))
def test_best_two_grid_scores_are_further_apart_than_rounding(case):
    from oracle import oracle as O
    box, band, astep, R, _ = G.CASES[case]
    vol, imgs, rows = G.dataset(box)
    c = G.cfg_for(box, band, astep, R)
    d = O.band_dims(c)
    B, Ns = d["B"], d["Ns"]
    assert Ns == G.NS and d["RSx"] == d["RSy"] == R
    o, bank = oracle_bank(box, band, astep)
    want, _ = O.refine_batch(o, c, imgs, rows)
    dirs, n_psi = grid_orientations(astep)
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
    s = np.arange(-R, R + 1)
    Ey = np.exp(2j * np.pi * np.outer(s, np.arange(-B, B + 1)) / Ns)             # [sy][ky]
    Ex = np.exp(2j * np.pi * np.outer(np.arange(B + 1), s) / Ns)                 # [kx][sx]
    step = G.grid_step_px(box) * G.PX
    for p in range(G.N_PART):
        I, wr = O.preprocess(c, imgs[p], c.mask_radius)
        cv = f64_ref.ctf(rows[p], box, G.PX, kx, ky) * wr[np.minimum(ring, B + 1)]
        W = np.where(inband, (al * cv * I).astype(np.complex64), 0).astype(np.complex128)
        C2 = np.where(inband, (al * cv * cv).astype(np.float32), 0).astype(np.float64)
        nI = float((al * np.abs(I.astype(np.complex128)) ** 2)[inband].sum())
        nP = (C2[None] * np.abs(bank) ** 2).sum(axis=(1, 2))
        win = np.empty((len(dirs), n_psi, 2 * R + 1, 2 * R + 1))
        for conj in range(2 if half else 1):
            Q = W[None] * (bank if conj else np.conj(bank))                          # psi + 180 deg: the conjugate slice
            cc = np.real(np.einsum("yk,okx,xs->oys", Ey, Q, Ex, optimize=True)) / np.sqrt(nP * nI)[:, None, None]
            win[:, conj * npsi_store:(conj + 1) * npsi_store] = cc.reshape(len(dirs), npsi_store, 2 * R + 1, 2 * R + 1)
        win = win.reshape(-1, 2 * R + 1, 2 * R + 1)
        best = win.max(axis=(1, 2))
        order = np.argsort(-best)
        b0, b1 = order[0], order[1]
        th, ph = dirs[b0 // n_psi]
        mine = want[p:p + 1].copy()
        mine[0, 1:4] = ((b0 % n_psi) * dpsi, th, ph)
        assert synth.angular_error_deg(want[p:p + 1], mine)[0] < 1e-4, (case, p)      # the restatement finds the oracle's grid point
        iy, ix = np.unravel_index(np.argmax(win[b0]), win[b0].shape)
        assert np.array_equal(np.round(want[p, 4:6] / step), [ix - R, iy - R]), (case, p)     # ... and its shift
        w = np.sort(win[b0].ravel())
        print("MARGIN %s particle %d: orientations %.3g, shifts %.3g" % (case, p, best[b0] - best[b1], w[-1] - w[-2]))
        assert best[b0] - best[b1] > MARGIN, (case, p, best[b0] - best[b1])
        assert w[-1] - w[-2] > MARGIN, (case, p, w[-1] - w[-2])
