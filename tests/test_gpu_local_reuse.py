"""k_local's full-band launch fetches the centre pose of a compass sweep first; a lane of a neighbour pose whose sample falls into the
centre's 2 x 2 x 2 cell takes the centre's taps instead of addressing the cube (pyp_amd/csrc/ppm_dev.h, "tap reuse").  Same taps, same
arithmetic, the same order of LDS adds per slot: the output rows must equal those of PPM_LOCAL_REUSE=0 (every lane gathers) in every
bit, and keep their tolerance against the oracle.  PPM_LOCAL_REUSE_COUNT=1 makes the kernel count (neighbour lane-gathers, reused ones);
the counts say that the path under test really ran, and ran on part of the lanes.  Box 64, the parity suite's synthetic set-up.
Run on the GPU box: pytest -m gpu"""
import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import RefineCfg

pytestmark = pytest.mark.gpu

ANG_TOL_DEG, SHIFT_TOL_PX = 0.1, 0.5       # BASELINE.json north_star, as in test_gpu_parity.py
M = 8


def cfg_for(n, px, **kw):
    base = dict(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / (0.375 * n), res_search=px * n / (0.16 * n),
                search_range_x=6 * px, search_range_y=6 * px, res_signed_cc=30.0)
    base.update(kw)
    return RefineCfg.make(**base)


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def d64(H, O):
    vol, stack, rows = synth.make_dataset(64, 24, pixel=2.0, snr=0.1)
    return vol, stack.numpy(), rows, H.Reference(vol, 32), O.Reference(vol, 32)


def both(monkeypatch, g, c, imgs, rows, **env):
    """rows with every lane gathering, rows with reuse, and the reuse counts of the second call"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PPM_LOCAL_REUSE_COUNT", "1")
    monkeypatch.setenv("PPM_LOCAL_REUSE", "0")
    plain = g.refine(c, imgs, rows)
    assert g.last_reuse() == (0, 0)                    # the plain instance counts nothing
    monkeypatch.delenv("PPM_LOCAL_REUSE")
    near = g.refine(c, imgs, rows)
    gathers, reused = g.last_reuse()
    print("tap reuse: %d of %d neighbour lane-gathers (%.3f)" % (reused, gathers, reused / max(gathers, 1)))
    assert np.array_equal(plain, near)
    return near, gathers, reused


def close_to_oracle(want, got, px):
    assert synth.angular_error_deg(want, got).max() < ANG_TOL_DEG
    assert synth.shift_error_px(want, got, px).max() < SHIFT_TOL_PX


def test_local_refinement_from_perturbed_rows(d64, O, monkeypatch):
    vol, imgs, rows, g, o = d64
    start = synth.perturb_rows(rows, 2.0, 1.0, 2.0)
    c = cfg_for(64, 2.0, global_search=0)
    got, gathers, reused = both(monkeypatch, g, c, imgs, start)
    assert 0 < reused < gathers
    monkeypatch.delenv("PPM_LOCAL_REUSE_COUNT")
    assert np.array_equal(got, g.refine(c, imgs, start)) and g.last_reuse() == (0, 0)     # counting changes nothing; off, it reports nothing
    want, _ = O.refine_batch(o, c, imgs, start)
    close_to_oracle(want, got, 2.0)
    assert np.abs(want[:, 14] - got[:, 14]).max() < 0.01                 # SCORE is 100 x cc


def test_full_refinement(d64, O, monkeypatch):
    vol, imgs, rows, g, o = d64
    c = cfg_for(64, 2.0, angular_step=15.0)
    got, gathers, reused = both(monkeypatch, g, c, imgs[:M], rows[:M])
    assert 0 < reused < gathers
    want, _ = O.refine_batch(o, c, imgs[:M], rows[:M])
    close_to_oracle(want, got, 2.0)


def test_first_step_decides_how_much_is_reused(d64, O, monkeypatch):
    """The steps halve from local_angle_step over the same number of iterations, so a smaller first step means smaller moves in every
    iteration and more lanes in the centre's cell.  At 0.02 degrees the band's edge (24 Fourier pixels) moves 0.008 voxels in the first
    iteration and a sample leaves its cell with a probability of about 1.5 times its move: below 1 % of the lanes address the cube, and
    most waves carry no real address at all.  At 20 degrees the first iterations move the edge of their band by more than a voxel."""
    vol, imgs, rows, g, o = d64
    start = synth.perturb_rows(rows, 2.0, 1.0, 2.0)
    frac = {}
    for step in (0.02, 2.5, 20.0):
        c = cfg_for(64, 2.0, global_search=0, local_angle_step=step)
        got, gathers, reused = both(monkeypatch, g, c, imgs[:M], start[:M])
        assert 0 < reused < gathers
        frac[step] = reused / gathers
        if step != 2.5:                                 # 2.5 degrees is the default step: the case above holds it to the oracle
            want, _ = O.refine_batch(o, c, imgs[:M], start[:M])
            close_to_oracle(want, got, 2.0)
    assert frac[0.02] > 0.95
    assert frac[20.0] < frac[2.5] < frac[0.02]


# the four flag sets of test_gpu_parity.py::test_partial_refine_flags_match_oracle (one or two free angles: fewer neighbour groups, other
# slot numbers of the centre), and no free angle at all: a single group per sweep, nothing to reuse
@pytest.mark.parametrize("flags", [dict(refine_phi=0), dict(refine_theta=0), dict(refine_psi=0, refine_x=0), dict(refine_theta=0, refine_phi=0),
                                   dict(refine_psi=0, refine_theta=0, refine_phi=0)])
def test_partial_refine_flags(d64, O, monkeypatch, flags):
    vol, imgs, rows, g, o = d64
    start = synth.perturb_rows(rows, 1.5, 0.7, 2.0, seed=11)
    c = cfg_for(64, 2.0, global_search=0, **flags)
    got, gathers, reused = both(monkeypatch, g, c, imgs[:M], start[:M])
    if c.refine_psi or c.refine_theta or c.refine_phi:
        assert 0 < reused < gathers
    else:
        assert (gathers, reused) == (0, 0)
    want, _ = O.refine_batch(o, c, imgs[:M], start[:M])
    close_to_oracle(want, got, 2.0)
    if not c.refine_x:
        assert np.allclose(got[:, 4], start[:M, 4], atol=1e-6)


def test_marching_off(d64, O, monkeypatch):
    """every iteration sweeps the full band: the first ones move its edge by more than kNearMove voxels and take the plain loop inside
    the reusing instance (gathers counted, none reused), the later ones reuse"""
    vol, imgs, rows, g, o = d64
    c = cfg_for(64, 2.0, band_factor=-1.0)
    got, gathers, reused = both(monkeypatch, g, c, imgs[:6], rows[:6])
    assert 0 < reused < gathers
    want, _ = O.refine_batch(o, c, imgs[:6], rows[:6])
    close_to_oracle(want, got, 2.0)


@pytest.mark.parametrize("n,px,m,pad", [(64, 2.0, 8, 2), (64, 2.0, 6, 4), (48, 3.0, 6, 2), (48, 3.0, 6, 4)])
def test_padded_reference(H, O, monkeypatch, n, px, m, pad):
    """the cube is sampled pad times finer: moves are pad times longer in voxels, the tables pad times wider"""
    vol, stack, rows = synth.make_dataset(n, m, pixel=px, snr=0.1)
    imgs = stack.numpy()
    g, o = H.Reference(vol, n / 2, pad=pad), O.Reference(vol, n / 2, pad=pad)
    c = cfg_for(n, px, angular_step=20.0)
    got, gathers, reused = both(monkeypatch, g, c, imgs, rows)
    assert 0 < reused < gathers
    want, _ = O.refine_batch(o, c, imgs, rows)
    close_to_oracle(want, got, px)
    assert np.abs(want[:, 14] - got[:, 14]).max() < 0.02


def test_arithmetic_addresses(d64, O, monkeypatch):
    """PPM_LOCAL_TABLES=0: the fetch that computes its offsets per gather reuses by the same rule"""
    vol, imgs, rows, g, o = d64
    c = cfg_for(64, 2.0)
    got, gathers, reused = both(monkeypatch, g, c, imgs[:M], rows[:M], PPM_LOCAL_TABLES="0")
    assert 0 < reused < gathers
    want, _ = O.refine_batch(o, c, imgs[:M], rows[:M])
    close_to_oracle(want, got, 2.0)


def test_two_chunks_with_the_overlap_on(d64, O, monkeypatch):
    """the final stage of chunk 0 runs on the second stream while chunk 1 is searched; both chunks add to the one pair of counters"""
    vol, imgs, rows, g, o = d64
    c = cfg_for(64, 2.0)
    got, gathers, reused = both(monkeypatch, g, c, imgs, rows, PPM_CHUNK="12")
    assert g.last_overlap() >= 1
    assert 0 < reused < gathers
    one, g1, r1 = both(monkeypatch, g, c, imgs, rows, PPM_CHUNK="24")
    assert g.last_overlap() == 0 and np.array_equal(one, got) and (g1, r1) == (gathers, reused)
    want, _ = O.refine_batch(o, c, imgs, rows)
    close_to_oracle(want, got, 2.0)
