"""The grid search in SECTIONS of the orientation grid (pyp_amd/csrc/ppm_sections.h; DESIGN.md sections 2, 3, 4c): the slice banks of
contiguous ranges of grid directions are built and searched one after another, every section keeps its K best, and the K best of those
lists are the hits.  Sectioning must not change a bit of the result; it must agree with the oracle; and it must run a call whose bank
of the whole grid passes what the transform kernel can address (4 GB).  PPM_BANK_BYTES lowers the banks' byte budget to force
sections on small cases.  Run on the GPU box: pytest -m gpu"""
import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import RefineCfg
from test_grid_sections_plan import grid_counts

pytestmark = pytest.mark.gpu

N, PX, BAND, SEARCH = 64, 2.0, 24.0, 10.24          # search grid of 32 points: Bs = 10, L = 16


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def data():
    vol, stack, rows = synth.make_dataset(N, 10, pixel=PX, snr=0.1)
    return vol, stack.numpy(), rows


@pytest.fixture(scope="module")
def ref(H, data):
    """One handle for the whole module: the banks and tables it caches pass from call to call, sectioned and not."""
    g = H.Reference(data[0], N / 2)
    yield g
    g.close()


def raw_cfg(n, px, band_px, search_px, **kw):
    """Grid search only: the hits stay at their grid points (test hook iters_hit = -1), no local refinement."""
    base = dict(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / band_px, res_search=px * n / search_px,
                search_range_x=0.0, search_range_y=0.0, res_signed_cc=30.0, local_refine=0, iters_hit=-1)
    base.update(kw)
    return RefineCfg.make(**base)


def same_grid_point_and_shift(want, got, px, step):
    assert synth.angular_error_deg(want, got).max() < 1e-4
    assert np.array_equal(np.round(want[:, 4:6] / px / step), np.round(got[:, 4:6] / px / step))
    assert np.abs(want[:, 14] - got[:, 14]).max() < 0.01                 # SCORE is 100 x cc


def direction_bytes(npsi_store, transform):
    """Bytes of one grid direction in the banks of this module's workload: k_global's bank keeps 2 (Bs + 1) = 22 paired rows, rounded up
    to the 8 rows of one trip, of 64 float2 per stored slice; the transform path adds L x L float4."""
    return npsi_store * (24 * 64 * 8 + (16 * 16 * 16 if transform else 0))


def budget_for(n_dir, npsi_store, transform, sections):
    return -(-n_dir // sections) * direction_bytes(npsi_store, transform)


GRIDS = {"A": dict(angular_step=15.0, top_hits=20),       # 24 in-plane angles, 12 stored: psi and psi + 180 from one slice
         "B": dict(angular_step=24.0, top_hits=64)}       # 15 in-plane angles, all stored: one direction holds fewer than K orientations
NARROW = dict(search_range_x=6 * PX, search_range_y=6 * PX)
VARIANTS = {
    "transform": (dict(), {}, True),
    "narrow_window": (NARROW, {}, False),                                        # +-3 steps: k_global, one tile
    "d2": (dict(symmetry="D2"), {}, True),
    "row_chunks": (dict(), {"PPM_GFFT_ROWS": "10"}, True),
    "several_chunks": (dict(), {"PPM_CHUNK": "4"}, True),                        # 3 chunks x S sections: the banks' cache keys
    "several_chunks_narrow": (NARROW, {"PPM_CHUNK": "4"}, False),
    "full_default_call": (dict(local_refine=1, iters_hit=0), {}, True),          # hits refined, the best one continued
}


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_sections_do_not_change_a_bit(ref, data, monkeypatch, grid, variant):
    """The rows of a call in 2, 3 and n_dir sections (one direction each; grid B: a section's in-plane set is shorter than K) equal the
    rows of the same call in one section, bit for bit."""
    _, imgs, rows = data
    kw, env, transform = VARIANTS[variant]
    kw = dict(GRIDS[grid], **kw)
    c = raw_cfg(N, PX, BAND, SEARCH, **kw)
    sym = kw.get("symmetry", "C1")
    n_dir, npsi_store = grid_counts(kw["angular_step"], *((180.0, 90.0) if sym == "D2" else (360.0, 180.0)))
    if grid == "B":
        assert npsi_store < kw["top_hits"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    one = ref.refine(c, imgs, rows)
    assert ref.last_sections() == 1
    assert ref.last_counts()["n_global"] == n_dir * (npsi_store * 2 if grid == "A" else npsi_store)
    for sections in (2, 3, n_dir):
        monkeypatch.setenv("PPM_BANK_BYTES", str(budget_for(n_dir, npsi_store, transform, sections)))
        got = ref.refine(c, imgs, rows)
        assert ref.last_sections() == sections
        assert np.array_equal(one, got), (sections, np.argwhere(one != got)[:8])
    monkeypatch.delenv("PPM_BANK_BYTES")
    again = ref.refine(c, imgs, rows)                     # back to one section on the same handle: the last section's bank is not section 0
    assert ref.last_sections() == 1 and np.array_equal(one, again)


def test_three_sections_match_oracle_mode_0(ref, O, data, monkeypatch):
    """The default grid in three sections against the oracle's zero-filled inverse transform: the same grid orientation and integer
    shift for every particle, and every orientation of the grid counted once."""
    vol, imgs, rows = data
    c = raw_cfg(N, PX, BAND, SEARCH, **GRIDS["A"])
    d = O.band_dims(c)
    assert d["Ns"] == 32
    n_dir, npsi_store = grid_counts(15.0)
    want, counts = O.refine_batch(O.Reference(vol, N / 2), c, imgs, rows, ccf_mode=0)
    monkeypatch.setenv("PPM_BANK_BYTES", str(budget_for(n_dir, npsi_store, True, 3)))
    got = ref.refine(c, imgs, rows)
    assert ref.last_sections() == 3
    assert ref.last_counts()["n_global"] == counts[0]
    same_grid_point_and_shift(want, got, PX, d["step"])


def test_the_note_names_the_sections_only_when_there_are_several(ref, data, monkeypatch):
    _, imgs, rows = data
    c = raw_cfg(N, PX, BAND, SEARCH, **GRIDS["A"])
    n_dir, npsi_store = grid_counts(15.0)
    ref.refine(c, imgs, rows)
    assert ref.last_sections() == 1 and "section" not in ref.note()
    monkeypatch.setenv("PPM_BANK_BYTES", str(budget_for(n_dir, npsi_store, True, 4)))
    ref.refine(c, imgs, rows)
    assert ref.last_sections() == 4 and "grid search in 4 sections of the orientation grid" in ref.note()
    monkeypatch.delenv("PPM_BANK_BYTES")
    ref.refine(RefineCfg.make(box=N, pixel_size=PX, mask_radius=0.4 * N * PX, res_high=PX * N / BAND, global_search=0), imgs, rows)
    assert ref.last_sections() == 0                       # no grid search in that call


def test_a_bank_below_one_direction_is_refused_with_a_message(H, ref, data, monkeypatch):
    _, imgs, rows = data
    monkeypatch.setenv("PPM_BANK_BYTES", "1000")
    with pytest.raises(H.lib.PpmError, match="angular step"):
        ref.refine(raw_cfg(N, PX, BAND, SEARCH), imgs, rows)


def test_a_step_of_4p5_degrees_at_256_runs_in_sections_and_agrees_with_the_tiles(H, monkeypatch):
    """256^2, search band 64 px (L = 64: 64 KB per stored slice in the transform's bank), range 0 = the mask radius, angular step 4.5
    degrees: more than 65 536 stored slices, a bank beyond the 4 GB one buffer descriptor spans — refused with -22 before the search
    ran in sections.  No hook is set: the 4 GB rule alone splits the grid.  The CPU oracle is too slow for 163 k orientations at
    256^2, so this one case is a SELF-COMPARISON of two kernels of the library: k_gfft in sections against the tiled k_global
    (PPM_GLOBAL_PATH=tiles), which keeps the bank of the whole grid (5.3 GB) in one piece and searches it in 25 register tiles."""
    n, px, step = 256, 1.0, 4.5
    n_dir, npsi_store = grid_counts(step)
    assert n_dir * npsi_store > 65536                                       # fails if the grid rule ever moves
    vol, stack, rows = synth.make_dataset(n, 2, pixel=px, snr=0.05)
    imgs = stack.numpy()
    c = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.32 * n * px, res_high=4.0, res_search=4.0, search_range_x=0.0, search_range_y=0.0,
                       res_signed_cc=30.0, angular_step=step, local_refine=0, iters_hit=-1)
    g = H.Reference(vol, n / 2)
    got = g.refine(c, imgs, rows)
    assert g.last_sections() >= 2
    assert g.last_counts()["n_global"] == n_dir * npsi_store * 2
    assert "sections of the orientation grid" in g.note()
    monkeypatch.setenv("PPM_GLOBAL_PATH", "tiles")
    want = g.refine(c, imgs, rows)
    assert g.last_sections() == 1
    g.close()
    same_grid_point_and_shift(want, got, px, 2.0)
