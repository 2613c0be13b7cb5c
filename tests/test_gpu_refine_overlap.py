"""ppm_refine_batch runs the refinement of a chunk's hits on a second stream beside the grid search of the next chunk (two sets of the
per-chunk workspaces, events between the streams; pyp_amd/csrc/ppm_overlap.h holds the rule for when).  It moves work in time and
removes none, so the output rows must equal those of the serial order (PPM_REFINE_OVERLAP=0) in every bit: both parities of the
workspace sets reused, a last chunk of one particle, fewer particle pairs than CUs and more than twice as many, calls the rule keeps
serial, and a second call that meets used workspace sets.  The evaluation counts of a call (last_counts, which the benchmark's roofline
reads) come from its plan, so they do not depend on the order or on the chunking either.  Box 64, the parity suite's synthetic set-up.  Run on the GPU box: pytest -m gpu"""
import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import RefineCfg

pytestmark = pytest.mark.gpu

N, PX, M = 64, 2.0, 25


def cfg_for(**kw):
    # search band 10 Fourier pixels on a 32-point grid of 2-pixel steps; +-6 pixels = 3 steps: k_global keeps the window in registers
    base = dict(box=N, pixel_size=PX, mask_radius=0.4 * N * PX, res_high=PX * N / (0.375 * N), res_search=PX * N / (0.16 * N),
                search_range_x=6 * PX, search_range_y=6 * PX, res_signed_cc=30.0)
    base.update(kw)
    return RefineCfg.make(**base)


@pytest.fixture(scope="module")
def dataset():
    return synth.make_dataset(N, M, pixel=PX, snr=0.1)


@pytest.fixture(scope="module")
def data(dataset):
    from pyp_amd import host
    vol, stack, rows = dataset
    return stack.numpy(), rows, host.Reference(vol, N / 2)


def run(monkeypatch, ref, cfg, imgs, rows, chunk, overlap):
    monkeypatch.setenv("PPM_CHUNK", str(chunk))
    if overlap:
        monkeypatch.delenv("PPM_REFINE_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("PPM_REFINE_OVERLAP", "0")
    out = ref.refine(cfg, imgs, rows)
    return out, ref.last_overlap()


# (particles, PPM_CHUNK): 2, 3 and 4 chunks; 12 + 12 + 1 and 8 + 8 + 8 + 1: a last chunk of one particle (an odd pair)
@pytest.mark.parametrize("n,chunk", [(24, 12), (24, 8), (24, 6), (25, 12), (25, 8)])
def test_rows_equal_the_serial_order(data, monkeypatch, n, chunk):
    imgs, rows, ref = data
    cfg = cfg_for()
    want, off = run(monkeypatch, ref, cfg, imgs[:n], rows[:n], chunk, False)
    counts_serial = ref.last_counts()
    got, on = run(monkeypatch, ref, cfg, imgs[:n], rows[:n], chunk, True)
    counts_overlapped = ref.last_counts()
    assert off == 0 and on >= 1                                    # the second call did overlap
    assert np.array_equal(want, got)
    one, _ = run(monkeypatch, ref, cfg, imgs[:n], rows[:n], n, True)          # one chunk: serial by the rule, and chunking changes nothing
    assert ref.last_overlap() == 0 and np.array_equal(want, one)
    print("last_counts: serial", counts_serial, "overlapped", counts_overlapped, "one chunk", ref.last_counts())
    assert counts_serial == counts_overlapped == ref.last_counts()             # the counts are the plan's, not the last chunk's


def test_more_particle_pairs_than_twice_the_cus(data, monkeypatch):
    """k_global's resident grid: a block walks several particle pairs here (more than two per CU); the other cases of this file, 13 pairs
    at the most, leave most CUs without a block.  The 25 images are repeated to make up the count."""
    import torch
    imgs, rows, ref = data
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = 2 * (2 * cus + 3)                                        # pairs per chunk: 2 CUs + 3
    n = 2 * per + 1                                                # two such chunks and a last one of one particle
    idx = np.arange(n) % M
    big_i, big_r = np.ascontiguousarray(imgs[idx]), np.ascontiguousarray(rows[idx])
    cfg = cfg_for()
    want, _ = run(monkeypatch, ref, cfg, big_i, big_r, per, False)
    got, on = run(monkeypatch, ref, cfg, big_i, big_r, per, True)
    assert on >= 1 and np.array_equal(want, got)


@pytest.mark.parametrize("path,kw", [("tiles", dict(search_range_x=16 * PX, search_range_y=16 * PX)), (None, dict(search_range_x=0.0, search_range_y=0.0)),
                                     (None, dict(global_search=0))])
def test_calls_the_rule_keeps_serial(data, monkeypatch, path, kw):
    """tiles of a wide window, the full-window transform (search range 0 = the mask radius) and a call without a grid search"""
    imgs, rows, ref = data
    if path:
        monkeypatch.setenv("PPM_GLOBAL_PATH", path)
    cfg = cfg_for(**kw)
    want, off = run(monkeypatch, ref, cfg, imgs[:12], rows[:12], 12, False)
    counts_one = ref.last_counts()
    got, on = run(monkeypatch, ref, cfg, imgs[:12], rows[:12], 5, True)       # three chunks, and still one stream
    assert off == 0 and on == 0 and np.array_equal(want, got)
    print("last_counts: one chunk", counts_one, "three chunks", ref.last_counts())
    assert counts_one == ref.last_counts()


def test_second_call_meets_used_workspace_sets(data, monkeypatch):
    imgs, rows, ref = data
    cfg = cfg_for()
    a, on_a = run(monkeypatch, ref, cfg, imgs[:24], rows[:24], 8, True)
    b, on_b = run(monkeypatch, ref, cfg, imgs[3:20], rows[3:20], 8, True)     # 8 + 8 + 1
    assert on_a >= 1 and on_b >= 1
    want_b, _ = run(monkeypatch, ref, cfg, imgs[3:20], rows[3:20], 8, False)
    want_a, _ = run(monkeypatch, ref, cfg, imgs[:24], rows[:24], 8, False)
    assert np.array_equal(a, want_a) and np.array_equal(b, want_b)


def test_handle_teardown_after_both_lanes(dataset, data, monkeypatch):
    """A second handle that has allocated both workspace sets (an overlapped call) and run a call without a grid search is closed: its
    buffers go with it, and the first handle computes what it computed before."""
    from pyp_amd import host
    imgs, rows, ref = data
    cfg = cfg_for()
    want, _ = run(monkeypatch, ref, cfg, imgs[:24], rows[:24], 8, False)
    other = host.Reference(dataset[0], N / 2)
    _, on = run(monkeypatch, other, cfg, imgs[:24], rows[:24], 8, True)
    assert on >= 1
    run(monkeypatch, other, cfg_for(global_search=0), imgs[:24], rows[:24], 8, True)
    other.close()
    again, _ = run(monkeypatch, ref, cfg, imgs[:24], rows[:24], 8, False)
    assert np.array_equal(want, again)
