"""Cases of the folded row order of k_global (pyp_amd/csrc/ppm_rows.h), shared by tests/test_gpu_global_fold.py and
tests/test_global_fold_margins_cpu.py: the smallest shapes at which the fold can go wrong.  Bands beyond 32 pixels search on the
Ns = 128 grid, whose quads pair t with 64 - t:
    box  72, band 34 (Bs = 33)   exactly one quad (31 <-> 33) and 32 plain pairs
    box  96, band 48 (Bs = 47)   half folded
    box 128, band 64 (Bs = 63)   fully folded, the row plan of the benchmark's headline
    box 128, band 33 (Bs = 32)   no quad: the paired order
Five particles (k_global takes two per block: a short last block), seeded synth data."""
import functools

from pyp_amd import synth
from pyp_amd.abi import RefineCfg

PX = 2.0
N_PART = 5
NS = 128

# id: (box, band, angular step, window half-width in search-grid steps, PPM_GLOBAL_PATH)
CASES = {
    "one-quad": (72, 34, 30.0, 3, None),
    "half-folded": (96, 48, 30.0, 3, None),
    "fully-folded": (128, 64, 30.0, 3, None),
    "no-quad": (128, 33, 30.0, 3, None),
    "half-folded-R1": (96, 48, 30.0, 1, None),
    "fully-folded-R6": (128, 64, 30.0, 6, None),
    "one-quad-odd-psi": (72, 34, 24.0, 3, None),              # 15 in-plane angles: every one stored, no psi / psi + 180 pairing
    "fully-folded-tiles": (128, 64, 30.0, 10, "tiles"),       # a window wider than the kernel's: tiles of R = 6
}


@functools.lru_cache(maxsize=None)
def dataset(box):
    # box 128 with the default pose seed has a particle whose true shift lies half-way between two points of the search grid (the best
    # two shifts 1.4e-6 apart in cc, tests/test_global_fold_margins_cpu.py): other poses there
    vol, stack, rows = synth.make_dataset(box, N_PART, pixel=PX, snr=0.1, seed_poses=synth.SEED_POSES + (1 if box == 128 else 0))
    return vol, stack.numpy(), rows


def grid_step_px(box):
    return box / NS


def cfg_for(box, band, astep, R):
    """Search band of band - 0.5 Fourier pixels (Bs = band - 1 whatever the rounding of the division), full band to Nyquist, a window
    of +-R search-grid steps; the hits stay on the grid (iters_hit = -1, no local stage)."""
    rng = (R - 0.5) * grid_step_px(box) * PX
    return RefineCfg.make(box=box, pixel_size=PX, mask_radius=0.4 * box * PX, res_high=2.0 * PX, res_search=PX * box / (band - 0.5),
                          angular_step=astep, search_range_x=rng, search_range_y=rng, res_signed_cc=30.0, local_refine=0, iters_hit=-1)
