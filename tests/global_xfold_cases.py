"""Cases of k_global's folded kx sum (columns kx and kx + 32, pyp_amd/csrc/ppm_window.h), shared by tests/test_gpu_global_xfold.py and
tests/test_global_xfold_margins_cpu.py.  The fold pairs the window rows (0, 1), (2, 3), (4, 5), (6, -) in the halves of the wave and
gives every lane one (row, column) of the window, so the cases ask for every row and every column as the winner:
    box 128 (a search-grid step is one pixel), bands 64 and 33, R = 3: 49 copies of ONE seeded particle without a shift of its own,
    rolled by (sx, sy) whole pixels, sx, sy = -3 .. 3 — an odd particle count, and the last block of k_global is short;
    boxes 72 and 96 at R = 1 and 2 (6 and 15 values per lane instead of 28): the five particles of tests/global_fold_cases.py;
    box 128, band 64 with a window of +-3 by +-2 steps (RSx != RSy): the rolled copies with |sy| <= 2."""
import functools

import numpy as np

import global_fold_cases as G
from pyp_amd import synth
from pyp_amd.formats import cistem
from pyp_amd.abi import RefineCfg

BOX = 128
R_MAX = 3
# pose seed of the rolled particle: tests/test_global_xfold_margins_cpu.py shows that with it the best two shifts and the best two
# orientations of every copy are more than 1e-5 apart in cc
SEED_ROLLED = synth.SEED_POSES + 3
GRID_POSE = (60.0, 60.0, 36.0)       # (psi, theta, phi): direction 60 deg / 36 deg has 10 points on its ring of the 30 deg grid

# id: (box, band, angular step, (RSx, RSy), data set)
CASES = {
    "rolled-band64": (128, 64, 30.0, (3, 3), "rolled"),
    "rolled-band33": (128, 33, 30.0, (3, 3), "rolled"),
    "rolled-3x2": (128, 64, 30.0, (3, 2), "rolled-2"),
    "box72-R1": (72, 34, 30.0, (1, 1), "five"),
    "box72-R2": (72, 34, 30.0, (2, 2), "five"),
    "box96-R1": (96, 48, 30.0, (1, 1), "five"),
    "box96-R2": (96, 48, 30.0, (2, 2), "five"),
}


def rolls(max_sy=R_MAX):
    return [(sx, sy) for sy in range(-max_sy, max_sy + 1) for sx in range(-R_MAX, R_MAX + 1)]


@functools.lru_cache(maxsize=None)
def rolled(max_sy=R_MAX):
    """(vol, imgs, rows, rolls): one seeded particle of box 128 — CTF and noise from the seeds, no shift of its own, its orientation set
    on a point of the 30 deg grid so that the correlation peak is the roll and nothing else — rolled by whole pixels; left unchanged"""
    vol, _, rows = synth.make_dataset(BOX, 1, pixel=G.PX, snr=0.1, seed_poses=SEED_ROLLED, shift_sigma=0.0)
    C = cistem.COL
    rows[0, C["PSI"]], rows[0, C["THETA"]], rows[0, C["PHI"]] = GRID_POSE
    img = synth.render_rows(vol, rows, pixel=G.PX, snr=0.1).numpy()[0]
    rl = rolls(max_sy)
    imgs = np.stack([np.roll(img, (sy, sx), axis=(0, 1)) for sx, sy in rl])
    imgs.setflags(write=False)
    rows = np.repeat(rows, len(rl), axis=0)
    rows.setflags(write=False)
    return vol, imgs, rows, rl


def data_for(case):
    """(vol, imgs, rows) of a case"""
    box, _, _, _, what = CASES[case]
    if what == "five":
        return G.dataset(box)
    return rolled(R_MAX if what == "rolled" else 2)[:3]


def cfg_for(case):
    """as global_fold_cases.cfg_for, with a window of +-RSx by +-RSy search-grid steps; the hits stay on the grid"""
    box, band, astep, (rx, ry), _ = CASES[case]
    step = G.grid_step_px(box) * G.PX
    return RefineCfg.make(box=box, pixel_size=G.PX, mask_radius=0.4 * box * G.PX, res_high=2.0 * G.PX, res_search=G.PX * box / (band - 0.5),
                          angular_step=astep, search_range_x=(rx - 0.5) * step, search_range_y=(ry - 0.5) * step, res_signed_cc=30.0,
                          local_refine=0, iters_hit=-1)
