#!/usr/bin/env python3
"""Generate tests/golden/extract_windows.npz by RUNNING the reference's own extraction loop
(src/pyp/extract/core.py:360-511, extract_particles_non_mpi) one coordinate at a time, without normalisation and without the
empty-frame fix: the raw windows it writes, or the fact that it raised.

Run in the build container only, like gen_golden.py (same stub modules; the call that asks IMOD's `header` program for the
image mode is answered with 2 = float32, which is what the input is).  Nothing of the reference's source is copied: the fixture
holds the input image, the coordinates and the windows the reference wrote.

    python tests/golden/gen_extract_golden.py
"""
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

ROWS, COLS, BOX = 40, 50, 16


def records():
    """(name, box, R0, C0): the window's first row / column; the coordinate is the corner plus box // 2."""
    rin, cin = 12, 17
    rec = [("inside", BOX, rin, cin), ("near_1", BOX, -1, -1), ("one_row_near", BOX, -(BOX - 1), cin), ("one_row_far", BOX, ROWS - 2, cin),
           ("one_column_near", BOX, rin, -(BOX - 1)), ("one_column_far", BOX, rin, COLS - 2), ("one_pixel", BOX, -(BOX - 1), -(BOX - 1)),
           ("one_row_two_columns", BOX, -(BOX - 1), -(BOX - 2)), ("far_noclip", BOX, ROWS - 1 - BOX, COLS - 1 - BOX), ("far_touch", BOX, ROWS - BOX, COLS - BOX),
           ("far_1", BOX, ROWS + 1 - BOX, cin), ("last", BOX, ROWS - 1, cin), ("out_far", BOX, rin, COLS + 3), ("out_near", BOX, -BOX, cin),
           ("near_gap", BOX, -BOX - 5, cin), ("out_near_far", BOX, rin, -BOX - COLS - 3), ("both_ends", 64, -10, -6), ("exact_fit", 64, ROWS - 64, COLS - 64)]
    return rec


def main():
    warnings.simplefilter("ignore")
    sys.dont_write_bytecode = True
    tmp = tempfile.mkdtemp(prefix="pypstub_")
    gen_golden._stubs(tmp)
    sys.path[:0] = [tmp, gen_golden.REF]
    os.environ.setdefault("PYP_SCRATCH", tmp)
    from pyp.extract import core as xc
    from pyp.inout.image import mrc as rmrc
    xc.get_image_mode = lambda path: 2
    img = np.random.default_rng(20264).normal(10.0, 3.0, (ROWS, COLS)).astype(np.float32)
    out = dict(image=img)
    names, boxes, coords, raised = [], [], [], []
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for i, (name, box, r0, c0) in enumerate(records()):
            bx, by = float(c0 + box // 2), float(r0 + box // 2)
            rmrc.write(img, "in.mrc")                       # the reference removes its input
            try:
                xc.extract_particles_non_mpi("in.mrc", "out.mrc", [[bx, by]], 5.0, box, 1, 1, 1.0, normalize=False, fixemptyframes=False)
                w, r = np.asarray(rmrc.read("out.mrc")), 0
            except ValueError:
                w, r = np.zeros((box, box), dtype=np.float32), 1
            names.append(name); boxes.append(box); coords.append([bx, by]); raised.append(r)
            out["win%d" % i] = w
    finally:
        os.chdir(cwd)
    out.update(names=np.array(names), boxes=np.array(boxes), coords=np.array(coords), raised=np.array(raised))
    np.savez_compressed(os.path.join(HERE, "extract_windows.npz"), **out)
    print("extract_windows.npz:", {n: ("raised" if r else str(out["win%d" % i].dtype)) for i, (n, r) in enumerate(zip(names, raised))})


if __name__ == "__main__":
    main()
