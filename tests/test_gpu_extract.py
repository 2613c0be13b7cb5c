"""ppm_extract_boxes / k_extract against the float64 model of tests/f64_extract.py, case by case: every edge, box,
radius, flag and emptiness case of the table, the layouts, the refusals, and `bin/csp` modes -2 / -2.1 from a frame list with
non-zero FSHIFT.  Tolerances are the model's own (f64_extract.model_box); one CASE line per case with the worst error and its
ratio to the bound."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import f64_extract as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def _extract(c, img, coords, out=None):
    from pyp_amd import host
    return host.extract_boxes(img, np.asarray(coords), c.box, radius_A=c.radius_px * c.cbin, pixel_size=1.0, coordinate_binning=c.cbin,
                              normalize=c.normalize, fix_empty=c.fix_empty, out=out)


def _worst(c, got, boxes):
    """(worst error / bound, report) over the boxes of a call; an exact bound (0) is met by equality only."""
    worst, rep = 0.0, None
    for i, b in enumerate(boxes):
        err, tol = X.compare(got[i], b, c.normalize)
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        if rep is None or ratio > worst:
            worst, rep = max(worst, ratio), dict(box_index=i, klass=b.klass, noisy=b.noisy, err=err, tol=tol)
    return worst, rep


@pytest.mark.parametrize("name", [c.name for c in X.CASES])
def test_case_matches_the_model(name):
    import torch
    c = X.BY_NAME[name]
    img, boxes, coords = X.image(c.image), X.model(name), list(c.coords)
    got = _extract(c, img, coords)
    assert got.shape == (len(coords), c.box, c.box) and got.dtype == np.float32
    if c.layout == "offset":                               # a device image that starts one float past a 16-byte boundary
        buf = torch.empty(img.size + 8, dtype=torch.float32, device="cuda")
        off = ((4 - buf.data_ptr()) % 16) // 4
        dimg = buf[off:off + img.size].view(img.shape)
        dimg.copy_(torch.from_numpy(np.array(img)))
        assert dimg.data_ptr() % 16 == 4 and dimg.is_contiguous()
        out = torch.full((len(coords), c.box, c.box), 123.0, dtype=torch.float32, device="cuda")
        assert _extract(c, dimg, coords, out=out) is out
        assert np.array_equal(out.cpu().numpy(), got)
    elif c.layout == "out":                                # device image in, the caller's device stack out: the host path's bits
        out = torch.full((len(coords) + 1, c.box, c.box), 123.0, dtype=torch.float32, device="cuda")
        _extract(c, torch.from_numpy(np.array(img)).cuda(), coords, out=out[:len(coords)])
        assert np.array_equal(out[:len(coords)].cpu().numpy(), got) and bool((out[len(coords)] == 123.0).all())
    elif c.layout == "perm":                               # boxes do not depend on their place in the call, the noise does
        perm = list(X.PERMUTATION)
        got_p = _extract(c, img, [coords[j] for j in perm])
        moved = 0
        for k, j in enumerate(perm):
            if boxes[j].noisy:
                b = X.model_box(img, coords[j][0], coords[j][1], c.box, c.cbin, c.radius_px, c.normalize, c.fix_empty, k)
                err, tol = X.compare(got_p[k], b, c.normalize)
                assert err <= tol, (name, j, k, err, tol)
                moved += k != j and not np.array_equal(got_p[k], got[j])
            else:
                assert np.array_equal(got_p[k], got[j]), (name, j, k)
        assert moved > 0
    worst, rep = _worst(c, got, boxes)
    print("CASE", json.dumps(dict(case=name, box=c.box, m=len(coords), worst_ratio=worst, **rep)))
    assert worst <= 1.0, (name, rep)


def _call(L, img, coords, box, cbin, radius_px, out):
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    return L.ppm_extract_boxes(img.ctypes.data_as(C.c_void_p), 0, img.shape[0], img.shape[1], coords.ctypes.data_as(C.c_void_p), len(coords), box,
                               float(cbin), float(radius_px), 1, 1, out.ctypes.data_as(C.c_void_p), 0)


def test_refusals_name_the_offender_and_leave_the_library_usable():
    """Decided on the host before anything is enqueued: the output is untouched, and the next call is right."""
    from pyp_amd import lib
    lib.init(0)
    L = lib.load()
    c = X.BY_NAME["single_b64_inside"]
    img, box, good = np.array(X.image("base")), 64, list(c.coords[0])
    limit = 2147483647.0 - 2.0 * box
    bad = [("nan x", 3, 0, float("nan"), 1.0), ("inf y", 0, 1, float("inf"), 1.0), ("-inf x", 4, 0, float("-inf"), 1.0),
           ("too large", 2, 1, 3.0e9, 1.0), ("too small", 1, 0, -3.0e9, 1.0), ("too large once binned", 4, 0, 1.2e9, 0.5),
           ("past the last value with room for the box", 2, 0, limit + 1.0, 1.0), ("huge", 0, 1, 1e300, 1.0)]
    for what, idx, axis, value, cbin in bad:
        coords = np.array([good] * 5) * cbin
        coords[idx, axis] = value
        out = np.full((5, box, box), 123.0, dtype=np.float32)
        rc, msg = _call(L, img, coords, box, cbin, c.radius_px, out), lib.last_error()
        assert rc == -22 and "ERROR" in msg and ("coordinate %d (%s)" % (idx, "xy"[axis])) in msg, (what, rc, msg)
        assert (out == 123.0).all(), what
    for what, radius in (("nan", float("nan")), ("negative", -1.0), ("-inf", float("-inf"))):
        out = np.full((1, box, box), 123.0, dtype=np.float32)
        rc, msg = _call(L, img, [good], box, 1.0, radius, out), lib.last_error()
        assert rc == -22 and "radius_px" in msg and (out == 123.0).all(), (what, rc, msg)
    out = np.full((1, box, box), 123.0, dtype=np.float32)
    assert _call(L, img, [good], box, 1.0, c.radius_px, out) == 0
    err, tol = X.compare(out[0], X.model(c.name)[0], True)
    assert err <= tol


def test_csp_modes_minus_2_and_minus_2_1_from_a_frame_list_with_frame_shifts(tmp_path):
    """Three movies of four 96 x 130 frames, two particles on frames 1..3, box 32, one particle over the far column edge, FSHIFT
    fractional with a sign per frame: the stack is the model at ORIGINAL + FSHIFT row for row, and mode -2.1 is the running-average
    formula on that stack."""
    from pyp_amd.formats import cistem, mrc
    K = cistem.COL
    box, px, rad_px = 32, 2.0, 12.3
    rng = np.random.default_rng(31)
    movies = rng.normal(10.0, 3.0, (3, 4, 96, 130)).astype(np.float32)
    (tmp_path / "frealign" / "maps").mkdir(parents=True)
    for t in range(3):
        mrc.write(movies[t], str(tmp_path / "frealign" / f"mv_{t:03d}.mrc"), pixel_size=px)
    (tmp_path / "frames_csp.txt").write_text("\n".join(f"frealign/mv_{t:03d}.mrc" for t in range(3)))
    shift_x, shift_y = {1: 1.37, 2: -2.61, 3: 0.73}, {1: -0.42, 2: 1.9, 3: -3.3}
    rows = []
    for t in range(3):
        for p, (x, y) in enumerate(((60.0, 50.0), (120.0, 40.0))):             # the second: columns 104 .. 135 of 130
            for f in (1, 2, 3):
                r = cistem.default_rows(1, px, 300.0, 2.7, 0.07)[0]
                r[K["PIND"]], r[K["TIND"]], r[K["IMIND"]], r[K["FIND"]] = p, t, t, f
                r[K["ORIGINAL_X_POSITION"]], r[K["ORIGINAL_Y_POSITION"]] = x + 2 * t, y - t
                r[K["FSHIFT_X"]], r[K["FSHIFT_Y"]] = shift_x[f] + 0.11 * t, shift_y[f] - 0.07 * p
                rows.append(r)
    rows = np.array(rows)
    rows[:, K["POSITION_IN_STACK"]] = np.arange(1, len(rows) + 1)
    cistem.write_parameters(str(tmp_path / "frealign/maps/fr_r01_02.cistem"), rows)
    parts, tilts = np.zeros((2, 12)), np.zeros((3, 6))
    parts[:, 0], tilts[:, 0] = np.arange(2), np.arange(3)
    cistem.write_extended(str(tmp_path / "frealign/maps/fr_r01_02_extended.cistem"), parts, tilts)
    (tmp_path / ".pyp_config.toml").write_text(
        f'data_set = "fr"\nscope_pixel = {px}\ndata_bin = 1\nextract_bin = 1\nextract_box = {box}\nparticle_rad = {rad_px * px}\nparticle_mw = 300\n'
        'refine_iter = 2\nrefine_rlref = 0.0\nrefine_rhref = "8.0"\nrefine_fboost = false\nreconstruct_norm = true\nrefine_invert = false\n')
    for mode, stack in (("-2", "frealign/fr_stack.mrc"), ("-2.1", "frealign/fr_avg_stack.mrc")):
        r = subprocess.run(f"{BIN}/csp frealign/maps/fr_r01_02.cistem frealign/maps/fr_r01_02_extended.cistem {mode} 0 1 1 frames_csp.txt {stack}",
                           shell=True, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stdout and "CSP: Normal termination" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    back = cistem.read_parameters(str(tmp_path / "frealign/maps/fr_r01_02.cistem"))                 # what the program read: float32 columns
    got = mrc.read(str(tmp_path / "frealign/fr_stack.mrc"))
    assert got.shape == (len(rows), box, box)
    assert np.abs(back[:, K["FSHIFT_X"]]).min() > 0.5 and len({np.sign(s) for s in shift_x.values()}) == 2
    worst, over = 0.0, 0
    for j, r in enumerate(back):
        bx, by = r[K["ORIGINAL_X_POSITION"]] + r[K["FSHIFT_X"]], r[K["ORIGINAL_Y_POSITION"]] + r[K["FSHIFT_Y"]]
        assert bx != round(bx) and by != round(by)
        b = X.model_box(movies[int(r[K["IMIND"]]), int(r[K["FIND"]])], bx, by, box, 1.0, rad_px, True, True, 0)
        assert not b.empty
        over += not b.inside.all()
        err, tol = X.compare(got[j], b, True)
        worst = max(worst, err / tol)
    print("CASE", json.dumps(dict(case="csp_minus_2_frames", box=box, m=len(rows), worst_ratio=worst)))
    assert worst <= 1.0 and over == 9
    avg = mrc.read(str(tmp_path / "frealign/fr_avg_stack.mrc"))
    want = X.running_average_formula(got, back[:, K["PIND"]], back[:, K["IMIND"]], back[:, K["FIND"]], 2, rad_px)
    err = float(np.abs(avg - want).max())
    print("CASE", json.dumps(dict(case="csp_minus_2_1_frames", box=box, m=len(rows), err=err, bound=1e-5)))
    assert avg.shape == got.shape and err < 1e-5
    assert np.abs(avg - got).max() > 0.1                                       # three frames per group: the average is not the frame
