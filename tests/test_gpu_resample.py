"""ppm_resample / ppm_resize / ppm_fit_volume, the executables and pipeline.iteration(reference_pixel=) on the GPU against the float64
restatement tests/f64_resample.py (which tests/test_resample_cpu.py holds to mathematics).

Resampled values are held to  f64_ref.MAP_K x EPS32 x d (log2 N + log2 M) x max|x|  (f64_resample.bound_resample: one float32 rounding per
butterfly stage along a path, d axes, a forward and an inverse transform each; MAP_K = 8 is the constant of the box sweep).  The error
measured, as a multiple of that floor, is printed per case as a `CASE` JSON line (CHANGELOG.md records it: 0.06 .. 0.13).  Copied voxels
of a resize are equal bit for bit; pad values are within 4 EPS32 of the model's, which accumulates in double like the kernel.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 - before libpypmatch.so is loaded: the two must end up on one HIP runtime

import f64_ref as R
import f64_resample as FR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = {c["case"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "resample_scripts.json")))["scripts"]}
PAIRS = [(32, 64), (64, 32), (48, 36), (50, 40), (56, 42), (96, 70), (64, 64)]
EPS32 = R.EPS32


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


@functools.lru_cache(maxsize=None)
def stack_case(items, n, m):
    x = FR.make_items((items, n, n))
    want = FR.resample(x, m, dims=2)
    x.setflags(write=False); want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def volume_case(n, m):
    x = FR.make_items((n, n, n))
    want = FR.resample(x, m)
    x.setflags(write=False); want.setflags(write=False)
    return x, want


def held(tag, got, want, n, m, d, x):
    err = float(np.abs(got.astype(np.float64) - want).max())
    floor = FR.floor_model_resample(n, m, d) * float(np.abs(x).max())
    print("CASE", json.dumps(dict(case=tag, n=n, m=m, dims=d, err=err, err_over_floor=err / floor)))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert err <= FR.bound_resample(n, m, d, x), (tag, err, FR.bound_resample(n, m, d, x))


# ------------------------------------------------------------------------------------------ 1: lines and axes
@pytest.mark.parametrize("items", [1, 3, 17])
@pytest.mark.parametrize("n, m", PAIRS)
def test_stacks(H, n, m, items):
    x, want = stack_case(items, n, m)
    held("stack x%d" % items, H.resample(x, m), want, n, m, 2, x)


@pytest.mark.parametrize("n, m", PAIRS)
def test_volumes(H, n, m):
    x, want = volume_case(n, m)
    held("volume", H.resample(x, m, volume=True), want, n, m, 3, x)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n, m", [p for p in PAIRS if p[0] != p[1]])
def test_nyquist_patterns(H, n, m, d):
    """Against the analytic values: a wrong Nyquist rule is of the order of the amplitude, not of the bound."""
    src, want = FR.nyquist(n, m, d)
    x = src.astype(np.float32)
    got = H.resample(x, m, volume=d == 3)
    # the float32 rounding of the input travels through the (linear, norm-preserving) rule: one more EPS32 of max|x| on top of the bound
    assert np.abs(got - want).max() <= FR.bound_resample(n, m, d, x) + EPS32 * np.abs(x).max()
    assert np.abs(want).max() > 0.05


# ------------------------------------------------------------------------------------------ 2: at size
@pytest.mark.parametrize("items, n, m", [(3, 256, 128), (2, 512, 256), (2, 384, 512)])
def test_large_images(H, items, n, m):
    x, want = stack_case(items, n, m)
    held("stack x%d" % items, H.resample(x, m), want, n, m, 2, x)


def test_large_volume(H):
    x, want = volume_case(128, 96)
    held("volume", H.resample(x, 96, volume=True), want, 128, 96, 3, x)


# ------------------------------------------------------------------------------------------ 3: resize
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape, b, volume", [((33, 33, 33), 48, True), ((48, 48, 48), 20, True), ((5, 40, 40), 64, False)])
def test_resize(H, shape, b, volume, normalize):
    x = FR.make_items(shape)
    want, wpad = FR.resize(x, b, normalize=normalize, volume=volume)
    got, pads = H.resize(x, b, normalize=normalize, volume=volume, pad_values=True)
    again, pads2 = H.resize(x, b, normalize=normalize, volume=volume, pad_values=True)
    assert got.tobytes() == again.tobytes() and pads.tobytes() == pads2.tobytes()                 # fixed-order sums: bit-reproducible
    print("CASE", json.dumps(dict(case="resize", shape=shape, b=b, normalize=normalize, pad_err=float(np.abs(pads - wpad).max()),
                                  err=float(np.abs(got - want).max()))))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.abs(pads.astype(np.float64) - wpad).max() <= 4 * EPS32
    n = shape[-1]
    d = 3 if volume else 2
    k = min(n, b)
    lo_o, lo_i = b // 2 - k // 2 if b > n else 0, n // 2 - k // 2 if n > b else 0
    # which output voxels are copies: i - b // 2 + n // 2 inside the input
    idx = np.arange(b) - b // 2 + n // 2
    inside = (idx >= 0) & (idx < n)
    assert inside.sum() == k and idx[inside][0] == lo_i and np.flatnonzero(inside)[0] == lo_o
    sl_o = (Ellipsis,) + (slice(lo_o, lo_o + k),) * d
    sl_i = (Ellipsis,) + (slice(lo_i, lo_i + k),) * d
    if not normalize:
        assert np.array_equal(got[sl_o], x[sl_i])                                                 # copied voxels: bit for bit
    else:
        # (x - mean) / sd formed in double and rounded once, against the model's double: half a float32 ulp, plus what separates the two means
        assert np.abs(got[sl_o] - want[sl_o]).max() <= EPS32 * np.abs(want).max()
    mask = np.ones(got.shape, dtype=bool)
    mask[sl_o] = False
    per_item = pads if not volume else pads[:1]
    if mask.any():
        full = np.broadcast_to(per_item.reshape((-1,) + (1,) * d) if not volume else per_item.reshape((1,) * d), got.shape)
        assert np.array_equal(got[mask], full[mask])                                              # everything else is the pad value as reported


def test_resize_refuses_a_flat_item_and_leaves_out_alone(H):
    from pyp_amd import lib
    x = FR.make_items((3, 40, 40)).copy()
    x[1] = 2.5
    out = np.full((3, 64, 64), 7.0, dtype=np.float32)
    with pytest.raises(lib.PpmError, match="ERROR.*image 1 .*standard deviation"):
        H.resize(x, 64, normalize=True, out=out)
    assert (out == 7.0).all()
    assert H.resize(x, 64, out=out) is out and not (out == 7.0).all()                             # without normalisation a flat image is fine


# ------------------------------------------------------------------------------------------ 4: device tensors, refusals
def test_device_tensors(H):
    from pyp_amd import lib
    x, want = stack_case(3, 48, 36)
    tx = torch.from_numpy(x.copy()).cuda()
    t = H.resample(tx, 36)
    assert t.is_cuda and t.shape == (3, 36, 36) and np.array_equal(tx.cpu().numpy(), x)           # input untouched
    assert np.array_equal(t.cpu().numpy(), H.resample(x, 36))                                     # the same numbers as from the host
    to = torch.full((3, 36, 36), 7.0, device="cuda")
    assert H.resample(tx, 36, out=to) is to and np.array_equal(to.cpu().numpy(), t.cpu().numpy())
    v, wv = volume_case(48, 36)
    tv = torch.from_numpy(v.copy()).cuda()
    assert np.array_equal(H.resample(tv, 36, volume=True).cpu().numpy(), H.resample(v, 36, volume=True))
    r, pads = H.resize(tv, 20, volume=True, pad_values=True)
    assert r.is_cuda and np.array_equal(r.cpu().numpy(), H.resize(v, 20, volume=True)) and np.array_equal(tv.cpu().numpy(), v)
    # refusals leave dst as it was
    bad = torch.full((3, 34, 34), 7.0, device="cuda")
    with pytest.raises(lib.PpmError, match="ERROR.*34.*32 and 36"):
        H.resample(tx, 34, out=bad)
    assert bool((bad == 7.0).all())
    hb = np.full((3, 34, 34), 7.0, dtype=np.float32)
    with pytest.raises(lib.PpmError, match="nearest to 34"):
        H.resample(x, 34, out=hb)
    assert (hb == 7.0).all()
    with pytest.raises(lib.PpmError, match="ERROR"):
        H.resample(np.zeros((2, 34, 34), np.float32), 32)
    with pytest.raises(lib.PpmError, match="8..512"):
        H.resize(x, 600)
    with pytest.raises(ValueError, match="ERROR"):
        H.resample(np.zeros((2, 32, 48), np.float32), 64)
    with pytest.raises(ValueError, match="ERROR"):
        H.resample(tx, 36, out=np.zeros((3, 36, 36), np.float32))
    # an unaligned device pointer takes the 4-byte accesses and gives the same numbers
    big = torch.zeros(3 * 48 * 48 + 1, device="cuda")
    off = big[1:].view(3, 48, 48)
    off.copy_(tx)
    assert np.array_equal(H.resample(off, 36).cpu().numpy(), t.cpu().numpy())


# ------------------------------------------------------------------------------------------ 5: fit_reference
@pytest.mark.parametrize("n, a_in, a_out, box", [(100, 1.06, 2.1, 64), (64, 2.0, 1.35, 96)])
def test_fit_reference(H, n, a_in, a_out, box, tmp_path):
    from pyp_amd.formats import mrc
    v = FR.make_items((n, n, n))
    want, wi = FR.fit(v, a_in, a_out, box)
    got, info = H.fit_reference(v, a_in, a_out, box)
    plan = H.fit_plan(n, a_in, a_out, box)
    for k in ("n_in", "box_out", "n_c", "P", "M", "scale", "pixel_achieved", "rel_error"):
        assert getattr(info, k) == getattr(plan, k), k
    assert (info.n_c, info.P, info.M, info.pixel_achieved, info.rel_error) == (wi["n_c"], wi["P"], wi["M"], wi["pixel_achieved"], wi["rel_error"])
    assert abs(info.pad_value_1 - wi["pad_value_1"]) <= 4 * EPS32
    # the stages' bounds: the resample stage on the padded map; the second pad value is a mean of resampled voxels
    b = FR.bound_resample(info.P, info.M, 3, v) + 4 * EPS32
    err = float(np.abs(got - want).max())
    print("CASE", json.dumps(dict(case="fit", n=n, box=box, P=info.P, M=info.M, pixel=info.pixel_achieved, err=err, bound=b)))
    assert err <= b and abs(info.pad_value_2 - wi["pad_value_2"]) <= b
    mrc.write(v, str(tmp_path / "ref.mrc"), pixel_size=a_in)
    r = subprocess.run([os.path.join(ROOT, "bin", "fit_reference"), str(tmp_path / "ref.mrc"), str(tmp_path / "fit.mrc"), "--pixel", repr(a_out), "--box", str(box)],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, PPM_LOCK_DIR=str(tmp_path)))
    assert r.returncode == 0 and "FitReference: Normal termination" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(mrc.read(str(tmp_path / "fit.mrc")), got)
    assert abs(mrc.read_header(str(tmp_path / "fit.mrc"))["pixel_size"] - info.pixel_achieved) <= 1e-6 * info.pixel_achieved


def test_fit_reference_refuses(H):
    """A 512 input whose whole extent the output box shows has no room to pad: P = 512 only, and s = 0.45 is 2.8 % from the nearest M."""
    from pyp_amd import lib
    assert not FR.fit_plan(512, 1.0, 1.0 / 0.45, 512)["ok"]
    v = np.zeros((512, 512, 512), np.float32)                                                    # never read: the plan refuses first
    out = np.full((512, 512, 512), 7.0, np.float32)
    with pytest.raises(lib.PpmError, match="ERROR: fit: .*the best is 512 -> "):
        H.fit_reference(v, 1.0, 1.0 / 0.45, 512, out=out)
    assert out[::7, ::5, ::3].min() == 7.0 and out[::7, ::5, ::3].max() == 7.0 and out[-1, -1, -1] == 7.0
    with pytest.raises(ValueError, match="ERROR"):
        H.fit_reference(np.zeros((32, 32, 40), np.float32), 1.0, 1.0, 32)


# ------------------------------------------------------------------------------------------ 6: the executables, one after the other
def test_executables_in_sequence(H, tmp_path):
    """PYP's resample_and_resize on a fixture record: bin/resample on the first command (the size answer is the float 36.0), bin/resize on
    the second; then bin/resample_mp.exe on a 6 x 64^2 stack with the recorded downsample_stack script."""
    from pyp_amd.formats import mrc
    env = dict(os.environ, PPM_LOCK_DIR=str(tmp_path))
    case = SCRIPTS["resample_and_resize"]
    work = tmp_path / "project"
    os.makedirs(work)
    vol = FR.make_items((48, 48, 48))
    mrc.write(vol, str(work / "model_48.mrc"), pixel_size=1.5)

    def script(cmd):
        s = cmd.replace("@TMP@", str(tmp_path))
        for prog, ours in (("/opt/pyp/external/cistem2/resample", "resample"), ("/opt/pyp/external/cistem2/resize", "resize"),
                           ("/opt/pyp/external/frealign_v9.11/bin/resample_mp.exe", "resample_mp.exe")):
            s = s.replace(prog + " <<", os.path.join(ROOT, "bin", ours) + " <<")
        return s
    r = subprocess.run(script(case["commands"][0]), shell=True, cwd=work, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Resample: Normal termination" in r.stdout, r.stdout + r.stderr
    mid = mrc.read(str(work / "model_48.mrc~"))
    want_mid = FR.resample(vol, 36)
    assert mid.shape == (36, 36, 36) and np.abs(mid - want_mid).max() <= FR.bound_resample(48, 36, 3, vol)
    assert abs(mrc.read_header(str(work / "model_48.mrc~"))["pixel_size"] - 1.5 * 48 / 36) < 1e-6
    r = subprocess.run(script(case["commands"][1]), shell=True, cwd=work, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Resize: Normal termination" in r.stdout, r.stdout + r.stderr
    out = mrc.read(str(work / "out.mrc"))
    assert np.array_equal(out, H.resize(mid, 32, volume=True)) and np.array_equal(out, mid[2:34, 2:34, 2:34])
    assert abs(mrc.read_header(str(work / "out.mrc"))["pixel_size"] - 2.0) < 1e-6
    st = FR.make_items((6, 64, 64))
    mrc.write(st, str(work / "stack_6x64.mrc"), pixel_size=1.0)
    os.remove(work / "out.mrc")
    r = subprocess.run(script(SCRIPTS["downsample_stack"]["commands"][0]), shell=True, cwd=work, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Resample_mp: Normal termination" in r.stdout, r.stdout + r.stderr
    got = mrc.read(str(work / "out.mrc"))
    assert got.shape == (6, 32, 32) and np.abs(got - FR.resample(st, 32, dims=2)).max() <= FR.bound_resample(64, 32, 2, st)
    assert abs(mrc.read_header(str(work / "out.mrc"))["pixel_size"] - 2.0) < 1e-6
    before = sorted(os.listdir(work))
    bad = script(case["commands"][0]).replace("36.0", "34.0")
    r = subprocess.run(bad.replace("model_48.mrc~", "none.mrc"), shell=True, cwd=work, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "ERROR" in r.stdout and "32 and 36" in r.stdout
    assert sorted(os.listdir(work)) == before


# ------------------------------------------------------------------------------------------ 7: the in-memory iteration
def test_iteration_fits_its_reference(H):
    """pipeline.iteration(reference_pixel=3) with a 48^3 reference for a 32-box data set at 2 A against the explicit fit_reference followed
    by iteration: the same rows."""
    from pyp_amd import pipeline, synth
    from pyp_amd.abi import RefineCfg
    n, px = 32, 2.0
    vol, stack, rows = synth.make_dataset(n, 8, pixel=px, snr=0.5)
    imgs = stack.numpy()
    # the same object in a 48 box at 3 A: padded to 48 voxels of 2 A, resampled to 32 voxels of 3 A, padded to 48
    ref48 = H.resize(H.resample(H.resize(np.asarray(vol, np.float32), 48, volume=True), 32, volume=True), 48, volume=True)
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 12.0, global_search=0, res_signed_cc=30.0)
    kw = dict(pixel_size=px, molecular_mass_kda=50.0)
    a_in = 3.0
    fitted, info = H.fit_reference(ref48, a_in, px, n)
    assert fitted.shape == (n, n, n) and abs(info.pixel_achieved / px - 1.0) <= 0.01
    auto = pipeline.iteration(ref48, imgs, rows, cfg, reference_pixel=a_in, **kw)
    two = pipeline.iteration(fitted, imgs, rows, cfg, **kw)
    assert np.array_equal(auto["rows"], two["rows"])
    assert bytes(auto["fit"]) == bytes(info)
    assert "fit" not in two
