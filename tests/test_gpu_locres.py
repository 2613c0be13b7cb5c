"""ppm_local_resolution / bin/resmap on the GPU against the float64 restatement tests/f64_locres.py.

Integer logic must be equal: the inside count, the levels, 1 + 3 L transforms, the level counts, repeated calls, host arrays against CUDA
tensors.  E_A and E_D of every level (the library's debug output keep_levels) and tau are held, on every voxel, to B x max(E_A over the
inside voxels) with one B per quantity: f64_locres.FACTOR x the largest error measured on an MI355X over the levels of boxes 32, 48 and 70
(f64_locres.MEASURED, CHANGELOG.md).  The resolution map is equal to the reference's on every voxel that is not undecided, i.e. whose E_A
lies farther than 2 B max E_A from tau at every level in float64; tests/test_locres_cpu.py holds those to 2 % of the inside voxels.
"""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 - before libpypmatch.so is loaded: the two must end up on one HIP runtime

import f64_locres as F
from pyp_amd.abi import LocresCfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = F.PIXEL
CASES = [(n, masked) for n in F.GPU_BOXES for masked in (False, True)]


@pytest.fixture(scope="module")
def H():
    from pyp_amd import host
    return host


def cfg_of(n, p=F.GPU_P, keep=True):
    lo, hi, step = F.gpu_level_grid(n)
    return LocresCfg.make(PX, p_value=p, min_res=lo, max_res=hi, step=step, keep_levels=keep)


_gpu = {}


def gpu_case(H, n, masked):
    if (n, masked) not in _gpu:
        h1, h2, m = F.gpu_inputs(n, masked)
        _gpu[(n, masked)] = H.local_resolution(h1, h2, cfg_of(n), mask=m)
    return _gpu[(n, masked)]


def check_against(ref, g, what):
    """Everything a result is held to; prints the measured figures first."""
    ins, L = ref["inside"], len(ref["levels"])
    gi = g["info"]
    rel = dict(E_A=[], E_D=[], tau=[])
    for i in range(L):
        top = float(ref["E_A"][i][ins].max())
        rel["E_A"].append(float(np.abs(g["energies"][i, ..., 0] - ref["E_A"][i]).max()) / top)
        rel["E_D"].append(float(np.abs(g["energies"][i, ..., 1] - ref["E_D"][i]).max()) / top)
        rel["tau"].append(abs(float(g["tau"][i]) - ref["tau"][i]) / top)
    und = F.undecided(ref, F.B_UNDECIDED)
    differ = (np.asarray(g["resolution"]) != ref["resolution"])
    print("FLOOR", json.dumps(dict(what=what, rel=rel, n_inside=[gi.n_inside, ref["n_inside"]], counts=[g["counts"].tolist(), ref["counts"].tolist()],
                                   undecided=int(und.sum()), differ=int(differ.sum()), differ_decided=int((differ & ~und).sum()))))
    assert gi.n_inside == ref["n_inside"] and gi.n_levels == L and gi.transforms == 1 + 3 * L
    assert np.array_equal(g["levels"], ref["levels"]) and g["levels"].dtype == np.float32
    assert max(rel["E_A"]) <= F.B_E_A and max(rel["E_D"]) <= F.B_E_D and max(rel["tau"]) <= F.B_TAU
    assert und.sum() <= F.UNDECIDED_CAP * ref["n_inside"]
    assert not (differ & ~und).any()
    assert np.array_equal(g["counts"], ref["counts"]) and gi.unassigned == ref["unassigned"]
    assert int(g["counts"].sum()) + gi.unassigned == gi.n_inside and gi.median == ref["median"]


# ------------------------------------------------------------------------------------------ 1: energies, thresholds, map, counts
@pytest.mark.parametrize("n,masked", CASES)
def test_against_float64(H, n, masked):
    check_against(F.gpu_case(n, masked), gpu_case(H, n, masked), "box %d%s" % (n, " masked" if masked else ""))


# ------------------------------------------------------------------------------------------ 2: equal bits
@pytest.mark.parametrize("n,masked", CASES)
def test_cuda_tensors_give_the_same_bits(H, n, masked):
    g = gpu_case(H, n, masked)
    dev = [None if v is None else torch.from_numpy(v).cuda() for v in F.gpu_inputs(n, masked)]
    d = H.local_resolution(dev[0], dev[1], cfg_of(n), mask=dev[2])
    assert d["resolution"].is_cuda and d["energies"].is_cuda
    assert np.array_equal(d["resolution"].cpu().numpy(), g["resolution"]) and np.array_equal(d["energies"].cpu().numpy(), g["energies"])
    assert np.array_equal(d["tau"], g["tau"]) and np.array_equal(d["counts"], g["counts"]) and bytes(d["info"]) == bytes(g["info"])


def test_two_calls_agree_and_the_debug_output_changes_nothing(H):
    n = 48
    h1, h2, m = F.gpu_inputs(n, True)
    g = gpu_case(H, n, True)
    again = H.local_resolution(h1, h2, cfg_of(n), mask=m)
    plain = H.local_resolution(h1, h2, cfg_of(n, keep=False), mask=m)
    assert "energies" not in plain
    for r in (again, plain):
        assert np.array_equal(r["resolution"], g["resolution"]) and np.array_equal(r["tau"], g["tau"]) and bytes(r["info"]) == bytes(g["info"])
    assert np.array_equal(again["energies"], g["energies"])


def test_tracing_changes_no_bit(H, monkeypatch, capfd):
    """PPM_TRACE=1 times the stages with pairs of events on the call's stream, summed over three levels: map, energies and info stay what
    they are without it, and stderr gets one line that names every stage."""
    n = 32
    h1, h2, m = F.gpu_inputs(n, True)
    lo, hi, _ = F.gpu_level_grid(n)
    cfg = LocresCfg.make(PX, p_value=F.GPU_P, min_res=lo, max_res=hi, step=(hi - lo) / 2.0, keep_levels=True)
    plain = H.local_resolution(h1, h2, cfg, mask=m)
    capfd.readouterr()
    monkeypatch.setenv("PPM_TRACE", "1")
    traced = H.local_resolution(h1, h2, cfg, mask=m)
    monkeypatch.delenv("PPM_TRACE")
    assert plain["info"].n_levels == 3 and plain["info"].transforms == 10
    assert np.array_equal(traced["resolution"], plain["resolution"]) and np.array_equal(traced["energies"], plain["energies"])
    assert np.array_equal(traced["tau"], plain["tau"]) and np.array_equal(traced["counts"], plain["counts"]) and bytes(traced["info"]) == bytes(plain["info"])
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("ppm_local_resolution:")]
    assert len(lines) == 1, lines
    assert "box 32, 3 levels, 10 transforms" in lines[0] and " ms wall" in lines[0], lines[0]
    for stage in ("init + pack", "forward transform", "band", "band back", "square", "squares forward", "window", "window back",
                  "threshold (2 histogram passes)", "assign"):
        assert f" {stage} " in lines[0], (stage, lines[0])


def test_device_maps_off_a_16_byte_boundary(H):
    n = 32
    g = gpu_case(H, n, True)
    dev = []
    for v in F.gpu_inputs(n, True):
        buf = torch.zeros(n ** 3 + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(v).cuda().reshape(-1)
        dev.append(buf[1:].view(n, n, n))
    assert all(t.data_ptr() % 16 == 4 for t in dev)
    d = H.local_resolution(dev[0], dev[1], cfg_of(n), mask=dev[2])
    assert np.array_equal(d["resolution"].cpu().numpy(), g["resolution"]) and np.array_equal(d["tau"], g["tau"])


# ------------------------------------------------------------------------------------------ 3: the ends of the mask and of the rank
def special(H, n, p, mask, what):
    h1, h2, _ = F.gpu_inputs(n, False)
    lv, _ = F.levels(n, PX, *F.gpu_level_grid(n))
    ref = F.run(h1, h2, PX, p, lv, mask=mask)
    g = H.local_resolution(h1, h2, cfg_of(n, p=p), mask=mask)
    check_against(ref, g, what)
    return ref, g


def test_mask_with_one_voxel(H):
    n = 32
    m = np.zeros((n, n, n), dtype=np.float32)
    m[13, 17, 9] = 1.0
    m[3, 3, 3] = 0.5                              # not above 0.5: outside
    ref, g = special(H, n, F.GPU_P, m, "one voxel")
    assert g["info"].n_inside == 1 and (np.delete(g["resolution"].ravel(), (13 * n + 17) * n + 9) == 100).all()


def test_mask_with_every_voxel(H):
    n = 32
    ref, g = special(H, n, F.GPU_P, np.ones((n, n, n), dtype=np.float32), "every voxel")
    assert g["info"].n_inside == n ** 3


@pytest.mark.parametrize("p,r_of", [(1.0 - 1e-9, lambda n_in: 1), (1e-9, lambda n_in: n_in)])
def test_rank_at_its_ends(H, p, r_of):
    n = 32
    ref, g = special(H, n, p, None, "p = %g" % p)
    assert F.rank(p, ref["n_inside"]) == r_of(ref["n_inside"])
    ed = np.maximum(g["energies"][..., 1][:, ref["inside"]], 0.0)          # tau is the smallest / the largest E_D the GPU itself computed
    assert np.array_equal(g["tau"], ed.min(axis=1) if r_of(2) == 1 else ed.max(axis=1))


# ------------------------------------------------------------------------------------------ 4: refusals
def test_refusals(H):
    from pyp_amd import lib
    h1, h2, m = F.gpu_inputs(32, True)
    ok = cfg_of(32, keep=False)
    bad = [(h1, h2, LocresCfg.make(PX, max_res=8.5), None),                      # above N a / 4
           (h1, h2, LocresCfg.make(PX, step=0.2), None),
           (h1, h2, LocresCfg.make(PX, min_res=6.0, max_res=5.0), None),         # no level
           (h1, h2, LocresCfg.make(4.0, min_res=10.0, max_res=32.0, step=0.25), None),   # more than 64
           (h1, h2, LocresCfg.make(0.0), None),
           (h1, h2, ok, np.zeros_like(h1)),                                      # nobody inside
           (np.zeros((34, 34, 34), np.float32), np.zeros((34, 34, 34), np.float32), LocresCfg.make(PX), None)]    # 34 = 2 x 17
    for a, b, cfg, mask in bad:
        with pytest.raises(lib.PpmError, match="ERROR"):
            H.local_resolution(a, b, cfg, mask=mask)
    with pytest.raises(ValueError, match="ERROR"):
        H.local_resolution(h1, h2[:16], ok)
    with pytest.raises(ValueError, match="ERROR"):
        H.local_resolution(h1, h2, ok, mask=m[:, :, :16])


# ------------------------------------------------------------------------------------------ 5: the program
def test_program(H, tmp_path, monkeypatch):
    """The command line of pyp_main.py:6826, from a shell, with and without --maskVol."""
    from pyp_amd.formats import mrc
    monkeypatch.setenv("PPM_LOCK_DIR", str(tmp_path))
    n = 32
    h1, h2, m = F.gpu_inputs(n, True)
    p1, p2, pm = (str(tmp_path / k) for k in ("t20s_r01_half1.mrc", "t20s_r01_half2.mrc", "mask.mrc"))
    for p, v in ((p1, h1), (p2, h2), (pm, m)):
        mrc.write(v, p, pixel_size=PX)
    exe = os.path.join(ROOT, "bin", "resmap")
    comm = f"{exe} --noguiSplit --vxSize {PX} --doBenchMarking --pVal 0.05 --minRes=0.0 --maxRes=0.0 --stepRes=1.0 --maskVol {pm} {p1} {p2}\n"
    r = subprocess.run(comm, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ResMap: Normal termination" in r.stdout, r.stdout + r.stderr
    out_map, out_cmd = p1.replace(".mrc", "_ori_resmap.mrc"), p1.replace(".mrc", "_ori_resmap_chimera.cmd")
    g = H.local_resolution(h1, h2, LocresCfg.make(PX), mask=m)
    assert np.array_equal(mrc.read(out_map), g["resolution"]) and abs(mrc.read_header(out_map)["pixel_size"] - PX) < 1e-6
    assert out_map in open(out_cmd).read() and "Notes" in r.stdout
    assert g["levels"].tolist() == [2.5, 3.5, 4.5] and g["info"].notes
    bad = comm.replace("t20s_r01_half1", "other_half1").replace("--maxRes=0.0", "--maxRes=9")
    os.rename(p1, p1.replace("t20s_r01_half1", "other_half1"))
    r = subprocess.run(bad, shell=True, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ERROR" in r.stdout and not [f for f in os.listdir(tmp_path) if "other_half1_ori" in f]


# ------------------------------------------------------------------------------------------ 6: the in-memory iteration
def test_iteration_adds_the_local_resolution(H):
    from pyp_amd import pipeline, synth
    from pyp_amd.abi import RefineCfg
    n, px = 32, 2.0
    vol, stack, rows = synth.make_dataset(n, 8, pixel=px, snr=0.5)
    imgs = stack.numpy()
    cfg = RefineCfg.make(box=n, pixel_size=px, mask_radius=0.4 * n * px, res_high=px * n / 12.0, global_search=0, res_signed_cc=30.0)
    kw = dict(pixel_size=px, molecular_mass_kda=50.0)
    lcfg = LocresCfg.make(px, step=2.0)
    plain = pipeline.iteration(vol, imgs, rows, cfg, **kw)
    none = pipeline.iteration(vol, imgs, rows, cfg, local_resolution=None, **kw)
    with_lr = pipeline.iteration(vol, imgs, rows, cfg, local_resolution=lcfg, **kw)
    assert sorted(plain) == sorted(none) == ["filtered", "half1", "half2", "rows", "stats"]
    assert sorted(with_lr) == sorted(list(plain) + ["local_resolution"])
    assert np.array_equal(plain["rows"], none["rows"]) and np.array_equal(plain["rows"], with_lr["rows"])
    want = H.local_resolution(with_lr["half1"], with_lr["half2"], lcfg)
    got = with_lr["local_resolution"]
    assert np.array_equal(got["resolution"], want["resolution"]) and np.array_equal(got["tau"], want["tau"])
    assert bytes(got["info"]) == bytes(want["info"]) and got["levels"].tolist() == [5.0, 7.0, 9.0]
