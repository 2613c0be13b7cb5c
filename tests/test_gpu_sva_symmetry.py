"""Point-group symmetry on the sub-tomogram path, on the GPU: the symmetrised average (k_sva_insert<true>: every sub-volume once per
operator S at the pose (S N, p)) against the untouched oracle fed the expanded data set, the resident and the fused paths, the global
search cut to the asymmetric unit (candidates G N0) against the full grid, bin/sva_align with the protocol's symmetry order, and a
loud refusal of an unknown symbol."""
import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import FinalCfg, SvaCfg

FINAL = dict(molecular_mass_kda=0.0, inner_radius=0.0, outer_radius=0.0, mask_falloff=0.0)


def cc(a, b, mask):
    a, b = a[mask], b[mask]
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def ball(n, r):
    k = np.arange(n) - n // 2
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    return (x * x + y * y + z * z) < r * r


def cfg_for(n, **kw):          # the alignment settings of tests/test_sva.py
    base = dict(window=(12, 12, 12), window_sigma=2.0, highpass=(0.03, 0.01), lowpass=(0.30, 0.04), tol_angle=10.0, tol_shift=4.0)
    base.update(kw)
    return SvaCfg.make(n, **base)


def sym_angle_error(found, truth, ops):
    """Per sub-volume: the smallest angle between S N_found and N_true over the operators S, degrees."""
    out = []
    for x, y in zip(found, truth):
        Nf, Nt = x[:9].reshape(3, 3), y[:9].reshape(3, 3)
        t = max((np.trace((S @ Nf).T @ Nt) - 1.0) / 2.0 for S in ops)
        out.append(np.degrees(np.arccos(np.clip(t, -1.0, 1.0))))
    return np.array(out)


@pytest.mark.gpu
@pytest.mark.parametrize("n,sym,nv,generic", [(48, "C3", 8, False), (40, "C3", 5, False), (48, "D2", 4, True)])
def test_gpu_symmetrised_average_is_the_oracles_average_of_the_expanded_set(n, sym, nv, generic, monkeypatch):
    """ppm_sva_insert into a Cn / Dn accumulator against orc_sva_insert on C1 with every sub-volume repeated once per operator at the pose
    (S N, p), same wedge and index: the comparisons and tolerances of test_gpu_average_matches_oracle (the same kernel arithmetic, at most
    24 summands against that test's 20).  ppm_accum_count counts the sub-volumes once each."""
    from oracle import oracle as O
    from pyp_amd import host as H
    if generic:
        monkeypatch.setenv("PPM_SVA_GENERIC_FFT", "1")
    ops = O.symmetry_ops(sym)
    vol, vols, poses, wedges = synth.make_subtomograms(n, nv, snr=0.5, seed=5, vol=synth.phantom_sym(n, ops))
    vols = vols.numpy()
    wedges[::3] = (-50.0, 64.0)
    poses = synth.perturb_poses(poses, 1.0, 0.5)
    index = np.arange(nv) * 3 + 1
    halves = (slice(0, nv // 2), slice(nv // 2, nv))
    # the expanded set in the order the sums are made: per call the operators, inside an operator the call's sub-volumes
    who = np.concatenate([np.tile(np.arange(nv)[h], len(ops)) for h in halves])
    which = np.concatenate([np.repeat(np.arange(len(ops)), len(np.arange(nv)[h])) for h in halves])
    xposes = poses[who].copy()
    for r, (v, s) in enumerate(zip(who, which)):
        xposes[r, :9] = (ops[s] @ poses[v, :9].reshape(3, 3)).ravel()
    acc_o, cnt_o = np.zeros(O.accum_floats(n), np.float32), np.zeros(2, np.int64)
    O.sva_insert(acc_o, cnt_o, SvaCfg.make(n, use_missing_wedge=1), vols[who], wedges[who], xposes, index[who])
    h1o, h2o, flo, st_o = O.finalize(acc_o, n, 1.0, FinalCfg(**FINAL))
    acc = H.Accumulator(n, 1.0, sym)
    cfg = SvaCfg.make(n, use_missing_wedge=1)
    for h in halves:                      # two calls: sums accumulate
        acc.sva_insert(cfg, vols[h], wedges[h], poses[h], index[h])
    g = acc.download()
    assert acc.counts() == [int((index % 2 == 0).sum()), int((index % 2 == 1).sum())]
    assert list(cnt_o) == [len(ops) * c for c in acc.counts()]
    go, gg = acc_o.reshape(-1, 3), g.reshape(-1, 3)
    ok = gg[:, 2] == go[:, 2]
    h1, h2, fl, st = acc.finalize(FinalCfg(**FINAL))
    acc.close()
    print("%s n %d: weights off by %.3g of %.3g, values rel L2 %.3g, maps %.3g x max, FSC %.3g" % (
        sym, n, np.abs(gg[:, 2] - go[:, 2]).sum(), go[:, 2].sum(), np.linalg.norm((gg - go)[ok, :2]) / np.linalg.norm(go[:, :2]),
        max(np.abs(a - b).max() / np.abs(b).max() for a, b in ((h1, h1o), (h2, h2o), (fl, flo))), np.abs(st[:, 3] - st_o[:, 3]).max()))
    assert np.abs(gg[:, 2] - go[:, 2]).sum() <= 1e-4 * go[:, 2].sum()            # a wedge edge can flip a voxel between float and double
    assert np.linalg.norm((gg - go)[ok, :2]) < 2e-5 * np.linalg.norm(go[:, :2])
    for a, b in ((h1, h1o), (h2, h2o), (fl, flo)):
        assert np.abs(a - b).max() < 2e-3 * np.abs(b).max()
    assert np.abs(st[:, 3] - st_o[:, 3]).max() < 2e-3


@pytest.mark.gpu
def test_gpu_symmetrised_average_resident_and_fused_paths_give_the_same_bits():
    """Under C3: a CUDA tensor gives the accumulator of host volumes, and ppm_sva_align_average the accumulator of ppm_sva_align
    followed by ppm_sva_insert (5 sub-volumes: one chunk, one batch - the same sums in the same order)."""
    import torch  # noqa: F401
    from oracle import oracle as O
    from pyp_amd import host as H
    n, nv = 32, 5
    vol, vols, poses, wedges = synth.make_subtomograms(n, nv, snr=0.5, seed=4, vol=synth.phantom_sym(n, O.symmetry_ops("C3")))
    index = np.arange(nv) + 7
    cfg = cfg_for(n)
    a1, a2 = H.Accumulator(n, 1.0, "C3"), H.Accumulator(n, 1.0, "C3")
    a1.sva_insert(cfg, vols.numpy(), wedges, poses, index)
    a2.sva_insert(cfg, vols.cuda(), wedges, poses, index)
    x, y = a1.download(), a2.download()
    a1.close(); a2.close()
    assert x.any() and np.array_equal(x, y)
    start = synth.perturb_poses(poses, 3.0, 1.0)
    ref = H.Reference(vol, n / 2)
    p0, s0 = ref.sva_align(cfg, vols.numpy(), wedges, start)
    a0 = H.Accumulator(n, 1.0, "C3")
    a0.sva_insert(cfg, vols.numpy(), wedges, p0, index)
    want, wc = a0.download(), a0.counts()
    a0.close()
    a3 = H.Accumulator(n, 1.0, "C3")
    p1, s1 = ref.sva_align(cfg, vols.numpy(), wedges, start, accumulator=a3, index=index)
    got, gc = a3.download(), a3.counts()
    a3.close(); ref.close()
    assert np.array_equal(p1, p0) and np.array_equal(s1, s0) and gc == wc == [2, 3]
    assert np.array_equal(got, want)
    w = want.reshape(2, n, n, n // 2 + 1, 3)[..., 2]
    assert w.max() <= 3 * 3 and w.max() > 3                    # weights count (sub-volume, operator) pairs, the counters sub-volumes


@pytest.mark.gpu
def test_gpu_global_search_on_the_asymmetric_unit_finds_what_the_full_grid_finds():
    """A C4 phantom (a 90 degree turn maps the voxel grid onto itself: the reference is exactly symmetric), starts anywhere on SO(3) as in
    test_gpu_global_search_matches_oracle.  The search with symmetry = "C4" ranks 504 grid rotations instead of 1908 and places at least
    as many sub-volumes within 1.5 degrees of an equivalent of the true rotation; where both runs do, their scores agree to 0.01."""
    from oracle import oracle as O
    from pyp_amd import host
    n = 32
    ops = O.symmetry_ops("C4")
    vol, vols, poses, wedges = synth.make_subtomograms(n, 6, snr=0.5, wedge=(-54.0, 60.0), vol=synth.phantom_sym(n, ops))
    rng = np.random.default_rng(4)
    start = poses.copy()
    for v in range(len(start)):
        R = synth.euler_matrix(rng.uniform(0, 360), np.degrees(np.arccos(rng.uniform(-1, 1))), rng.uniform(0, 360))
        start[v, :9] = (poses[v, :9].reshape(3, 3) @ R).ravel()
        start[v, 9:] += rng.normal(0, 1.5, 3)
    g = host.Reference(vol, n / 2)
    c1 = cfg_for(n, search_mode=1, global_step=20.0)
    c4 = cfg_for(n, search_mode=1, global_step=20.0, symmetry="C4")
    p1, s1 = g.sva_align(c1, vols.numpy(), wedges, start)
    n1 = g.last_counts()["n_global"]
    p4, s4 = g.sva_align(c4, vols.numpy(), wedges, start)
    n4 = g.last_counts()["n_global"]
    e1, e4 = sym_angle_error(p1, poses, ops), sym_angle_error(p4, poses, ops)
    print("C1 grid %d: errors %s scores %s\nC4 grid %d: errors %s scores %s" % (n1, np.round(e1, 3), np.round(s1, 4), n4, np.round(e4, 3), np.round(s4, 4)))
    assert (n1, n4) == (1908, 504)
    assert (e4 < 1.5).sum() >= (e1 < 1.5).sum()
    both = (e1 < 1.5) & (e4 < 1.5)
    assert both.any() and np.abs(s1[both] - s4[both]).max() < 0.01
    p4r, s4r = g.sva_align(c4, vols.cuda(), wedges, start)                   # resident volumes, same bits
    g.close()
    assert np.array_equal(p4, p4r) and np.array_equal(s4, s4r)


@pytest.mark.gpu
def test_sva_align_executable_applies_the_protocols_symmetry(tmp_path):
    """bin/sva_align on a mode-2 protocol with <refine_use_symmetrization>4: the average is its own quarter turn about z to the map
    tolerance (a C1 average of five noisy sub-volumes is far from that) and resembles the C4 phantom more than the run with the field at 1."""
    import os
    import subprocess
    import sys
    from oracle import oracle as O
    from pyp_amd import sva
    from pyp_amd.formats import mrc
    n, nv = 32, 5
    vol, vols, poses, wedges = synth.make_subtomograms(n, nv, snr=0.5, vol=synth.phantom_sym(n, O.symmetry_ops("C4")))
    start = synth.perturb_poses(poses, 3.0, 1.0)
    tab = np.zeros((nv, 32)); names = []
    for k in range(nv):
        tab[k, 0], tab[k, 1], tab[k, 2] = k + 1, wedges[k, 0], wedges[k, 1]
        tab[k, 12:28] = sva.pose_to_matrix(start[k, :9], start[k, 9:], tab[k, 9:12])
        names.append(f"TS_01_spk{k:04d}.rec")
        mrc.write(vols[k].numpy(), str(tmp_path / names[-1]))
    sva.write_volumes(str(tmp_path / "d_volumes.txt"), tab, names)
    mrc.write(vol, str(tmp_path / "ref.mrc"))
    protocol = """<config><general><mode>2</mode><metric><use_missing_wedge>1</use_missing_wedge></metric></general>
      <refine><refine_image_window_x>12</refine_image_window_x><refine_image_window_y>12</refine_image_window_y><refine_image_window_z>12</refine_image_window_z>
      <refine_image_window_sigma>2</refine_image_window_sigma><refine_high_pass_cutoff>.03</refine_high_pass_cutoff><refine_high_pass_decay>.01</refine_high_pass_decay>
      <refine_low_pass_cutoff>0.30</refine_low_pass_cutoff><refine_low_pass_decay>.04</refine_low_pass_decay>
      <refine_out_of_plane_search_range>10</refine_out_of_plane_search_range><refine_shifts_tolerance>4.0</refine_shifts_tolerance>
      <refine_use_symmetrization>%d</refine_use_symmetrization></refine></config>"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "sva_align")
    m = ball(n, 0.4 * n)
    got = {}
    for order in (4, 1):
        (tmp_path / "p.xml").write_text(protocol % order)
        r = subprocess.run([sys.executable, exe, "p.xml", "d_volumes.txt", "ref.mrc", "out_%d.txt" % order, "avg_%d" % order], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0 and "SVA: Normal termination" in r.stdout and "Averaged 3 + 2 sub-volumes" in r.stdout, r.stdout + r.stderr
        assert ("Symmetry C%d" % order) in r.stdout, r.stdout
        got[order] = mrc.read(str(tmp_path / ("avg_%d.mrc" % order)))
    a4, a1 = got[4], got[1]
    # a quarter turn about z through the box origin, voxel n / 2: np.rot90 turns about the middle of the array it is given, so it gets
    # the planes 1 .. n - 1 of y and x, which have voxel n / 2 in their middle (plane 0, at -n / 2, has no partner)
    a4, a1 = a4[:, 1:, 1:], a1[:, 1:, 1:]
    vol, m = vol[:, 1:, 1:], m[:, 1:, 1:]
    turn = lambda a: np.rot90(a, 1, axes=(1, 2))               # array axes z, y, x
    print("asymmetry: C4 %.3g x max, C1 %.3g x max; cc with the phantom: C4 %.4f, C1 %.4f" % (
        np.abs(a4 - turn(a4)).max() / np.abs(a4).max(), np.abs(a1 - turn(a1)).max() / np.abs(a1).max(), cc(a4, vol, m), cc(a1, vol, m)))
    assert np.abs(a4 - turn(a4)).max() < 2e-3 * np.abs(a4).max()
    assert np.abs(a1 - turn(a1)).max() > 2e-2 * np.abs(a1).max()
    assert cc(a4, vol, m) > cc(a1, vol, m)


@pytest.mark.gpu
def test_gpu_unknown_symmetry_symbol_is_refused_with_a_message():
    from pyp_amd import host, lib
    n = 32
    vol, vols, poses, wedges = synth.make_subtomograms(n, 2, snr=0.5)
    g = host.Reference(vol, n / 2)
    for bad in ("X9", "C61"):
        with pytest.raises(lib.PpmError, match="ERROR.*symmetry symbol '%s'" % bad):
            g.sva_align(cfg_for(n, symmetry=bad, search_mode=1), vols.numpy(), wedges, poses)
    # the field is read by the global search only, and the handle is fit for use after the refusal
    out, sc = g.sva_align(cfg_for(n, symmetry="X9"), vols.numpy(), wedges, poses)
    g.close()
    assert out.shape == (2, 12) and sc.min() > 0.8
