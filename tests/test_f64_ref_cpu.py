"""The float64 reference (tests/f64_ref.py) pinned against the CPU oracle, its CTF against the generator's, and proof that
its shell-by-shell comparator catches defects the whole-volume rel-L2 < 1e-4 check of the GPU parity tests lets through.

Oracle bounds: the oracle stores the image, its FFT and every accumulator voxel in float32 (ppm_oracle.c: `cpx` is two
floats, the accumulators are float), so each value carries a relative round-off of a few eps32 = 1.2e-7 per operation
(normalised image, log2 N FFT stages, the CTF and shift product, up to 8 x 6 accumulations per voxel).  A shell's relative L2
error therefore sits near 1e-7 and a single voxel's error near 1e-6 of its shell's RMS; the bounds are 1e-6 per shell and 2e-5
per voxel (the measured floors at these boxes are 3e-7 and 5e-6)."""
import numpy as np
import pytest

import f64_ref as R
from pyp_amd import synth
from pyp_amd.abi import FinalCfg, ReconCfg

CPU_BOXES = [32, 42, 50, 70, 98]       # odd N/2 (42, 50, 70, 98), radix 3 / 5 / 7, a box that is not a multiple of 4
ORACLE_SHELL, ORACLE_VOXEL = 1e-6, 2e-5


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_supported_boxes():
    b = R.supported_boxes()
    assert len(b) == 64 and b[0] == 32 and b[-1] == 512 and 490 in b and 486 in b and 44 not in b and 66 not in b


def recon_case(N):
    px, imgs, rows = R.seeded_particles(N, 6, N)
    rows[1, R.C["BEAM_TILT_X"]], rows[1, R.C["BEAM_TILT_Y"]] = 1.5, -1.0
    rows[2, R.C["OCCUPANCY"]] = 60.0
    rows[3, R.C["OCCUPANCY"]] = 0.0                                    # rejected
    rows[:, R.C["TIND"]] = np.arange(6) % 3
    rc = ReconCfg(box=N, pixel_size=px, res_limit=2 * px, score_weight_bfactor=2.0, score_average=20.0, score_threshold=0.0,
                  normalize=1, invert=0, split_by_pind=1, mask_radius=0.4 * N * px)
    rc.set_dose_weights([1.0, 0.8, 0.6], 4.0, 0.75)
    return px, imgs, rows, rc


@pytest.mark.parametrize("sym", ["C1", "D2"])
@pytest.mark.parametrize("N", CPU_BOXES)
def test_float64_insert_and_finalize_match_oracle(O, N, sym):
    px, imgs, rows, rc = recon_case(N)
    acc = np.zeros(O.accum_floats(N), np.float32)
    counts = np.zeros(2, np.int64)
    O.insert_batch(acc, counts, rc, sym, imgs, rows)
    want, c = R.insert(N, px, R.symmetry_ops(sym), imgs, rows, rc)
    assert list(counts) == c == [3, 2]
    rep = R.compare_by_shell(acc, want, N)
    assert rep.max_shell_rel < ORACLE_SHELL and rep.max_voxel_rel < ORACLE_VOXEL, f"box {N} {sym}: {rep}"
    assert R.stray_values(acc, want) == 0
    fc = FinalCfg(molecular_mass_kda=300.0, inner_radius=0.0, outer_radius=0.45 * N * px, mask_falloff=0.0)
    o = O.finalize(acc, N, float(np.float32(px)), fc)
    f = R.finalize(want, N, px, fc)
    assert np.array_equal(o[3][:, :3], f[3][:, :3])                    # shell, resolution, radius
    assert np.abs(o[3][:, 3:5] - f[3][:, 3:5]).max() < 1e-6            # FSC, part-FSC: ratios of float32-stored sums
    rel = np.abs(o[3][:, 5:7] - f[3][:, 5:7]) / np.maximum(np.abs(f[3][:, 5:7]), 1.0)
    assert rel.max() < 1e-4, rel.max()                                 # SSNRs: 1 / (1 - FSC) amplifies near FSC = 0.999
    for a, b in zip(o[:3], f[:3]):                                     # maps: float32 3-D FFT of the oracle
        assert R.rel_l2(a, b) < 2e-6


def test_ctf_matches_the_generator():
    """f64_ref.ctf against pyp_amd.synth.ctf_image (independent of the oracle) on the full centred grid, float32 vs float64:
    chi reaches ~60 rad here, so float32 phases are good to ~1e-5."""
    N, px = 98, 1.3
    _, _, rows = R.seeded_particles(N, 3, 5, px=px)
    rows[:, R.C["PHASE_SHIFT"]] = [0.0, 0.3, 1.1]
    k = np.arange(-N // 2, N // 2)
    ky, kx = np.meshgrid(k, k, indexing="ij")
    for r in rows:
        want = synth.ctf_image(N, px, [r[6]], [r[7]], [r[8]], 300.0, 2.7, 0.07, r[9], "cpu")[0].numpy()
        got = R.ctf(r, N, px, kx, ky)
        tol = 4 * R.EPS32 * R.max_ctf_phase(r, N, px, N / np.sqrt(2)) + 1e-6
        assert np.abs(got - want).max() < tol


def test_prep_band_beam_tilt_removes_the_rendered_tilt():
    """A rendered image of a tilted beam, prepared with the row's tilt, equals the untilted one's band (noise-free)."""
    N, px = 64, 1.5
    vol = synth.phantom(N, n_blobs=6, n_atoms=200)
    _, _, rows = synth.make_dataset(N, 1, pixel=px, snr=0, vol=vol)
    tilted = rows.copy()
    tilted[:, 19], tilted[:, 20] = 1.5, -1.0
    a = synth.render_rows(vol, rows, px, snr=0, normalize=False).numpy()[0]
    b = synth.render_rows(vol, tilted, px, snr=0, normalize=False).numpy()[0]
    pa = R.prep_band(a, rows[0], N, px, N / 2 - 1, 0, 0, 0.4 * N * px)
    pb = R.prep_band(b, tilted[0], N, px, N / 2 - 1, 0, 0, 0.4 * N * px)
    assert np.linalg.norm(pa - pb) / np.linalg.norm(pa) < 1e-5
    assert np.linalg.norm(pa - R.prep_band(b, rows[0], N, px, N / 2 - 1, 0, 0, 0.4 * N * px)) / np.linalg.norm(pa) > 1e-2


# ----------------------------------------------------------------------------------------------------------- mutations
def mutations(acc, N):
    """Defects a kernel could make, applied one at a time to the float64 accumulator in place (yielded, then undone: at 512 a
    copy is 3.2 GB)."""
    ns = N // 2
    shell = R.shell_index(N)
    energy = np.bincount(shell.ravel(), weights=(acc ** 2).sum(axis=(0, 4)).ravel())
    b = 2 + int(np.argmin(np.where(energy[2:ns] > 0, energy[2:ns], np.inf)))
    sel = shell == b
    keep = acc[:, sel, :].copy()
    acc[:, sel, :] *= 1.0 + 1e-3                                        # the populated shell of least energy scaled by 1 + 1e-3
    yield "scale one shell"
    acc[:, sel, :] = keep
    keep = acc[:, ns + 3, :, 0, 1].copy()
    acc[:, ns + 3, :, 0, 1] *= -1.0                                     # one line (kz = 3) of the kx = 0 plane conjugated
    yield "conjugate a kx=0 line"
    acc[:, ns + 3, :, 0, 1] = keep
    y0 = int(np.flatnonzero(acc[..., 2].any(axis=(0, 1, 3)))[0])      # ky = -N/2, or the lowest ky the slices reach
    keep = acc[:, :, y0].copy()
    acc[:, :, y0] = 0.0                                                 # that edge row of every plane zeroed
    yield "zero the ky edge row"
    acc[:, :, y0] = keep
    w = acc[0, ..., 2]
    z, y, x = np.unravel_index(int(np.argmax(np.where(shell == ns // 2, w, 0))), w.shape)
    keep = acc[0, z, y, x:x + 2, 2].copy()
    acc[0, z, y, x + 1, 2] += acc[0, z, y, x, 2]                        # one voxel's weight moved to its kx neighbour
    acc[0, z, y, x, 2] = 0.0
    yield "move one weight"
    acc[0, z, y, x:x + 2, 2] = keep


@pytest.mark.parametrize("N", [42, 64, 98, 384, 512])
def test_comparator_flags_defects_the_old_bound_misses(N):
    """compare_by_shell at the GPU sweep's bounds flags each defect; the whole-volume rel-L2 < 1e-4 of test_gpu_parity.py
    misses at least one (scaling the shell of least energy by 1 + 1e-3 moves the whole volume by well under 1e-4).  Run at
    the largest boxes too, where the CTF phase term makes the bounds widest (at 512: shell 7.4e-4, voxel 0.074 of the shell RMS)."""
    px, imgs, rows, rc = R.leg_a_rows(N)
    acc, _ = R.insert(N, px, R.symmetry_ops("C1"), imgs, rows, rc)
    model = R.floor_model(N, rows)
    assert R.compare_by_shell(acc.astype(np.float32), acc, N).ok(R.SHELL_K * model, R.VOXEL_K * model)   # float32 storage passes
    missed = []
    ref = acc.astype(np.float32)             # the comparison side: float32, as a kernel's download
    for name in mutations(acc, N):
        rep = R.compare_by_shell(acc, ref, N)
        assert not rep.ok(R.SHELL_K * model, R.VOXEL_K * model), (name, str(rep))
        if R.rel_l2(acc, ref) < 1e-4:
            missed.append(name)
    assert "scale one shell" in missed, missed

