"""Cost of point-group symmetry on the sub-tomogram path at BASELINE config 5's geometry (192^3 sub-volumes, resident, one MI355X):
ppm_sva_insert into a C1 and a C6 accumulator, and the global search (ppm_sva_cfg.search_mode 1) over the full grid and over C6's
asymmetric unit.  One warm-up and REPEATS timed repeats each; transform (PPM_K_PREP) and gather (PPM_K_INSERT) times from ppm_profile_get.
    sva_sym_rate.py [box] [n_vol] [symbol ...]          (default 192 64 C1 C6)
A library without the feature refuses the symbols other than C1; the script says so and goes on (the C1 figures of two builds compare:
the sha256 of the C1 accumulator after the warm-up is printed for that)."""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyp_amd import host, lib, synth
from pyp_amd.abi import SvaCfg

REPEATS = 3
n = int(sys.argv[1]) if len(sys.argv) > 1 else 192
nv = int(sys.argv[2]) if len(sys.argv) > 2 else 64
symbols = sys.argv[3:] or ["C1", "C6"]
vol, vols, poses, wedges = synth.make_subtomograms(n, nv, snr=0.1, device="cuda")
torch.cuda.synchronize()


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x))


icfg = SvaCfg.make(n, use_missing_wedge=1)
for sym in symbols:
    acc = host.Accumulator(n, 1.0, sym)
    try:
        acc.sva_insert(icfg, vols, wedges, poses)              # warm-up
    except lib.PpmError as e:
        print("insert %s: refused by this library (%s)" % (sym, e))
        acc.close()
        continue
    digest = hashlib.sha256(acc.download().tobytes()).hexdigest()[:16]
    wall, prep, ins = [], [], []
    for _ in range(REPEATS):
        host.profile(True, True)
        t0 = time.time()
        acc.sva_insert(icfg, vols, wedges, poses)
        wall.append((time.time() - t0) * 1e3 / nv)
        p = host.profile_report()
        prep.append(p["prep"]["ms"] / nv); ins.append(p["insert"]["ms"] / nv)
    host.profile(False, False)
    acc.close()
    print("insert %s box %d, %d sub-volumes, ms per sub-volume, median (min .. max) of %d: wall %s, transforms %s, gather %s; sha256 after one call %s" % (
        sym, n, nv, REPEATS, spread(wall), spread(prep), spread(ins), digest))

rng = np.random.default_rng(4)
start = poses.copy()
for v in range(nv):
    R = synth.euler_matrix(rng.uniform(0, 360), np.degrees(np.arccos(rng.uniform(-1, 1))), rng.uniform(0, 360))
    start[v, :9] = (poses[v, :9].reshape(3, 3) @ R).ravel()
ref = host.Reference(vol, n / 2)
for sym in symbols:
    cfg = SvaCfg.make(n, window=(0.33 * n, 0.33 * n, 0.33 * n), window_sigma=4.0, highpass=(0.05, 0.01), lowpass=(0.125, 0.05), tol_angle=10.0, tol_shift=10.0,
                      search_mode=1, global_step=15.0)
    if sym != "C1":
        if not hasattr(cfg, "symmetry"):
            print("global search %s: this library's settings have no symmetry field" % sym)
            continue
        cfg.symmetry = sym.encode()
    ref.sva_align(cfg, vols, wedges, start)                     # warm-up
    wall, glob, loc = [], [], []
    for _ in range(REPEATS):
        host.profile(True, True)
        t0 = time.time()
        ref.sva_align(cfg, vols, wedges, start)
        wall.append((time.time() - t0) * 1e3 / nv)
        p = host.profile_report()
        glob.append(p["global"]["ms"] / nv); loc.append(p["local"]["ms"] / nv)
    host.profile(False, False)
    print("global search %s box %d, step 15, grid %d, ms per sub-volume, median (min .. max) of %d: wall %s, grid ranking %s, candidate sweeps %s" % (
        sym, n, ref.last_counts()["n_global"], REPEATS, spread(wall), spread(glob), spread(loc)))
ref.close()
