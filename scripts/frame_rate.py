"""Rate of movie-frame refinement (host.Reference.frame_refine) on one tilt series: 300 particles x 41 tilts x 8 frames at box 128 by
default, the frame stack resident on the device.  Prints rows per second and the split of the device time between k_prep and the frame
kernels (the library's profiling counters: `prep`, and `local`, which in this call holds k_frame_maps + k_frame_peak alone).  The frames
of a (particle, tilt) are its tilt-series projection with fresh noise: the timing does not depend on the images' content."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyp_amd import host, synth  # noqa: E402
from pyp_amd.abi import FrameCfg, RefineCfg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=300)
ap.add_argument("--tilts", type=int, default=41)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--box", type=int, default=128)
ap.add_argument("--band", type=float, default=40.0, help="high-resolution limit in Fourier pixels")
ap.add_argument("--range", type=float, default=2.0, help="shift range, pixels")
ap.add_argument("--half-width", type=int, default=2)
a = ap.parse_args()

N, px, F = a.box, 1.5, a.frames
C = synth.cistem.COL
vol = synth.phantom(64)
if N > 64:
    big = np.zeros((N, N, N), dtype=np.float32)
    o = N // 2 - 32
    big[o:o + 64, o:o + 64, o:o + 64] = vol
    vol = big
angles = np.linspace(-60.0, 60.0, a.tilts)
_, _, rows0, _, _ = synth.make_tilt_series(N, a.particles, angles, pixel=px, snr=0.2, vol=vol, device="cuda")
m0 = len(rows0)
rows = np.repeat(rows0, F, axis=0)
rows[:, C["FIND"]] = np.tile(np.arange(F), m0)
rows[:, C["POSITION_IN_STACK"]] = np.arange(1, m0 * F + 1)
stack = synth.render_rows(vol, rows0, px, 0.2, 3, "cuda", 64, m=m0 * F, rep=np.repeat(np.arange(m0), F))
cfg = RefineCfg.make(box=N, pixel_size=px, mask_radius=0.4 * N * px, res_high=px * N / a.band, global_search=0, local_refine=0)
fc = FrameCfg.make(a.range, 0.0, a.half_width)
ref = host.Reference(vol, N / 2)
warm = min(len(rows), 64 * F)
ref.frame_refine(cfg, fc, stack[:warm], rows[:warm])
host.profile(True, True)
t = time.perf_counter()
out, info = ref.frame_refine(cfg, fc, stack, rows)
dt = time.perf_counter() - t
pr = host.profile_report()
prep, frame = pr["prep"]["ms"], pr["local"]["ms"]
print(json.dumps(dict(rows=len(rows), box=N, band_px=a.band, grid=2 * info["n_steps"] + 1, half_width=a.half_width, seconds=round(dt, 4),
                      rows_per_s=round(len(rows) / dt, 1), k_prep_ms=round(prep, 2), frame_kernels_ms=round(frame, 2),
                      frame_share=round(frame / max(prep + frame, 1e-9), 3), groups=info["groups"], models=info["models"],
                      moved_px_median=round(float(np.median(np.hypot(out[:, 4] - rows[:, 4], out[:, 5] - rows[:, 5]))) / px, 4))))
