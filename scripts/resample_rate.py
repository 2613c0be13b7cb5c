#!/usr/bin/env python3
"""Rates of the Fourier resampling (ppm_resample) on resident data: images/s and the share of the HBM peak (8.0 TB/s) that the
COMPULSORY bytes - 4 (N^2 + M^2) per image, read once and written once - would need (the two line passes themselves move
4 (N^2 + 2 N M + M^2)), for

  256 -> 128   several rounds: the spread between rounds is what a difference between two builds has to exceed
  512 -> 256
  256^3 -> 128^3
  bin/resample_mp.exe on a stack file of --file-images 256^2 images (wall time of the whole program; 0 = skip)

Every call ends in the library's own stream synchronise, so a host clock around it measures finished work.  One JSON line per figure.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyp_amd import host  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def stack_rate(n, m, images, reps):
    x = stack_rate.cache.setdefault((n, images), torch.randn(images, n, n, device="cuda"))
    out = stack_rate.cache.setdefault((m, images, "o"), torch.empty(images, m, m, device="cuda"))
    host.resample(x, m, out=out)                                                  # warm-up of this shape
    dt = timed(lambda: host.resample(x, m, out=out), reps)
    return dict(n=n, m=m, images=images, ms=1e3 * dt, images_per_s=images / dt,
                hbm_share_of_compulsory_bytes=4.0 * (n * n + m * m) * images / dt / HBM_PEAK,
                hbm_share_of_bytes_moved=4.0 * (n * n + 2 * n * m + m * m) * images / dt / HBM_PEAK)


stack_rate.cache = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--file-images", type=int, default=20000)
    a = ap.parse_args()
    rates = []
    for r in range(a.rounds):
        res = stack_rate(256, 128, a.images, a.reps)
        rates.append(res["images_per_s"])
        print(json.dumps(dict(res, round=r)), flush=True)
    print(json.dumps(dict(summary="256->128", median_images_per_s=float(np.median(rates)), spread_between_rounds=(max(rates) - min(rates)) / float(np.median(rates)))), flush=True)
    stack_rate.cache.clear()
    print(json.dumps(stack_rate(512, 256, max(a.images // 4, 1), a.reps)), flush=True)
    stack_rate.cache.clear()
    v = torch.randn(256, 256, 256, device="cuda")
    o = torch.empty(128, 128, 128, device="cuda")
    host.resample(v, 128, volume=True, out=o)
    dt = timed(lambda: host.resample(v, 128, volume=True, out=o), a.reps)
    print(json.dumps(dict(volume="256^3 -> 128^3", ms=1e3 * dt, hbm_share_of_compulsory_bytes=4.0 * (256 ** 3 + 128 ** 3) / dt / HBM_PEAK)), flush=True)
    del v, o
    if a.file_images > 0:
        from pyp_amd.formats import mrc
        with tempfile.TemporaryDirectory() as d:
            src, dst = os.path.join(d, "stack.mrc"), os.path.join(d, "binned.mrc")
            mm = mrc.create(src, (a.file_images, 256, 256), pixel_size=1.0)
            block = np.random.default_rng(1).standard_normal((256, 256, 256)).astype(np.float32)
            for i0 in range(0, a.file_images, 256):
                mm[i0:i0 + 256] = block[:min(256, a.file_images - i0)]
            mm.flush()
            del mm
            answers = "\n".join([src, dst, "no", "no", "128", "128"]) + "\n"
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "resample_mp.exe")], input=answers, capture_output=True, text=True,
                               env=dict(os.environ, PPM_LOCK_DIR=d))
            wall = time.perf_counter() - t0
            ok = r.returncode == 0 and "Normal termination" in r.stdout
            print(json.dumps(dict(program="bin/resample_mp.exe", images=a.file_images, n=256, m=128, wall_s=wall, ok=ok,
                                  timing=[ln for ln in r.stdout.splitlines() if ln.startswith("Timing")])), flush=True)
            if not ok:
                print(r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    main()
