#!/usr/bin/env python
"""
tools/bench_displacement.py — the displacement kernels (csrc/displacement.hip) on device-resident frames: 315 entities
x 10 000 frames with one job (the ions of the residence example) and 50 000 entities x 5 000 frames with four jobs
(configuration C4's shape), wrapped coordinates (image counts rebuilt) and unwrapped ones. Times every call with the
library's own event timer (all launches of the call under one timer) and a host clock around the synchronous call,
after a warm-up call, and sets both against ONE read of the trajectory — 24 B per entity per frame — at the HBM rate
profiles/r05_ubench_hbm.txt measured for a flat streaming read (7.2 TB/s). Next to the measured ratio stands the byte
count the design implies, in reads of the trajectory per call:
  image counts   1 (shift totals) + 1.5 (the shifts again, 4 B of image count written per 8 B read)
  binning        per job, windows / (frames * entities) of 2 frames x (8 B coordinate + 4 B image count) = 3 reads
                 wrapped, 2 unwrapped, before any reuse in cache (a frame is the start of one window and the end of
                 another, of every job)
Writes profiles/displacement_bench.json.

    python tools/bench_displacement.py [--reps 10] [--shapes 315x10000x1,50000x5000x4] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import displacement_ref as R  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

HBM_BYTES_PER_S = 7.2e12  # profiles/r05_ubench_hbm.txt, flat 8 KB per block
BIN, N_BINS, BOX, CHECK_FRAMES = 0.05, 300, 30.0, 200
LAGS = {1: [100], 4: [10, 100, 1000, 2500]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="315x10000x1,50000x5000x4")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "displacement_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    rec = {"device": ctx.name, "bin_size": BIN, "n_bins": N_BINS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": []}
    for shape in a.shapes.split(","):
        n, frames, n_jobs = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n)
        xu = torch.randn((frames, 3, n), generator=g, device="cuda", dtype=torch.float64) * 0.05
        xu[0] = torch.rand((3, n), generator=g, device="cuda", dtype=torch.float64) * BOX
        xu.cumsum_(dim=0)
        x = torch.remainder(xu, BOX)
        box = np.full((frames, 3), BOX)
        off = np.array([0, n], dtype=np.int64)
        lags = LAGS.get(n_jobs) or [max(1, (frames - 1) * (j + 1) // (2 * n_jobs)) for j in range(n_jobs)]
        jobs = [(0, k, 1) for k in lags]
        once = frames * n * 24
        roof_ms = once / HBM_BYTES_PER_S * 1e3
        share = sum((frames - k) / frames for k in lags)
        srec = {"entities": n, "frames": frames, "jobs": jobs, "trajectory_bytes": once, "one_read_ms": roof_ms}
        for name, r, bx, reads in (("wrapped", x, box, 2.5 + 3.0 * share), ("unwrapped", xu, None, 2.0 * share)):
            ms, wall = [], []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                out = B.displacement_hist(r, bx, off, jobs, BIN, N_BINS, ctx=ctx)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(ctx.last_kernel_ms()[0])
            ms, wall = np.array(ms[1:]), np.array(wall[1:])
            med = float(np.median(ms))
            srec[name] = {"launches": ctx.last_kernel_ms()[1], "kernel_median_ms": med, "kernel_best_ms": float(ms.min()),
                          "wall_median_ms": float(np.median(wall)), "kernel_over_one_read": med / roof_ms,
                          "wall_over_one_read": float(np.median(wall)) / roof_ms, "design_reads_of_trajectory": reads,
                          "windows": [int(w) for w in out[2]], "beyond_r_max": [int(w) for w in out[1]],
                          "crossings": out[4], "reps": a.reps}
        # the same integers as the numpy restatement on the first frames
        nf = min(frames, CHECK_FRAMES)
        small = [(0, min(k, nf - 1), 1) for k in lags]
        got = B.displacement_hist(x[:nf].contiguous(), box[:nf], off, small, BIN, N_BINS, ctx=ctx)
        t0 = time.perf_counter()
        want = R.displacement_hist(x[:nf].cpu().numpy(), box[:nf], off, small, BIN, N_BINS)
        srec["cpu_numpy_one_core"] = {"frames": nf, "ms": (time.perf_counter() - t0) * 1e3,
                                      "equal_to_gpu": bool(np.array_equal(got[0], want[0]) and got[4] == want[4]
                                                           and np.array_equal(got[1], want[1]))}
        rec["shapes"].append(srec)
        del x, xu
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
