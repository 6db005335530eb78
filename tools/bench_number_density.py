#!/usr/bin/env python
"""
tools/bench_number_density.py — the axis-profile kernel (csrc/density.hip) on device-resident frames: 100 000 atoms x
1 000 frames (the split path: two launches per group of frames) and 10 000 atoms x 10 000 frames (one workgroup per
frame), codes shared by the frames, positive reference mode and the profile mode. Times every call with the library's
own event timer (all launches of the call under one timer) after a warm-up call and prices it against ONE read of the
algorithmic bytes — 8 B of coordinate per atom per frame, the 2 B codes once per call (they are shared and stay in
cache) — at the HBM rate profiles/r05_ubench_hbm.txt measured for a flat streaming read (7.2 TB/s). The CPU sample is
the numpy restatement (tests/number_density_ref.py) on one core over a few frames. Writes
profiles/number_density_bench.json.

    python tools/bench_number_density.py [--reps 10] [--shapes 100000x1000,10000x10000]
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

import number_density_ref as R  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

HBM_BYTES_PER_S = 7.2e12  # profiles/r05_ubench_hbm.txt, flat 8 KB per block
BIN, DIST, CPU_FRAMES = 0.25, 12.0, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="100000x1000,10000x10000")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "number_density_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    rec = {"device": ctx.name, "bin_size": BIN, "dist": DIST, "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": []}
    n_bins = int(DIST / BIN)
    for shape in a.shapes.split(","):
        n, frames = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.rand((frames, n), generator=g, device="cuda", dtype=torch.float64) * 30.0
        n_surf = n // 10
        x[:, :n_surf] = 1.0 + 4.0 * torch.rand((frames, n_surf), generator=g, device="cuda", dtype=torch.float64)
        row = np.arange(n) % 2
        row[:n_surf] = -1
        codes = B.axis_profile_codes(row, np.arange(n) < n_surf)
        bytes_once = frames * n * 8 + n * 2
        roof_ms = bytes_once / HBM_BYTES_PER_S * 1e3
        srec = {"atoms": n, "frames": frames, "algorithmic_bytes": bytes_once, "roof_ms": roof_ms}
        for name, mode, d in (("ref_pos", B.AP_REF_POS, DIST), ("profile", B.AP_PROFILE, -5.0)):
            ms, wall = [], []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                counts, _, _ = B.axis_profile(x, codes, mode, BIN, d, n_bins, 2, origin="hi", ctx=ctx)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(ctx.last_kernel_ms()[0])
            ms, wall = np.array(ms[1:]), np.array(wall[1:])
            med = float(np.median(ms))
            srec[name] = {"kernel": ctx.last_kernel_name(), "launches": ctx.last_kernel_ms()[1], "median_ms": med,
                          "best_ms": float(ms.min()), "wall_median_ms": float(np.median(wall)),
                          "atoms_per_s": frames * n / (med * 1e-3), "frac_of_hbm_roof": roof_ms / med,
                          "binned": int(counts.sum(dtype=np.int64)), "reps": a.reps}
        xs = x[:CPU_FRAMES].cpu().numpy()
        t0 = time.perf_counter()
        want = R.axis_profile(xs, codes, R.REF_POS, BIN, DIST, n_bins, 2)
        cpu_s = time.perf_counter() - t0
        got = B.axis_profile(x[:CPU_FRAMES].contiguous(), codes, B.AP_REF_POS, BIN, DIST, n_bins, 2, ctx=ctx)
        srec["cpu_numpy_one_core"] = {"frames": CPU_FRAMES, "ms_per_frame": cpu_s * 1e3 / CPU_FRAMES,
                                      "atoms_per_s": CPU_FRAMES * n / cpu_s,
                                      "equal_to_gpu": bool(np.array_equal(got[0], want[0]))}
        rec["shapes"].append(srec)
        del x
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
