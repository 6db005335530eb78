#!/usr/bin/env python
"""
tools/bench_hydration.py — the hydration search (csrc/hydration.hip) on a synthetic ion / 3-site-water trajectory:
30 000 waters, 540 cations, 1 000 frames, device-resident coordinates, r_cut 3.5. Times both modes with the library's
own event timer (every launch of one call under one timer) and prices them against the FP64 VALU roof: 15 unfused
f64 operations per (cation, water) test at 39.3e12 op/s. Writes profiles/hydration_bench.json.

    python tools/bench_hydration.py [--frames 1000] [--reps 10]
"""

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

OPS_PER_TEST, VALU_OPS = 15, 39.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--waters", type=int, default=30000)
    ap.add_argument("--cations", type=int, default=540)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "hydration_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    n = a.cations + 3 * a.waters
    L = (a.waters / 0.0334) ** (1.0 / 3.0)  # liquid-water density
    g = torch.Generator(device="cuda").manual_seed(0)
    xyz = torch.rand((a.frames, 3, n), generator=g, device="cuda", dtype=torch.float64) * L
    o = a.cations + 3 * np.arange(a.waters)
    ot = torch.as_tensor(o, device="cuda")
    for h in (1, 2):
        xyz[:, :, ot + h] = xyz[:, :, ot] + 0.6 * torch.randn((a.frames, 3, a.waters), generator=g, device="cuda",
                                                              dtype=torch.float64)
    box = np.full((a.frames, 3), L)
    ions = np.arange(a.cations)
    rec = {"frames": a.frames, "waters": a.waters, "cations": a.cations, "box": L, "r_cut": 3.5,
           "tests": a.frames * a.waters * a.cations, "device": ctx.name}
    roof_ms = rec["tests"] * OPS_PER_TEST / VALU_OPS * 1e3
    rec["roof_ms"] = roof_ms
    for mode in ("counts", "list"):
        ms = []
        for _ in range(a.reps + 1):
            if mode == "counts":
                B.hydration_counts(xyz, box, ions, o, 3.5 ** 2, -0.72, 0.02, 100, ctx=ctx)
            else:
                B.hydration_cosines(xyz, box, ions, o, 3.5 ** 2, cap=32, ctx=ctx)
            ms.append(ctx.last_kernel_ms()[0])  # (ms, launches)
        ms = np.array(ms[1:])
        rec[mode] = {"median_ms": float(np.median(ms)), "best_ms": float(ms.min()),
                     "median_frac_of_roof": roof_ms / float(np.median(ms)), "reps": a.reps}
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
