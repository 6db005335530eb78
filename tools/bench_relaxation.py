#!/usr/bin/env python
"""
tools/bench_relaxation.py — mdhip_self_relaxation (csrc/relaxation.hip) on device-resident frames at a production-like
shape (1 000 entities x 10 000 frames, max_lag 5 000, every frame an origin, unwrapped) with n_q = 0, 1 and 4 wave
numbers, and mdhip_orient_corr — the closest existing all-lags direct sweep (csrc/lag_tiles.h organisation) — at the
same series count, n and max_lag, in the same process with the calls alternating. Timed with the library's own event
timer (all launches of a call under one timer) after one warm-up round.

Reported: ms and ns per (cell, entity) — a cell is one (origin, lag), so there are entities * sum_k (F - k) of them —
for every variant, and their ratios to orient_corr per window position. Recorded, not gated: the ratio to orient_corr
is the number a later performance change starts from. Writes profiles/relaxation_bench.json.

    python tools/bench_relaxation.py [--reps 3] [--entities 1000] [--frames 10000] [--max-lag 5000] [--out FILE]
"""

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

FP64_FMA_PEAK_FLOPS = 78.6e12  # half the FP32 vector peak of the chip table (157.3 TFLOP/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--entities", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--max-lag", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "relaxation_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    E, F, K = a.entities, a.frames, a.max_lag
    g = torch.Generator(device="cuda").manual_seed(E)
    # a random walk of 0.05 per frame and axis: |dr| reaches about 6 at the largest lag, q |dr| about 12
    r = (0.05 * torch.randn((F, 3, E), generator=g, device=dev, dtype=torch.float64)).cumsum_(dim=0).contiguous()
    U = torch.randn((E, 3, F), generator=g, device=dev, dtype=torch.float64)
    U = (U / U.norm(dim=1, keepdim=True)).contiguous()
    off = np.array([0, E], dtype=np.int64)
    sums = torch.empty((K + 1, 1, 2), dtype=torch.float64, device=dev)
    cells = float(sum(F - k for k in range(K + 1)))
    work = cells * E
    qs = {0: None, 1: [1.0], 4: [0.5, 1.0, 1.5, 2.0]}
    last = {}

    def relax(n_q):
        last[n_q] = B.self_relaxation(r, None, off, K, 1, 1.0, qs[n_q], ctx=ctx)

    calls = [("self_relaxation_nq0", lambda: relax(0)), ("self_relaxation_nq1", lambda: relax(1)),
             ("self_relaxation_nq4", lambda: relax(4)), ("orient_corr", lambda: B.orient_corr(U, off, K, out=sums, ctx=ctx))]
    ms = {name: [] for name, _ in calls}
    launches = {}
    for rep in range(a.reps + 1):       # round 0 is the warm-up; the variants alternate inside every round
        for name, call in calls:
            call()
            t, n = ctx.last_kernel_ms()
            launches[name] = n
            if rep:
                ms[name].append(t)
    res = {"device": ctx.name, "entities": E, "frames": F, "max_lag": K, "origin_stride": 1, "reps": a.reps,
           "cells": cells, "cell_entities": work, "fp64_fma_peak_flops": FP64_FMA_PEAK_FLOPS}
    for name, _ in calls:
        med = float(np.median(ms[name]))
        res[name] = {"kernel_median_ms": med, "kernel_best_ms": float(np.min(ms[name])), "launches": launches[name],
                     "ns_per_cell_entity": med * 1e6 / work, "cell_entities_per_s": work / (med * 1e-3)}
    base = res["orient_corr"]["ns_per_cell_entity"]
    for n_q in qs:
        res["self_relaxation_nq%d" % n_q]["over_orient_corr"] = res["self_relaxation_nq%d" % n_q]["ns_per_cell_entity"] / base
    per_q = (res["self_relaxation_nq4"]["kernel_median_ms"] - res["self_relaxation_nq1"]["kernel_median_ms"]) / 3.0
    res["ms_per_extra_wave_number"] = per_q
    res["ns_per_sinc"] = per_q * 1e6 / work
    origins, c1, c2, fs, bad = last[4]
    res["checks"] = {"fs_at_lag_0_is_exact": bool(np.all(fs[0, 0] == F * E * (1 << 32))),
                     "count1_at_lag_0": int(c1[0, 0]), "nonfinite": int(bad.sum()),
                     "Q_at_max_lag": float(c1[K, 0]) / float(origins[K] * E),
                     "Fs_q1_at_max_lag": float(fs[K, 0, 1]) / float(1 << 32) / float(origins[K] * E)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
