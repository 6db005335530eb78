#!/usr/bin/env python
"""
tools/bench_reorientation.py — the two kernels of `Reorientation` (csrc/reorient.hip) on device-resident inputs at one
plausible size (4 096 molecules of three atoms, 5 000 frames, max_lag 2 500), timed with the library's own event timer
(all launches of a call under one timer) after a warm-up call, and mdhip_cross_msd with one group at the same n and
max_lag in the same process.

Reported: window positions per second of mdhip_orient_corr (n_series * sum_k (n - k) positions) and of mdhip_cross_msd
(sum_k (n - k)); the FP64 rate of orient_corr — five FP64 instructions per position (a product, two multiply-adds for
c, an addition and a multiply-add for the two sums), eight floating-point operations — against the FP64 vector
multiply-add peak (78.6 TFLOP/s: half the FP32 vector rate of MI355X_MICROARCH.md's chip table, one instruction per
two operations); the bytes of the trajectory mdhip_axis_vectors reads per second against one read at the measured HBM
streaming rate. Recorded, not gated. Writes profiles/reorientation_bench.json.

    python tools/bench_reorientation.py [--reps 5] [--mols 4096] [--frames 5000] [--max-lag 2500] [--out FILE]
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

HBM_BYTES_PER_S = 6.29e12      # MI355X_MICROARCH.md: measured float4 copy
FP64_FMA_PEAK_FLOPS = 78.6e12  # half the FP32 vector peak (157.3 TFLOP/s)


def timed(ctx, call, reps):
    """(median kernel ms, best, launches) of `reps` calls after one warm-up call."""
    ms = []
    for _ in range(reps + 1):
        call()
        ms.append(ctx.last_kernel_ms()[0])
    ms = np.array(ms[1:])
    return float(np.median(ms)), float(ms.min()), ctx.last_kernel_ms()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mols", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--max-lag", type=int, default=2500)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "reorientation_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    M, F, K, per = a.mols, a.frames, a.max_lag, 3
    g = torch.Generator(device="cuda").manual_seed(M)
    # molecules of three atoms about 1 wide anywhere in a box of 40: the bond 2 -> 3 names every atom of the molecule
    L = 40.0
    centre = torch.rand((F, 3, M, 1), generator=g, device=dev, dtype=torch.float64) * L
    x = torch.remainder(centre + 0.6 * torch.randn((F, 3, M, per), generator=g, device=dev, dtype=torch.float64), L)
    x = x.reshape(F, 3, M * per).contiguous()
    del centre
    box = np.full((F, 3), L)
    U = torch.empty((M, 3, F), dtype=torch.float64, device=dev)
    jobs = ([0], [M], [per], [[(1, -1.0), (2, 1.0)]])
    res = {"device": ctx.name, "molecules": M, "atoms_per_molecule": per, "frames": F, "max_lag": K, "reps": a.reps,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "fp64_fma_peak_flops": FP64_FMA_PEAK_FLOPS}

    deg = []
    ms, best, launches = timed(ctx, lambda: deg.append(B.axis_vectors(x, box, *jobs, out=U, ctx=ctx)[1]), a.reps)
    read_b, write_b = F * 3 * M * per * 8, M * 3 * F * 8
    res["axis_vectors"] = {
        "kernel_median_ms": ms, "kernel_best_ms": best, "launches": launches, "degenerate": int(deg[-1].sum()),
        "trajectory_bytes": read_b, "written_bytes": write_b, "read_bytes_per_s": read_b / (ms * 1e-3),
        "moved_bytes_per_s": (read_b + write_b) / (ms * 1e-3), "one_read_ms": read_b / HBM_BYTES_PER_S * 1e3,
        "kernel_over_one_read": ms / (read_b / HBM_BYTES_PER_S * 1e3),
        "kernel_over_read_and_write": ms / ((read_b + write_b) / HBM_BYTES_PER_S * 1e3)}
    del x

    off = np.array([0, M], dtype=np.int64)
    sums = torch.empty((K + 1, 1, 2), dtype=torch.float64, device=dev)
    per_series = float(sum(F - k for k in range(K + 1)))
    ms, best, launches = timed(ctx, lambda: B.orient_corr(U, off, K, out=sums, ctx=ctx), a.reps)
    pos = per_series * M
    res["orient_corr"] = {
        "kernel_median_ms": ms, "kernel_best_ms": best, "launches": launches, "window_positions": pos,
        "window_positions_per_s": pos / (ms * 1e-3), "fp64_instructions_per_s": 5 * pos / (ms * 1e-3),
        "flops": 8 * pos / (ms * 1e-3), "flops_over_fma_peak": 8 * pos / (ms * 1e-3) / FP64_FMA_PEAK_FLOPS,
        "instructions_over_fma_issue_peak": 5 * pos / (ms * 1e-3) / (FP64_FMA_PEAK_FLOPS / 2),
        "c1_at_lag_0": float(sums[0, 0, 0].item() / (F * M))}

    P = torch.randn((1, 3, F), generator=g, device=dev, dtype=torch.float64).cumsum_(dim=2)
    out = torch.empty((K + 1, 1, 1), dtype=torch.float64, device=dev)
    ms_c, best_c, launches_c = timed(ctx, lambda: B.cross_msd(P, K, out=out, ctx=ctx), a.reps)
    res["cross_msd_one_group"] = {
        "kernel_median_ms": ms_c, "kernel_best_ms": best_c, "launches": launches_c, "window_positions": per_series,
        "window_positions_per_s": per_series / (ms_c * 1e-3), "fp64_instructions_per_s": 6 * per_series / (ms_c * 1e-3)}
    ratio = res["orient_corr"]["window_positions_per_s"] / res["cross_msd_one_group"]["window_positions_per_s"]
    res["orient_over_cross_msd_per_position"] = ratio
    res["note"] = (
        "cross_msd with ONE group at this n is a grid of a few lag tiles x time slabs of a single series set: it "
        "measures launch-bound work on part of the chip, orient_corr the same organisation over %d series that fill "
        "it." % M if ratio >= 0.5 else
        "orient_corr runs below half of cross_msd's rate per window position: see DESIGN 4.13b for what bounds it")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
