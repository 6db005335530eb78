#!/usr/bin/env python
"""
tools/bench_einstein.py — the two kernels of the Einstein-Helfand conductivity (csrc/collective.hip) on device-resident
inputs, timed with the library's own event timer (all launches of a call under one timer) after a warm-up call.

mdhip_cross_msd on synthetic collective series [G,3,n], n = 10 000 and 100 000, G = 1, 3, 8, max_lag = n // 2: the rate of
its fused multiply-adds (3 G (G + 1) / 2 per window position, sum_k (n - k) positions) and of all its FP64 operations
(3 G subtractions per position more), next to the multiply-add rate of the direct correlation kernel
(backend.xcorr, method XCORR_DIRECT, one series of the same n and the same lags) in the same run.
mdhip_collective_displacement on a block [F,3,M] of configuration C4's size (50 000 entities x 5 000 frames, three
groups), with and without the per-entity output: bytes of the trajectory per second, next to one read at the HBM rate
profiles/r05_ubench_hbm.txt measured for a flat streaming read (7.2 TB/s).
Writes the table to profiles/einstein_bench.txt.

    python tools/bench_einstein.py [--reps 5] [--n 10000,100000] [--groups 1,3,8] [--block 50000x5000] [--out FILE]
"""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

HBM_BYTES_PER_S = 7.2e12  # profiles/r05_ubench_hbm.txt, flat 8 KB per block


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
    ap.add_argument("--n", default="10000,100000")
    ap.add_argument("--groups", default="1,3,8")
    ap.add_argument("--block", default="50000x5000")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "einstein_bench.txt"))
    a = ap.parse_args()
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    lines = ["device: %s   reps: %d (median kernel ms of the library's event timer, after a warm-up call)" % (ctx.name, a.reps),
             "", "mdhip_cross_msd (cross_msd_kernel) against xcorr_direct_kernel, max_lag = n // 2",
             "%8s %3s %5s %9s %10s %12s %12s %10s" % ("n", "G", "abs", "launches", "kernel ms", "TFMA/s", "FP64 Top/s",
                                                      "vs xcorr")]
    for n in (int(v) for v in a.n.split(",")):
        max_lag = n // 2
        positions = float(sum(n - k for k in range(max_lag + 1)))
        g = torch.Generator(device="cuda").manual_seed(n)
        series = torch.randn((1, n), generator=g, device=dev, dtype=torch.float64).cumsum_(dim=1)
        lags = torch.empty((1, max_lag + 1), dtype=torch.float64, device=dev)
        x_ms, _, _ = timed(ctx, lambda: B.xcorr(series, method=B.XCORR_DIRECT, n_lags=max_lag + 1, out=lags, ctx=ctx),
                           a.reps)
        x_rate = positions / (x_ms * 1e-3) / 1e12
        lines.append("%8d %3s %5s %9d %10.3f %12.2f %12.2f %10s" % (n, "-", "-", 1, x_ms, x_rate, x_rate, "xcorr"))
        for G in (int(v) for v in a.groups.split(",")):
            P = torch.randn((G, 3, n), generator=g, device=dev, dtype=torch.float64).cumsum_(dim=2)
            out = torch.empty((max_lag + 1, G, G), dtype=torch.float64, device=dev)
            ab = torch.empty((max_lag + 1, G, G), dtype=torch.float64, device=dev)
            for with_abs in (False, True):
                ms, _, launches = timed(ctx, lambda: B.cross_msd(P, max_lag, out=out, abs_out=ab if with_abs else None,
                                                                 ctx=ctx), a.reps)
                fma = positions * 3 * G * (G + 1) / 2 * (2 if with_abs else 1)
                ops = fma + positions * 3 * G
                lines.append("%8d %3d %5s %9d %10.3f %12.2f %12.2f %10.2f" % (
                    n, G, "yes" if with_abs else "no", launches, ms, fma / (ms * 1e-3) / 1e12, ops / (ms * 1e-3) / 1e12,
                    fma / (ms * 1e-3) / 1e12 / x_rate))
            del P, out, ab
        del series, lags
    M, F = (int(v) for v in a.block.split("x"))
    g = torch.Generator(device="cuda").manual_seed(M)
    r = torch.randn((F, 3, M), generator=g, device=dev, dtype=torch.float64)
    w = np.where(np.arange(M) % 2 == 0, 1.0, -1.0) * 1.602e-19
    off = np.array([0, M // 3, 2 * M // 3, M], dtype=np.int64)
    P = torch.empty((3, 3, F), dtype=torch.float64, device=dev)
    once = F * 3 * M * 8
    lines += ["", "mdhip_collective_displacement (collective_kernel), %d entities x %d frames, 3 groups: %.2f GB, one read at "
              "%.1f TB/s = %.3f ms" % (M, F, once / 1e9, HBM_BYTES_PER_S / 1e12, once / HBM_BYTES_PER_S * 1e3),
              "%22s %10s %14s %16s" % ("per-entity output", "kernel ms", "read TB/s", "kernel / one read")]
    ms, _, _ = timed(ctx, lambda: B.collective_displacement(r, w, off, scale=1e-10, out=P, ctx=ctx), a.reps)
    lines.append("%22s %10.3f %14.2f %16.2f" % ("no", ms, once / (ms * 1e-3) / 1e12, ms / (once / HBM_BYTES_PER_S * 1e3)))
    wt = torch.empty((F, 3, M), dtype=torch.float64, device=dev)
    ms, _, _ = timed(ctx, lambda: B.collective_displacement(r, w, off, scale=1e-10, out=P, weighted=wt, ctx=ctx), a.reps)
    lines.append("%22s %10.3f %14.2f %16.2f" % ("yes (as much written)", ms, once / (ms * 1e-3) / 1e12,
                                                 ms / (once / HBM_BYTES_PER_S * 1e3)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
