#!/usr/bin/env python
"""
tools/bench_velocity.py — mdhip_velocity_spectrum (csrc/velocity_spectrum.hip) on device-resident velocities at two sizes
(100 000 entities x 2 000 frames and 50 000 x 10 000, three interleaved groups, every lag), timed with the library's own
event timer (all launches of a call under one timer), and, in the same process with the calls alternating after a
warm-up of each, mdhip_lag_msd forced onto the batched transforms (lag_variant 4) at the same shape, groups and padded
length: it runs the same forward transforms plus the S1 sums, the bound and the centring pass, so the new call is
expected to be no slower. Reported per shape: median and best of both, the run-to-run spread (max - min over the median)
of both, their ratio; the time one read plus one write of the trajectory takes at the device-to-device copy rate
measured in this process — the floor of the gather pass. Recorded, not gated. Writes profiles/velocity_bench.json.

    python tools/bench_velocity.py [--reps 5] [--shapes 100000x2000,50000x10000] [--out FILE]
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


def copy_rate(dev, n_bytes=1 << 30, reps=5):
    """Bytes moved per second (read + write) by a device-to-device copy of n_bytes, best of `reps`."""
    src = torch.empty(n_bytes // 8, dtype=torch.float64, device=dev).normal_()
    dst = torch.empty_like(src)
    best = float("inf")
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return 2 * n_bytes / (best * 1e-3)


def stats(ms):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"median_ms": med, "best_ms": float(ms.min()), "worst_ms": float(ms.max()),
            "spread_over_median": float((ms.max() - ms.min()) / med)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="100000x2000,50000x10000")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "velocity_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    rate = copy_rate(dev)
    res = {"device": ctx.name, "reps": a.reps, "groups": 3, "copy_bytes_per_s": rate, "shapes": []}
    for shape in a.shapes.split(","):
        E, F = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(E + F)
        v = torch.randn((F, 3, E), generator=g, device=dev, dtype=torch.float64)
        interleaved = (np.arange(E) % 3).astype(np.int32)                # types inside molecules
        off = np.array([0, E // 3, 2 * (E // 3), E], dtype=np.int64)     # the MSD's contiguous groups, same sizes (+-1)
        K, L = F - 1, B.spectrum_length(F)
        sums = torch.empty((K + 1, 3, 4), dtype=torch.float64, device=dev)
        msd = torch.empty((K + 1, 3, 4), dtype=torch.float64, device=dev)

        def new():
            B.velocity_spectrum(v, interleaved, K, L=L, out=sums, ctx=ctx)
            return ctx.last_kernel_ms()[0]

        def old():
            ctx.set_option("lag_variant", 4)
            try:
                B.lag_msd(v, K, off, out=msd, ctx=ctx)
            finally:
                ctx.set_option("lag_variant", 3)
            return ctx.last_kernel_ms()[0]

        new(), old()                                                      # warm-up of each
        kernel = {"velocity_spectrum": None, "lag_msd_batched": None}
        t_new, t_old = [], []
        for _ in range(a.reps):                                           # alternating
            t_new.append(new())
            kernel["velocity_spectrum"] = ctx.last_kernel_name()
            t_old.append(old())
            kernel["lag_msd_batched"] = ctx.last_kernel_name()
        s_new, s_old = stats(t_new), stats(t_old)
        traffic = 2 * F * 3 * E * 8
        res["shapes"].append({
            "entities": E, "frames": F, "max_lag": K, "padded_length": L, "kernels": kernel,
            "velocity_spectrum": s_new, "lag_msd_batched": s_old,
            "ratio_new_over_msd": s_new["median_ms"] / s_old["median_ms"],
            "ratio_spread": s_new["spread_over_median"] + s_old["spread_over_median"],
            "trajectory_read_plus_write_bytes": traffic, "gather_floor_ms": traffic / rate * 1e3,
            "floor_over_call": traffic / rate * 1e3 / s_new["median_ms"]})
        del v, sums, msd
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
