#!/usr/bin/env python
"""
tools/bench_shape.py — mdhip_mol_shape (csrc/mol_shape.hip) on device-resident frames, one process, for molecules of 3,
16 and 100 atoms (about 300 000 atoms a frame, 300 frames, wrapped coordinates, chain mode), timed with the library's own
event timer (all launches of a call under one timer): (a) the histograms alone — no principal moments, nothing written
per molecule —, (b) with the per-molecule values written to a device tensor, (c) with the totals as well. In the same
process and alternating with them, rep by rep, after one warm-up round: mdhip_segment_com over the same molecules — the
staged sibling that reads the same bytes and writes three values per molecule and frame.

Reported per call: median, best and worst of the reps, the bytes it has to move (one read of the trajectory, plus what
it writes) and that over the HBM streaming rate of MI355X_MICROARCH.md (6.29 TB/s measured float4 copy): `measured` are
times, `modelled` are bytes over that rate. Recorded, not gated. Writes profiles/shape_bench.json.

    python tools/bench_shape.py [--reps 7] [--atoms 300000] [--frames 300] [--out FILE]
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

HBM_BYTES_PER_S = 6.29e12  # MI355X_MICROARCH.md: measured float4 copy
LENGTHS = (3, 16, 100)


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "best_ms": float(ms.min()), "worst_ms": float(ms.max()), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=300000)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "shape_bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    F, L = a.frames, 60.0
    box = np.full((F, 3), L)
    res = {"device": ctx.name, "frames": F, "hbm_bytes_per_s_modelled_from": "MI355X_MICROARCH.md, measured float4 copy",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": {}}
    for per in LENGTHS:
        M = a.atoms // per
        g = torch.Generator(device="cuda").manual_seed(per)
        # chains with bonds about 1.5 long anywhere in a box of 60, wrapped atom by atom
        x = torch.rand((F, 3, M, 1), generator=g, device=dev, dtype=torch.float64) * L
        x = x + torch.cumsum(0.9 * torch.randn((F, 3, M, per), generator=g, device=dev, dtype=torch.float64), dim=3)
        x = torch.remainder(x, L).reshape(F, 3, M * per).contiguous()
        w = np.linspace(1.0, 16.0, per)
        jobs = ([0], [M], [per], [w])
        r_max = max(8.0, 2.0 * per ** 0.5 * 1.6)
        bins = dict(bin_size=0.05, n_bins=int(r_max / 0.05), n_kbins=50)
        values = torch.empty((F, 6, M), dtype=torch.float64, device=dev)
        com = torch.empty((F, 3, M), dtype=torch.float64, device=dev)
        mass, seg_off = np.tile(w, M), np.arange(M + 1, dtype=np.int64) * per

        def hist_only():
            got = B.mol_shape(x, box, *jobs, totals=False, ctx=ctx, **bins)
            return ctx.last_kernel_ms()[0], got

        def with_values():
            got = B.mol_shape(x, box, *jobs, totals=False, out=values, ctx=ctx, **bins)
            return ctx.last_kernel_ms()[0], got

        def with_totals():
            got = B.mol_shape(x, box, *jobs, totals=True, out=values, ctx=ctx, **bins)
            return ctx.last_kernel_ms()[0], got

        def segment_com():
            B.segment_com(x, mass, seg_off, out=com, ctx=ctx)
            return ctx.last_kernel_ms()[0], None

        calls = {"shape_hist_only": hist_only, "shape_with_per_mol": with_values, "shape_with_per_mol_and_totals": with_totals,
                 "segment_com_same_molecules": segment_com}
        times = {k: [] for k in calls}
        last = {}
        for rep in range(a.reps + 1):            # the first round warms every shape up
            for name, call in calls.items():
                ms, got = call()
                last[name] = got
                if rep:
                    times[name].append(ms)
        read_b = F * 3 * M * per * 8
        moved = {"shape_hist_only": read_b, "shape_with_per_mol": read_b + F * 6 * M * 8,
                 "shape_with_per_mol_and_totals": read_b + 2 * F * 7 * M * 8, "segment_com_same_molecules": read_b + F * 3 * M * 8}
        shape = {"molecules": M, "atoms_per_molecule": per, "trajectory_bytes": read_b, "n_bins": bins["n_bins"],
                 "one_read_of_the_trajectory_ms_modelled": read_b / HBM_BYTES_PER_S * 1e3}
        for name in calls:
            s = stats(times[name])
            s["kind"] = "measured"
            s["bytes_to_move"] = moved[name]
            s["bytes_over_hbm_rate_ms_modelled"] = moved[name] / HBM_BYTES_PER_S * 1e3
            s["median_over_modelled"] = s["median_ms"] / s["bytes_over_hbm_rate_ms_modelled"]
            s["median_over_one_read"] = s["median_ms"] / shape["one_read_of_the_trajectory_ms_modelled"]
            shape[name] = s
        for name in ("shape_hist_only", "shape_with_per_mol", "shape_with_per_mol_and_totals"):
            shape[name + "_over_segment_com"] = shape[name]["median_ms"] / shape["segment_com_same_molecules"]["median_ms"]
        h = last["shape_hist_only"]
        assert all(np.array_equal(h[k], last["shape_with_per_mol_and_totals"][k]) for k in ("hist_rg", "hist_ee", "hist_k"))
        assert int(h["hist_rg"].sum()) + int(h["beyond"][0, 0]) == M * F
        shape["beyond_rg"], shape["beyond_ree"] = int(h["beyond"][0, 0]), int(h["beyond"][0, 1])
        res["shapes"][str(per)] = shape
        del x, values, com
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
