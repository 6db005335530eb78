#!/usr/bin/env python
"""
tools/bench_dihedrals.py — mdhip_dihedral_angles (csrc/dihedrals.hip) on device-resident frames at a production-like
size (1 000 frames x 10 000 molecules of 10 atoms, four quadruples pooled into one histogram row of 360 bins, wrapped
coordinates), timed with the library's own event timer (all launches of a call under one timer): (a) histogram only,
(b) histogram and the series U. In the same process and alternating with them, rep by rep, after one warm-up round:
mdhip_axis_vectors with four jobs over the same molecules whose terms name the same atoms (apart from the third
component of U it moves the same bytes; it also reads the molecule's first atom in every job), and one
device-to-device copy of the coordinates (torch, device events: one read AND one write of them). Two more points say
where the time goes: the series without a histogram ((b) minus this is binning and the LDS atomics), and the first
quadruple alone (the same lines from HBM, a quarter of the load instructions).

Reported per kernel: median, best and worst of the reps, the bytes it has to move (one read of the trajectory — the four
quadruples name all ten atoms — plus U when written) and that over the HBM streaming rate of MI355X_MICROARCH.md
(6.29 TB/s measured float4 copy): `measured` are times, `modelled` are bytes over that rate. Recorded, not gated.
Writes profiles/dihedral_bench.json.

    python tools/bench_dihedrals.py [--reps 7] [--mols 10000] [--frames 1000] [--bins 360] [--out FILE]
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
PER = 10
QUADS = [(0, 1, 2, 3), (2, 3, 4, 5), (4, 5, 6, 7), (6, 7, 8, 9)]


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "best_ms": float(ms.min()), "worst_ms": float(ms.max()), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mols", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--bins", type=int, default=360)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "dihedral_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    M, F, J = a.mols, a.frames, len(QUADS)
    g = torch.Generator(device="cuda").manual_seed(M)
    # chains with bonds about 1.5 long anywhere in a box of 60, wrapped atom by atom
    L = 60.0
    x = torch.rand((F, 3, M, 1), generator=g, device=dev, dtype=torch.float64) * L
    x = x + torch.cumsum(0.9 * torch.randn((F, 3, M, PER), generator=g, device=dev, dtype=torch.float64), dim=3)
    x = torch.remainder(x, L).reshape(F, 3, M * PER).contiguous()
    box = np.full((F, 3), L)
    jobs = ([0] * J, [M] * J, [PER] * J)
    rows = [0] * J
    terms = [[(k, w) for k, w in zip(q, (-1.0, 1.0, 0.5, -0.5)) if k > 0] for q in QUADS]
    U = torch.empty((J * M, 3, F), dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def hist_only():
        h, _, d = B.dihedral_angles(x, box, *jobs, QUADS, job_row=rows, n_bins=a.bins, ctx=ctx)
        return ctx.last_kernel_ms()[0], h, d

    def with_series():
        h, _, d = B.dihedral_angles(x, box, *jobs, QUADS, job_row=rows, n_bins=a.bins, out=U, ctx=ctx)
        return ctx.last_kernel_ms()[0], h, d

    def series_only():                       # no histogram: what binning and the LDS atomics cost is (b) minus this
        _, _, d = B.dihedral_angles(x, box, *jobs, QUADS, out=U, ctx=ctx)
        return ctx.last_kernel_ms()[0], None, d

    def one_job():                           # the first quadruple alone: the same lines from HBM, a quarter of the loads
        h, _, d = B.dihedral_angles(x, box, [0], [M], [PER], QUADS[:1], n_bins=a.bins, ctx=ctx)
        return ctx.last_kernel_ms()[0], h, d

    def axis():
        _, d = B.axis_vectors(x, box, *jobs, terms, out=U, ctx=ctx)
        return ctx.last_kernel_ms()[0], None, d

    def copy():
        torch.cuda.synchronize(dev)
        ev0.record()
        y.copy_(x)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1), None, None

    calls = {"dihedral_hist_only": hist_only, "dihedral_hist_and_series": with_series, "axis_vectors_same_jobs": axis,
             "d2d_copy_of_the_coordinates": copy, "dihedral_series_only": series_only,
             "dihedral_hist_only_one_job": one_job}
    times = {k: [] for k in calls}
    last = {}
    for rep in range(a.reps + 1):            # the first round warms every shape up
        for name, call in calls.items():
            ms, h, d = call()
            last[name] = (h, d)
            if rep:
                times[name].append(ms)
    read_b, u_b = F * 3 * M * PER * 8, J * M * 3 * F * 8
    moved = {"dihedral_hist_only": read_b, "dihedral_hist_and_series": read_b + u_b,
             "axis_vectors_same_jobs": read_b + u_b, "d2d_copy_of_the_coordinates": 2 * read_b,
             "dihedral_series_only": read_b + u_b, "dihedral_hist_only_one_job": read_b}
    res = {"device": ctx.name, "molecules": M, "atoms_per_molecule": PER, "frames": F, "jobs": J, "quadruples": QUADS,
           "n_bins": a.bins, "hbm_bytes_per_s_modelled_from": "MI355X_MICROARCH.md, measured float4 copy",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "trajectory_bytes": read_b, "series_bytes": u_b,
           "one_read_of_the_trajectory_ms_modelled": read_b / HBM_BYTES_PER_S * 1e3}
    for name in calls:
        s = stats(times[name])
        s["kind"] = "measured"
        s["bytes_to_move"] = moved[name]
        s["bytes_over_hbm_rate_ms_modelled"] = moved[name] / HBM_BYTES_PER_S * 1e3
        s["median_over_modelled"] = s["median_ms"] / s["bytes_over_hbm_rate_ms_modelled"]
        s["moved_bytes_per_s"] = moved[name] / (s["median_ms"] * 1e-3)
        res[name] = s
    h, d = last["dihedral_hist_and_series"]
    assert np.array_equal(h, last["dihedral_hist_only"][0]) and int(h.sum()) + int(d.sum()) == J * M * F
    res["counted"], res["degenerate"] = int(h.sum()), int(d.sum())
    res["hist_only_over_axis_vectors"] = res["dihedral_hist_only"]["median_ms"] / res["axis_vectors_same_jobs"]["median_ms"]
    res["hist_and_series_over_axis_vectors"] = (res["dihedral_hist_and_series"]["median_ms"]
                                                / res["axis_vectors_same_jobs"]["median_ms"])
    res["hist_only_over_d2d_copy"] = (res["dihedral_hist_only"]["median_ms"]
                                      / res["d2d_copy_of_the_coordinates"]["median_ms"])
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
