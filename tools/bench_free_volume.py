#!/usr/bin/env python
"""
tools/bench_free_volume.py — mdhip_free_volume (csrc/free_volume.hip) on device-resident frames, one process, at a
workload-like size: 20 000 atoms in a box at liquid density (0.1 atoms per cubic Angstrom), a grid of 0.5 A spacing, 20
frames, three classes with Bondi-like radii, s_max = 4 A. Timed with the library's own event timer (all launches of a call
under one timer; the call's aux time is the pre-pass — bin, scan, scatter — of its first batch):
  (a) the histograms and n_free alone, (b) with the occupancy map as well, (c) with the field (s, nearest) written to
  device tensors.
In the same process and alternating with them, rep by rep, after one warm-up round:
  the brute-force organisation the tree has — the counts mode of the hydration search (shell_search.h: every tile of
  centres against every chunk of candidates) given as many centres as there are grid points and as many candidates as
  there are atoms, at r_cut = r_search, on --brute-frames frames, reported per frame;
  one device-to-device copy of a buffer of 256 MiB: the copy rate of this process, from which `one read of the
  coordinates` is modelled (bytes over that rate).
The candidates per point and the staged atoms per point are counted on the host for a sample of the points of frame 0.
`measured` are times, `modelled` are bytes or counts over a measured rate. Recorded, not gated — except that the cell
sweep must come out faster per frame than the brute sweep (it does at most 27 r_search^3 / V of its tests): the tool
says so and exits 1 otherwise. Writes profiles/free_volume_bench.json and prints the table of DESIGN 4.13g as markdown.

    python tools/bench_free_volume.py [--reps 7] [--atoms 20000] [--frames 20] [--brute-frames 2] [--out FILE]
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

DENSITY = 0.1       # atoms per cubic Angstrom
SPACING = 0.5
RADII = np.array([1.20, 1.70, 1.52])
S_MAX, BIN = 4.0, 0.05
MAX_NC, MARGIN = 64, 2.0 ** -20  # csrc/cell_plan.h


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "best_ms": float(ms.min()), "worst_ms": float(ms.max()), "reps": len(ms)}


def cells(L, r):
    need = r * (1.0 + MARGIN)
    return int(max(1, min(MAX_NC, np.floor(L / need))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=20000)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--brute-frames", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "free_volume_bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    F, N = a.frames, a.atoms
    L = float((N / DENSITY) ** (1.0 / 3.0))
    g = int(np.ceil(L / SPACING))
    G = g ** 3
    rng = np.random.default_rng(N)
    box = L + 0.05 * rng.random((F, 3))                       # NPT-like: a little different every frame
    x_host = rng.random((F, 3, N)) * box[:, :, None]
    cls = rng.integers(0, 3, size=N).astype(np.int32)
    edges = np.arange(int(round(S_MAX / BIN)) + 1) * BIN
    r_search = float(edges[-1] + RADII.max())
    x = torch.as_tensor(x_host, device=dev)
    s_out = torch.empty((F, g, g, g), dtype=torch.float64, device=dev)
    near_out = torch.empty((F, g, g, g), dtype=torch.int32, device=dev)
    nc = cells(L, r_search)

    # the brute sweep's input: the grid points as atoms 0 .. G-1, then `N` three-atom candidates (its candidates are water
    # molecules: the O and two more atoms, which only the cosine reads)
    Fb = min(a.brute_frames, F)
    pts = (np.arange(g) + 0.5) / g
    bx = np.empty((Fb, 3, G + 3 * N))
    for f in range(Fb):
        P = np.stack(np.meshgrid(pts * box[f, 0], pts * box[f, 1], pts * box[f, 2], indexing="ij")).reshape(3, G)
        mol = np.repeat(x_host[f], 3, axis=1) + np.tile(np.array([0.0, 0.6, -0.6]), N)[None, :]
        bx[f] = np.concatenate([P, mol], axis=1)
    brute_x = torch.as_tensor(bx, device=dev)
    del bx
    centres = np.arange(G, dtype=np.int32)
    waters = (G + 3 * np.arange(N)).astype(np.int32)

    buf = torch.empty(32 << 20, dtype=torch.float64, device=dev)  # 256 MiB
    dst = torch.empty_like(buf)

    def fv(**kw):
        got = B.free_volume(x, box, cls, RADII, (g, g, g), r_search, edges, (0.0, 0.5, 1.0), ctx=ctx, **kw)
        return ctx.last_kernel_ms()[0], ctx.last_aux_ms(), got

    def brute():
        n_water, _, _ = B.hydration_counts(brute_x, box[:Fb], centres, waters, r_search * r_search, 0.0, 0.05, 40, ctx=ctx)
        return ctx.last_kernel_ms()[0] / Fb, 0.0, n_water

    def copy():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(buf)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), 0.0, None

    calls = {"free_volume_hist_only": lambda: fv(), "free_volume_with_map": lambda: fv(want_map=True),
             "free_volume_with_field": lambda: fv(out=(s_out, near_out)), "brute_hydration_counts_per_frame": brute,
             "copy_256MiB": copy}
    times, aux, last = {k: [] for k in calls}, {k: [] for k in calls}, {}
    for rep in range(a.reps + 1):            # the first round warms everything up
        for name, call in calls.items():
            ms, pre, got = call()
            last[name] = got
            if rep:
                times[name].append(ms)
                aux[name].append(pre)
    copy_rate = 2 * buf.numel() * 8 / (np.median(times["copy_256MiB"]) * 1e-3)   # bytes moved (read + write) per second
    read_b = F * 3 * N * 8
    # the work counts, on a sample of frame 0
    sample = rng.choice(G, size=500, replace=False)
    P = np.stack(np.meshgrid(pts, pts, pts, indexing="ij")).reshape(3, G)[:, sample] * box[0][:, None]
    d = np.abs(P[:, :, None] - x_host[0][:, None, :])
    d = np.minimum(d, np.abs(d - box[0][:, None, None]))
    cand = float(((d * d).sum(axis=0) < r_search * r_search).sum(axis=1).mean())
    staged = 27.0 * (L / nc) ** 3 * DENSITY if nc >= 3 else float(N)
    res = {"device": ctx.name, "frames": F, "atoms": N, "box_edge_A": L, "grid": [g, g, g], "grid_points": G,
           "r_search_A": r_search, "cells_per_axis": nc, "brute_frames": Fb,
           "copy_rate_bytes_per_s_measured": copy_rate, "trajectory_bytes": read_b,
           "one_read_of_the_coordinates_ms_modelled": read_b / copy_rate * 1e3,
           "candidates_per_point_counted_on_a_sample": cand, "staged_atoms_per_point_modelled": staged,
           "brute_tests_per_point": float(N), "work_bound_27_r3_over_V": 27.0 * r_search ** 3 / L ** 3, "calls": {}}
    for name in calls:
        s = stats(times[name])
        s["kind"] = "measured"
        if name.startswith("free_volume"):
            s["per_frame_ms"] = s["median_ms"] / F
            s["pre_pass_ms_median"] = float(np.median(aux[name]))
            s["pre_pass_share"] = s["pre_pass_ms_median"] / s["median_ms"]
            s["median_over_one_read"] = s["median_ms"] / res["one_read_of_the_coordinates_ms_modelled"]
            s["point_atom_tests_per_s_modelled"] = staged * G * F / (s["median_ms"] * 1e-3)
        res["calls"][name] = s
    per_frame = res["calls"]["free_volume_hist_only"]["per_frame_ms"]
    brute_ms = res["calls"]["brute_hydration_counts_per_frame"]["median_ms"]
    res["brute_over_cells_per_frame"] = brute_ms / per_frame
    res["brute_point_centre_tests_per_s_modelled"] = float(N) * G / (brute_ms * 1e-3)
    h, m = last["free_volume_hist_only"], last["free_volume_with_map"]
    assert np.array_equal(h["hist"], m["hist"]) and np.array_equal(h["n_free"], m["n_free"])
    assert int(h["hist"].sum()) + int(h["occupied"].sum()) + h["beyond"] == F * G
    assert int(m["free_map"].sum()) == int(h["n_free"][:, 0].sum())
    res["ffv_probe_0"] = float(h["n_free"][:, 0].mean() / G)
    res["brute_mean_candidates_frame_0"] = float(last["brute_hydration_counts_per_frame"][0].mean())
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print("\n| call | median ms | best | worst | per frame ms | pre-pass share | x one read |\n|---|---|---|---|---|---|---|")
    for name, s in res["calls"].items():
        print("| %s | %.3f | %.3f | %.3f | %s | %s | %s |" % (
            name, s["median_ms"], s["best_ms"], s["worst_ms"], "%.3f" % s["per_frame_ms"] if "per_frame_ms" in s else "",
            "%.3f" % s["pre_pass_share"] if "pre_pass_share" in s else "",
            "%.0f" % s["median_over_one_read"] if "median_over_one_read" in s else ""))
    if not brute_ms > per_frame:
        print("THE CELL SWEEP IS NOT FASTER THAN THE BRUTE SWEEP: %.3f ms against %.3f ms per frame" % (per_frame, brute_ms))
        sys.exit(1)


if __name__ == "__main__":
    main()
