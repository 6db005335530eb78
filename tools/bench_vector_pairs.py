#!/usr/bin/env python
"""
tools/bench_vector_pairs.py — the orientational pair sweep (csrc/vector_pairs.hip) against the same sweep without its
payload, in one process: mdhip_van_hove_distinct at lag 0 on the same sites, groups, box and bins. Shape: 10 000
water-like three-site molecules and 20 ions at the density of water (L = 66.9), 64 device-resident frames, r_cut = L/2,
bins of 0.05; the jobs water-water (a == b) and ions against water, each timed on its own. The sites lie inside the box,
where the single wrap of the van Hove kernel and the nearest image of the pair sweep are the same image: the two
histograms must be equal. The two calls alternate, after one warm-up call each; the library's event timer and a host
clock around the synchronous call; medians of --reps calls. Also mdhip_mol_moments (dipole and first-atom site of every
molecule, device in, device out) against the bytes it has to move — one read of the trajectory, one write of the two
outputs — over the HBM streaming rate of MI355X_MICROARCH.md (6.29 TB/s, measured float4 copy): `measured` are times,
`modelled` are bytes over that rate. Recorded, not gated. Writes profiles/vector_pairs.txt.

    python tools/bench_vector_pairs.py [--reps 7] [--mols 10000] [--frames 64] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

BIN = 0.05
IONS = 20
VOLUME_PER_MOLECULE = 29.9  # cubic angstrom: water at 1 g/cm^3
HBM_BYTES_PER_S = 6.29e12   # MI355X_MICROARCH.md: measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mols", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "vector_pairs.txt"))
    a = ap.parse_args()
    ctx = default_context(0)
    n, F = a.mols, a.frames
    L = (n * VOLUME_PER_MOLECULE) ** (1.0 / 3.0)
    n_bins = int(L / 2 / BIN)
    g = torch.Generator(device="cuda").manual_seed(n)
    rand = lambda *shape: torch.rand(shape, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    oxygen = rand(F, 3, n) * L
    arms = torch.randn((F, 3, n, 2), generator=g, device="cuda", dtype=torch.float64)
    arms /= arms.norm(dim=1, keepdim=True)
    water = torch.cat([oxygen[..., None], torch.remainder(oxygen[..., None] + arms, L)], dim=3).reshape(F, 3, 3 * n)
    x = torch.cat([water, rand(F, 3, IONS) * L], dim=2).contiguous()
    del oxygen, arms, water
    box = np.full((F, 3), L)
    a0, mols, length = [0, 3 * n], [n, IONS], [3, 1]
    S = n + IONS
    site, vec = (torch.empty((F, 3, S), dtype=torch.float64, device="cuda") for _ in range(2))
    moments = lambda: B.mol_moments(x, box, a0, mols, length, [[], []], [[(1, 0.4), (2, 0.4)], []], [1, 0],  # noqa: E731
                                    site_out=site, vec_out=vec, ctx=ctx)
    ms, wall = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = moments()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_kernel_ms()[0])
    assert not got["degenerate"].any()
    moved = x.numel() * 8 + 2 * site.numel() * 8
    rec = {"device": ctx.name, "hip": torch.version.hip, "date": time.strftime("%Y-%m-%d"), "molecules": n, "ions": IONS,
           "frames": F, "box": L, "bin_size": BIN, "n_bins": n_bins, "reps": a.reps, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "mol_moments": {"kernel": ctx.last_kernel_name(), "kernel_median_ms": float(np.median(ms[1:])),
                           "kernel_best_ms": float(np.min(ms[1:])), "wall_median_ms": float(np.median(wall[1:])),
                           "bytes_moved": moved, "bytes_over_hbm_rate_ms_modelled": moved / HBM_BYTES_PER_S * 1e3,
                           "achieved_bytes_per_s": moved / (float(np.median(ms[1:])) * 1e-3)},
           "jobs": []}
    off = np.array([0, n, S], dtype=np.int64)
    ok = True
    for label, job in (("water-water (a == b)", (0, 0)), ("ions-water", (1, 0))):
        calls = {"vector_pair_hist": lambda: B.vector_pair_hist(site, vec, box, off, [job], BIN, n_bins, ctx=ctx),
                 "van_hove_distinct_lag0": lambda: B.van_hove_distinct(site, box, off, [job + (0, 1)], BIN, n_bins, ctx=ctx)}
        ms, wall, out, kernel = {k: [] for k in calls}, {k: [] for k in calls}, {}, {}
        for _ in range(a.reps + 1):  # (the first round is the warm-up; the two calls alternate)
            for name, call in calls.items():
                t0 = time.perf_counter()
                out[name] = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                ms[name].append(ctx.last_kernel_ms()[0])
                kernel[name] = ctx.last_kernel_name()
        hist, sums, beyond, unsummed, pairs = out["vector_pair_hist"]
        equal = bool(np.array_equal(hist, out["van_hove_distinct_lag0"][0]))
        ok = ok and equal and int(unsummed[0]) == 0
        n_pairs = int(pairs[0])
        jrec = {"job": label, "pairs": n_pairs, "inside_r_cut_share": float(hist.sum()) / n_pairs,
                "unsummed": int(unsummed[0]), "hist_equal_to_van_hove": equal}
        for name in calls:
            med = float(np.median(ms[name][1:]))
            jrec[name] = {"kernel": kernel[name], "kernel_median_ms": med, "kernel_best_ms": float(np.min(ms[name][1:])),
                          "kernel_spread_ms": float(np.max(ms[name][1:]) - np.min(ms[name][1:])),
                          "wall_median_ms": float(np.median(wall[name][1:])), "pairs_per_s": n_pairs / (med * 1e-3)}
        jrec["kernel_time_over_van_hove"] = jrec["vector_pair_hist"]["kernel_median_ms"] / jrec["van_hove_distinct_lag0"]["kernel_median_ms"]
        rec["jobs"].append(jrec)
    text = json.dumps(rec, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    if not ok:
        sys.exit("the histograms of the two sweeps differ, or a pair could not be summed: see " + a.out)


if __name__ == "__main__":
    main()
