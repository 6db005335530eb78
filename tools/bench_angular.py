#!/usr/bin/env python
"""
tools/bench_angular.py — the bond-angle histograms (csrc/angles.hip) on the synthetic ion / 3-site-water trajectory of
tools/bench_hydration.py: 30 000 waters, 540 cations, 1 000 frames, device-resident coordinates, the triplet
O - cation - O at r_cut 3.5, bins of 1 degree. The library's event timers give the search pass (gather + sweep: the
call's aux time) and the angle pass (the rest of the call's kernel time) separately. In the same process the list mode
of the hydration search (cap 32) runs at the same centres and candidates: the same (cation, O) tests with an append
per hit. Both are priced against the FP64 VALU roof: 15 unfused f64 operations per test at 39.3e12 op/s (DESIGN.md
§4.1e). Writes profiles/angular_bench.json.

    python tools/bench_angular.py [--frames 1000] [--reps 10]
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


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--waters", type=int, default=30000)
    ap.add_argument("--cations", type=int, default=540)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "angular_bench.json"))
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
    types = np.full(n, 3, dtype=np.int32)  # cation 1, O 2, H 3
    types[ions], types[o] = 1, 2
    edges = B.angle_cos_edges(1.0)
    rec = {"frames": a.frames, "waters": a.waters, "cations": a.cations, "box": L, "r_cut": 3.5, "bin_size": 1.0,
           "triplet": "O-cation-O", "tests": a.frames * a.waters * a.cations, "device": ctx.name, "reps": a.reps}
    roof_ms = rec["tests"] * OPS_PER_TEST / VALU_OPS * 1e3
    rec["roof_ms"] = roof_ms
    total, search, hyd = [], [], []
    for _ in range(a.reps + 1):
        hist, degen, count, _ = B.angle_hist(xyz, box, types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges, ctx=ctx)
        total.append(ctx.last_kernel_ms()[0])
        search.append(ctx.last_aux_ms())
        _, _, hcount = B.hydration_cosines(xyz, box, ions, o, 3.5 ** 2, cap=32, ctx=ctx)
        hyd.append(ctx.last_kernel_ms()[0])
    assert np.array_equal(count, hcount)  # the same hits: every O within r_cut of every cation
    total, search, hyd = np.array(total[1:]), np.array(search[1:]), np.array(hyd[1:])
    rec["angles"] = int(hist.sum())
    rec["hits"] = int(count.sum())
    rec["largest_row"] = int(count.max())
    rec["search"] = dict(_stats(search), median_frac_of_roof=roof_ms / float(np.median(search)))
    rec["angle_pass"] = _stats(total - search)
    rec["call"] = _stats(total)
    rec["angle_share_of_call"] = float(np.median(total - search) / np.median(total))
    rec["hydration_list"] = dict(_stats(hyd), median_frac_of_roof=roof_ms / float(np.median(hyd)))
    rec["search_over_hydration"] = float(np.median(search) / np.median(hyd))
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
