#!/usr/bin/env python
"""
tools/bench_aggregates.py — the contact components (csrc/aggregates.hip) on the synthetic ion / 3-site-water trajectory
of tools/bench_hydration.py: 30 000 molecules of three sites whose first site is the candidate, 540 cations, 1 000
frames, device-resident coordinates, the contact cation - first site at r_cut 3.5, molecules as nodes. The library's
event timers give the gather and the union sweep (the call's aux time) and the rest (the initialisation of the parent
rows and the label pass) separately. After every call, in the same process, the counts mode of the hydration search
runs at the same centres and candidates: the same (cation, site) tests and no graph work — the yardstick. One dense
case follows (r_cut 12: hundreds of contacts per centre, every union into one giant component), the price of contended
compare-and-swaps, against the same search at that cutoff. Writes profiles/aggregates_bench.json.

    python tools/bench_aggregates.py [--frames 1000] [--reps 10]
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


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def _case(ctx, xyz, box, ions, o, node_of, n_nodes, r_cut, reps):
    """`reps` timed calls (after one untimed) of contact_components, each followed by the counts-mode search."""
    zeros_a, zeros_b = np.zeros(len(ions), dtype=np.int32), np.zeros(len(o), dtype=np.int32)
    total, sweep, search = [], [], []
    for _ in range(reps + 1):
        label, n_comp, n_con = B.contact_components(xyz, box, ions, zeros_a, o, zeros_b, [[r_cut ** 2]], node_of,
                                                    n_nodes, ctx=ctx)
        total.append(ctx.last_kernel_ms()[0])
        sweep.append(ctx.last_aux_ms())
        n_water, _, _ = B.hydration_counts(xyz, box, ions, o, r_cut ** 2, 0.0, 0.01, 200, ctx=ctx)
        search.append(ctx.last_kernel_ms()[0])
    assert int(n_con.sum()) == int(n_water.sum())  # the same hits: every candidate within r_cut of every cation
    total, sweep, search = np.array(total[1:]), np.array(sweep[1:]), np.array(search[1:])
    sizes = np.bincount(np.bincount(label[0], minlength=n_nodes))
    return {"r_cut": r_cut, "frames": len(box), "tests": len(box) * len(ions) * len(o), "contacts": int(n_con.sum()),
            "contacts_per_centre_frame": float(n_con.sum() / (len(box) * len(ions))),
            "components_frame0": int(n_comp[0]), "largest_frame0": int(len(sizes) - 1),
            "call": _stats(total), "gather_and_sweep": _stats(sweep), "init_and_labels": _stats(total - sweep),
            "counts_search": dict(_stats(search), spread_ms=float(search.max() - search.min())),
            "sweep_over_search": float(np.median(sweep) / np.median(search)),
            "call_over_search": float(np.median(total) / np.median(search)),
            "excess_ms": {"sweep": float(np.median(sweep) - np.median(search)),
                          "init_and_labels": float(np.median(total - sweep))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--dense-frames", type=int, default=100)
    ap.add_argument("--waters", type=int, default=30000)
    ap.add_argument("--cations", type=int, default=540)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "aggregates_bench.json"))
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
    node_of = np.concatenate([ions, a.cations + np.repeat(np.arange(a.waters), 3)]).astype(np.int32)
    n_nodes = a.cations + a.waters
    rec = {"molecules": a.waters, "cations": a.cations, "box": L, "nodes": n_nodes, "device": ctx.name,
           "reps": a.reps, "note": "one machine, one run"}
    rec["first_shell"] = _case(ctx, xyz, box, ions, o, node_of, n_nodes, 3.5, a.reps)
    nd = min(a.dense_frames, a.frames)
    rec["dense"] = _case(ctx, xyz[:nd].contiguous(), box[:nd], ions, o, node_of, n_nodes, 12.0, a.reps)
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
