#!/usr/bin/env python
"""
tools/bench_order.py — the order parameters (csrc/bond_order.hip) on the synthetic ion / 3-site-water trajectory of
tools/bench_angular.py: 30 000 waters, 540 cations, device-resident coordinates, O around O at r_cut 3.5 with
degrees (4, 6) and the tetrahedral pair. Every O is a centre here (30 000 x 30 000 tests per frame, against 540 x 30 000
of the cation benchmarks), so the default is 20 frames. The library's event timers give the search pass (gather + sweep:
the call's aux time) and the row pass (the rest of the call's kernel time) separately. In the same process the search of
angle_hist (the triplet O-O-O at the same cutoff) runs at the same centres and candidates: the same sweep with the same
per-hit work. Both are priced against the FP64 VALU roof: 15 unfused f64 operations per test at 39.3e12 op/s (DESIGN.md
§4.1e). Writes profiles/order_bench.json.

    python tools/bench_order.py [--frames 20] [--reps 10]
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
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--waters", type=int, default=30000)
    ap.add_argument("--cations", type=int, default=540)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "order_bench.json"))
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
    types = np.full(n, 3, dtype=np.int32)  # cation 1, O 2, H 3
    types[np.arange(a.cations)], types[o] = 1, 2
    edges = B.angle_cos_edges(1.0)
    rec = {"frames": a.frames, "waters": a.waters, "cations": a.cations, "box": L, "r_cut": 3.5, "degrees": [4, 6],
           "tetrahedral": True, "centres": "O", "neighbours": "O", "tests": a.frames * a.waters * a.waters,
           "device": ctx.name, "reps": a.reps}
    roof_ms = rec["tests"] * OPS_PER_TEST / VALU_OPS * 1e3
    rec["roof_ms"] = roof_ms
    total, search, ang = [], [], []
    for _ in range(a.reps + 1):
        out = B.bond_order(xyz, box, types, 2, [2], 3.5 ** 2, degrees=(4, 6), tetrahedral=True, ctx=ctx)
        total.append(ctx.last_kernel_ms()[0])
        search.append(ctx.last_aux_ms())
        _, _, acount, _ = B.angle_hist(xyz, box, types, [(2, 2, 2)], [[3.5 ** 2] * 2], edges, ctx=ctx)
        ang.append(ctx.last_aux_ms())
    assert np.array_equal(out["count"], acount)  # the same hits: every O within r_cut of every O
    total, search, ang = np.array(total[1:]), np.array(search[1:]), np.array(ang[1:])
    fl = out["flags"]
    rec["rows"] = int(fl.size)
    rec["hits"] = int(out["count"].sum())
    rec["largest_row"] = int(out["count"].max())
    rec["rows_q_short"] = int(np.count_nonzero(fl & B.BOND_Q_SHORT))
    rec["rows_tet_short"] = int(np.count_nonzero(fl & B.BOND_TET_SHORT))
    rec["mean_q4"], rec["mean_q6"] = (float(np.nanmean(out["q"][..., d])) for d in range(2))
    rec["mean_q_tet"] = float(np.nanmean(out["tet"][..., 0]))
    rec["search"] = dict(_stats(search), median_frac_of_roof=roof_ms / float(np.median(search)))
    rec["row_pass"] = _stats(total - search)
    rec["call"] = _stats(total)
    rec["row_share_of_call"] = float(np.median(total - search) / np.median(total))
    rec["angle_hist_search"] = dict(_stats(ang), median_frac_of_roof=roof_ms / float(np.median(ang)))
    rec["search_over_angle_hist_search"] = float(np.median(search) / np.median(ang))
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
