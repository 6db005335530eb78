#!/usr/bin/env python
"""
tools/bench_hbonds.py — the hydrogen-bond kernels (csrc/hbonds.hip) on a synthetic water-like trajectory: 3 000
three-site molecules O H H at liquid density, 1 000 frames, device-resident coordinates; the O sites jitter around
fixed places and the O-H directions around fixed directions, so that a bond that exists in one frame mostly exists in
the next (uncorrelated frames would make every bond a new pair). Donors and acceptors are the O sites, r_da 3.5,
angle_cut 150.

  counts:   backend.hbond_counts; after every call, in the same process, the counts mode of the hydration search
            (mdhip_hydration_counts) with the same centres, candidates and cutoff: the same (centre, candidate) tests
            and one cosine per hit — the yardstick for "the hydration search plus rare-hit work".
  lifetime: backend.hbond_lifetime; the library's event timers give the two lag kernels (the call's aux time) and
            the rest (gather and sweeps) separately. After every call mdhip_shell_residence on the O sites with the
            shell (0, 3.5] at the same frame count: its sweep and its lag kernel over the O-O pairs in reach (many more
            pairs than there are bonds; the numbers of pairs are recorded beside the times).

Writes profiles/hbonds_bench.json.

    python tools/bench_hbonds.py [--frames 1000] [--waters 3000] [--reps 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--waters", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "hbonds_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    W, F = a.waters, a.frames
    L = (W / 0.0334) ** (1.0 / 3.0)  # liquid-water density
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    place = torch.rand((1, 3, W), generator=g, device="cuda", dtype=torch.float64) * L
    xyz = torch.empty((F, 3, 3 * W), device="cuda", dtype=torch.float64)
    xyz[:, :, 0::3] = place + 0.1 * rnd(F, 3, W)
    for h in (1, 2):
        u = rnd(1, 3, W) + 0.25 * rnd(F, 3, W)
        xyz[:, :, h::3] = xyz[:, :, 0::3] + 0.96 * u / u.norm(dim=1, keepdim=True)
    box = np.full((F, 3), L)
    o = (3 * np.arange(W)).astype(np.int32)
    h_off = (2 * np.arange(W + 1)).astype(np.int32)
    h_atoms = np.stack([o + 1, o + 2], axis=1).ravel().astype(np.int32)
    zeros = np.zeros(W, dtype=np.int32)
    mol_of = (np.arange(3 * W) // 3).astype(np.int32)
    r2, cut = 3.5 ** 2, float(np.cos(np.radians(150.0)))
    edges = B.angle_cos_edges(1.0)
    o_planes = xyz[:, :, 0::3].contiguous()

    counts, search, life, lags, resid, launches = [], [], [], [], [], []
    for _ in range(a.reps + 1):
        n_bonds, n_don, n_acc, hist, degen = B.hbond_counts(xyz, box, o, zeros, h_off, h_atoms, o, zeros, r2, cut,
                                                            cos_edges=edges, mol_of=mol_of)
        counts.append(ctx.last_kernel_ms()[0])
        n_water, _, _ = B.hydration_counts(xyz, box, o, o, r2, 0.0, 0.01, 200, ctx=ctx)
        search.append(ctx.last_kernel_ms()[0])
    for _ in range(a.reps + 1):
        c_int, c_cont, n_pairs, n_rec = B.hbond_lifetime(xyz, box, o, h_off, h_atoms, o, r2, cut, mol_of=mol_of)
        ms, n_launch = ctx.last_kernel_ms()
        life.append(ms)
        lags.append(ctx.last_aux_ms())
        launches.append(n_launch)
        r_counts, r_rec = B.shell_residence(o_planes, o_planes, box, 0.0, r2, exclude_diagonal=True, ctx=ctx)
        resid.append(ctx.last_kernel_ms()[0])
    assert int(n_bonds.sum()) == n_rec == int(c_int[0]) == int(c_cont[0])
    assert int(hist.sum()) + degen == 2 * (int(n_water.sum()) - F * W)  # every O-O hit but the centre itself, two H each
    counts, search, life, lags, resid = (np.array(v[1:]) for v in (counts, search, life, lags, resid))
    rec = {
        "molecules": W, "frames": F, "box": L, "device": ctx.name, "reps": a.reps, "note": "one machine, one run",
        "tests": F * W * W, "bonds": int(n_bonds.sum()), "bonds_per_molecule_frame": float(n_bonds.sum() / (F * W)),
        "angle_tests": int(hist.sum()) + int(degen),
        "counts": {"call": _stats(counts), "hydration_counts_search": _stats(search),
                   "call_over_search": float(np.median(counts) / np.median(search)),
                   "excess_ms": float(np.median(counts) - np.median(search))},
        "lifetime": {"call": _stats(life), "lag_kernels": _stats(lags), "gather_and_sweeps": _stats(life - lags),
                     "launches": int(launches[-1]), "n_pairs": n_pairs, "n_records": n_rec,
                     "c_int_at_10": int(c_int[min(10, F - 1)]), "c_cont_at_10": int(c_cont[min(10, F - 1)]),
                     "shell_residence_call": _stats(resid), "residence_records": int(r_rec),
                     "sweeps_over_counts_call": float(np.median(life - lags) / np.median(counts)),
                     "call_over_residence": float(np.median(life) / np.median(resid))},
    }
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
