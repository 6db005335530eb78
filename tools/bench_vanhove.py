#!/usr/bin/env python
"""
tools/bench_vanhove.py — the distinct van Hove kernel (csrc/vanhove.hip) on device-resident frames, two species in a
box of 30 with 300 bins of 0.05 (r_max = L/2: nothing can be culled), stride 1:
  2 x 500 entities x 5000 frames, 20 lags      2 x 20 000 entities x 200 frames, 4 lags
For each shape the a != b jobs run alone, in ONE call, against the route that existed before, in the same process: one
backend.rdf_mol_loop(..., per_frame=False) call per lag on the contiguous device views r[:F-k] of species a and r[k:] of
species b — once with default options (the packed-f32 sweep) and once with the all-f64 sweep (rdf_pk = 0; the kernel
name the library reports says whether the option took). The integers of the routes must be equal. The same-species
jobs (a, a) and (b, b) are timed beside them. Every call is timed with the library's event timer and with a host clock
around the synchronous call, after one warm-up call; medians of --reps calls. Writes profiles/vanhove_bench.json.

    python tools/bench_vanhove.py [--reps 10] [--shapes 500x5000,20000x200] [--out FILE]
"""

import argparse
import json
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd._lib import default_context  # noqa: E402

BIN, N_BINS, BOX = 0.05, 300, 30.0
LAGS = {5000: [1, 2, 3, 5, 8, 10, 20, 30, 50, 80, 100, 200, 300, 500, 800, 1000, 1500, 2000, 3000, 4000],
        200: [1, 10, 50, 100]}


def timed(ctx, reps, call):
    """One warm-up call, then `reps`: (median kernel ms, best, median wall ms, median preparation ms, last result)."""
    ms, wall, aux = [], [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_kernel_ms()[0])
        aux.append(ctx.last_aux_ms())
    return (float(np.median(ms[1:])), float(np.min(ms[1:])), float(np.median(wall[1:])), float(np.median(aux[1:])),
            out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="500x5000,20000x200")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "vanhove_bench.json"))
    a = ap.parse_args()
    ctx = default_context(0)
    rec = {"device": ctx.name, "hip": torch.version.hip, "date": time.strftime("%Y-%m-%d"), "bin_size": BIN,
           "n_bins": N_BINS, "box": BOX, "reps": a.reps, "shapes": []}
    ok = True
    for shape in a.shapes.split(","):
        n, frames = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n)
        xu = torch.randn((frames, 3, 2 * n), generator=g, device="cuda", dtype=torch.float64) * 0.05
        xu[0] = torch.rand((3, 2 * n), generator=g, device="cuda", dtype=torch.float64) * BOX
        xu.cumsum_(dim=0)
        x = torch.remainder(xu, BOX).contiguous()
        del xu
        box = np.full((frames, 3), BOX)
        off = np.array([0, n, 2 * n], dtype=np.int64)
        lags = LAGS.get(frames) or sorted({max(1, frames * (j + 1) // 10) for j in range(4)})
        srec = {"entities_per_species": n, "frames": frames, "lags": lags}

        # the a != b jobs alone, one call
        jobs = [(0, 1, k, 1) for k in lags]
        med, best, wall, _, out = timed(ctx, a.reps, lambda: B.van_hove_distinct(x, box, off, jobs, BIN, N_BINS, ctx=ctx))
        hist, beyond, pairs = out
        n_pairs = int(pairs.sum())
        srec["van_hove_ab"] = {"kernel": ctx.last_kernel_name(), "launches": ctx.last_kernel_ms()[1], "calls": 1,
                               "kernel_median_ms": med, "kernel_best_ms": best, "wall_median_ms": wall,
                               "pairs": n_pairs, "beyond_share": float(beyond.sum()) / n_pairs,
                               "kernel_ps_per_pair": med * 1e9 / n_pairs}
        assert np.array_equal(hist.sum(axis=1) + beyond, pairs)

        # the route that existed: one atoms x sites sweep per lag on shifted views of the two species
        xa = x[:, :, :n].contiguous()
        xb = x[:, :, n:].contiguous()
        ones = np.ones(n, dtype=np.int32)
        rel = np.array([[1, 1]])

        def loop_of_calls(stats):
            rows = []
            for k in lags:
                part, _ = B.rdf_mol_loop(xa[:frames - k], ones, xb[k:], ones, box[:frames - k], rel, N_BINS * BIN, BIN,
                                         N_BINS, per_frame=False, ctx=ctx)
                rows.append(np.asarray(part).reshape(N_BINS))
                stats.append((ctx.last_kernel_ms()[0], ctx.last_aux_ms(), ctx.last_kernel_name()))
            return np.stack(rows)

        for label, pk in (("rdf_sites_default", -1), ("rdf_sites_f64", 0)):
            ctx.set_option("rdf_pk", pk)
            kern, prep, wall, names = [], [], [], set()
            for _ in range(a.reps + 1):
                stats = []
                t0 = time.perf_counter()
                rows = loop_of_calls(stats)
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(sum(s[0] for s in stats))
                prep.append(sum(s[1] for s in stats))
                names |= {s[2] for s in stats}
            modes = sorted({int(m) for nm in names for m in re.findall(r"pair_hist_sj_kernel<(\d+)", nm)})
            equal = bool(np.array_equal(rows.astype(np.uint64), hist))
            ok = ok and equal
            srec[label] = {"kernels": sorted(names), "sj_modes": modes, "packed_f32": any(m >= 3 for m in modes),
                           "calls": len(lags), "kernel_median_ms": float(np.median(kern[1:])),
                           "kernel_best_ms": float(np.min(kern[1:])), "preparation_median_ms": float(np.median(prep[1:])),
                           "wall_median_ms": float(np.median(wall[1:])), "equal_to_van_hove": equal,
                           "kernel_ps_per_pair": float(np.median(kern[1:])) * 1e9 / n_pairs}
        ctx.set_option("rdf_pk", -1)
        if srec["rdf_sites_f64"]["packed_f32"]:
            ok = False
            srec["rdf_sites_f64"]["note"] = "rdf_pk = 0 did not take: the reported kernel is a packed-f32 one"
        srec["kernel_time_over_f64_sweep"] = med / srec["rdf_sites_f64"]["kernel_median_ms"]
        srec["kernel_time_over_default_sweep"] = med / srec["rdf_sites_default"]["kernel_median_ms"]
        srec["wall_over_loop_of_calls_default"] = srec["van_hove_ab"]["wall_median_ms"] / srec["rdf_sites_default"]["wall_median_ms"]
        srec["wall_over_loop_of_calls_f64"] = srec["van_hove_ab"]["wall_median_ms"] / srec["rdf_sites_f64"]["wall_median_ms"]
        del xa, xb

        # the same-species jobs
        jobs = [(g_, g_, k, 1) for g_ in (0, 1) for k in lags]
        med, best, wall, _, out = timed(ctx, a.reps, lambda: B.van_hove_distinct(x, box, off, jobs, BIN, N_BINS, ctx=ctx))
        n_same = int(out[2].sum())
        assert np.array_equal(out[0].sum(axis=1) + out[1], out[2])
        srec["van_hove_aa_bb"] = {"calls": 1, "kernel_median_ms": med, "kernel_best_ms": best, "wall_median_ms": wall,
                                  "pairs": n_same, "kernel_ps_per_pair": med * 1e9 / n_same}
        rec["shapes"].append(srec)
        del x
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    if not ok:
        sys.exit("the routes disagree, or the all-f64 option did not take: see " + a.out)


if __name__ == "__main__":
    main()
