#!/usr/bin/env python
"""
tools/bench_sdf.py — the spatial distribution histograms (csrc/sdf.hip) on a synthetic liquid: 512 three-atom reference
molecules and 20 000 observed atoms of two species in a box of 50, 500 frames resident on the device, r_cut 9 and cells
of 0.5 (G = 36): 2.4 % of all (origin atom, observed atom) tests are hits. The library's event timers give the frame
pre-pass and the gather (the call's aux time) and the sweep (the rest of the call's kernel time) separately. In the
same process, alternating with it call by call:
  the counts mode of the hydration search (backend.hydration_counts) over the same centres and candidates: the same
  tests, and per hit one cosine and three counters where the SDF makes three projections and one grid atomic;
  with --variant LIB.so, the same call through another BUILD of the library (tools/build_variant.sh: the serial-loop
  form of the sweep while the two were being compared); its results are compared byte for byte.
Both sweeps are priced against the FP64 VALU roof: 15 unfused f64 operations per test at 39.3e12 op/s (DESIGN.md
§4.1e). Writes profiles/sdf_bench.json.

    python tools/bench_sdf.py [--frames 500] [--reps 10] [--variant tools/_bin/libmdhip_NAME.so]
"""

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import _lib  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402

OPS_PER_TEST, VALU_OPS = 15, 39.3e12


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def _ctx_of(path):
    """A context on another build of the library (the way of tools/ab_libs_shell.py)."""
    _lib._lib = None
    _lib.STRICT = False
    _lib.LIB_PATH = os.path.abspath(path)
    return _lib.Context(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--mols", type=int, default=512)
    ap.add_argument("--observed", type=int, default=20000)
    ap.add_argument("--box", type=float, default=50.0)
    ap.add_argument("--r-cut", type=float, default=9.0)
    ap.add_argument("--bin-size", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "sdf_bench.json"))
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    var = _ctx_of(a.variant) if a.variant else None
    n = 3 * a.mols + a.observed + 2  # (two trailing atoms: every `water` of the hydration leg has its two followers)
    g = torch.Generator(device="cuda").manual_seed(0)
    xyz = torch.rand((a.frames, 3, n), generator=g, device="cuda", dtype=torch.float64) * a.box
    o = 3 * np.arange(a.mols)
    ot = torch.as_tensor(o, device="cuda")
    for k in (1, 2):
        xyz[:, :, ot + k] = xyz[:, :, ot] + 0.7 * torch.randn((a.frames, 3, a.mols), generator=g, device="cuda",
                                                              dtype=torch.float64)
    box = np.full((a.frames, 3), a.box)
    cand = np.arange(3 * a.mols, 3 * a.mols + a.observed)
    cls = (cand % 2).astype(np.int32)
    G = B.sdf_grid(a.r_cut, a.bin_size)
    rec = {"frames": a.frames, "mols": a.mols, "observed": a.observed, "box": a.box, "r_cut": a.r_cut,
           "bin_size": a.bin_size, "grid": G, "species": 2, "tests": a.frames * a.mols * a.observed,
           "device": ctx.name, "reps": a.reps, "variant": a.variant}
    roof_ms = rec["tests"] * OPS_PER_TEST / VALU_OPS * 1e3
    rec["roof_ms"] = roof_ms

    def sdf(c):
        out = B.sdf_hist(xyz, box, o, o + 1, o + 2, cand, cls, 2, a.r_cut, a.bin_size, ctx=c)
        return out, c.last_kernel_ms()[0], c.last_aux_ms()

    total, pre, hyd, vtotal, vpre = [], [], [], [], []
    for _ in range(a.reps + 1):  # (the first round warms up)
        out, ms, aux = sdf(ctx)
        total.append(ms)
        pre.append(aux)
        n_water, _, _ = B.hydration_counts(xyz, box, o, cand, B.cutoff_sq(a.r_cut), 0.0, 0.02, 100, ctx=ctx)
        hyd.append(ctx.last_kernel_ms()[0])
        if var is not None:
            vout, ms, aux = sdf(var)
            vtotal.append(ms)
            vpre.append(aux)
            same = all(np.array_equal(x, y) for x, y in zip(out[:3], vout[:3])) and out[3] == vout[3]
            assert same, "the variant's results differ"
    hist, degen, n_hits, bad_rows = out
    assert np.array_equal(n_hits, n_water)  # the same hits: every observed atom within r_cut of every origin atom
    assert int(hist.sum()) + int(degen.sum()) == int(n_hits.sum())
    total, pre, hyd = np.array(total[1:]), np.array(pre[1:]), np.array(hyd[1:])
    rec["hits"] = int(n_hits.sum())
    rec["hit_share"] = rec["hits"] / rec["tests"]
    rec["degenerate_rows"] = bad_rows
    rec["call"] = _stats(total)
    rec["pre_pass"] = _stats(pre)
    rec["sweep"] = dict(_stats(total - pre), median_frac_of_roof=roof_ms / float(np.median(total - pre)))
    rec["hydration_counts"] = dict(_stats(hyd), median_frac_of_roof=roof_ms / float(np.median(hyd)))
    rec["call_over_hydration"] = float(np.median(total) / np.median(hyd))
    if var is not None:
        vtotal, vpre = np.array(vtotal[1:]), np.array(vpre[1:])
        rec["variant_call"] = _stats(vtotal)
        rec["variant_sweep"] = _stats(vtotal - vpre)
        rec["sweep_over_variant_sweep"] = float(np.median(total - pre) / np.median(vtotal - vpre))
        rec["variant_results"] = "identical"
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
