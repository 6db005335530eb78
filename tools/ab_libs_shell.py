#!/usr/bin/env python
"""tools/ab_libs_shell.py LIB.so LIB.so [LIB.so ...] — the consumers of csrc/shell_search.h through several BUILDS of
libmdhip.so in one process: hydration_counts and hydration_cosines on the system of tools/bench_hydration.py, angle_hist
on that of tools/bench_angular.py, shell_members on that of tools/bench_clusters.py and shell_coordination on the same
atoms with classes and a pass mask. One round per LIB argument, in the order given (a path may repeat: P N P N); every
output array of a call is compared with the first round's, byte for byte; kernel time per call from the library's own
timer, after a warm-up call, with the repetitions of those tools (10, 10, 20; --reps-scale multiplies them)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cluster_ref as R  # noqa: E402
from bench_clusters import replica  # noqa: E402
from mdproptools_amd import _lib  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402

args = sys.argv[1:]
scale = int(args[args.index("--reps-scale") + 1]) if "--reps-scale" in args else 1
frames = int(args[args.index("--frames") + 1]) if "--frames" in args else 1000
libs = [a for a in args if a.endswith(".so")]


def ctx_of(path):
    _lib._lib = None
    _lib.STRICT = False
    _lib.LIB_PATH = os.path.abspath(path)
    return _lib.Context(0)


ctxs = {}
for p in libs:
    if p not in ctxs:
        ctxs[p] = ctx_of(p)

# the ion / 3-site-water trajectory of tools/bench_hydration.py and tools/bench_angular.py
n_wat, n_cat = 30000, 540
n = n_cat + 3 * n_wat
L = (n_wat / 0.0334) ** (1.0 / 3.0)
g = torch.Generator(device="cuda").manual_seed(0)
xyz = torch.rand((frames, 3, n), generator=g, device="cuda", dtype=torch.float64) * L
o = n_cat + 3 * np.arange(n_wat)
ot = torch.as_tensor(o, device="cuda")
for h in (1, 2):
    xyz[:, :, ot + h] = xyz[:, :, ot] + 0.6 * torch.randn((frames, 3, n_wat), generator=g, device="cuda",
                                                          dtype=torch.float64)
box = np.full((frames, 3), L)
ions = np.arange(n_cat)
types = np.full(n, 3, dtype=np.int32)  # cation 1, O 2, H 3
types[ions], types[o] = 1, 2
edges = B.angle_cos_edges(1.0)

# the 4 x 4 x 4 replica of tools/bench_clusters.py, with classes from the atom types and a pass mask
cxyz, cL, ctypes_, cmol = replica(R.load())
centres = np.flatnonzero(ctypes_ == 9).astype(np.int32)
_, seg_off, mol_type = R.layout([m * 64 for m in R.NUM_MOLS], R.NUM_ATOMS)
cls = np.where(ctypes_ % 4 == 3, 0xFF, ctypes_ % 4).astype(np.uint8)
passes = np.random.default_rng(0).uniform(size=(1, len(mol_type))) < 0.8

CALLS = [
    ("hydration_counts", 10, lambda c: B.hydration_counts(xyz, box, ions, o, 3.5 ** 2, -0.72, 0.02, 100, ctx=c)),
    ("hydration_cosines", 10, lambda c: B.hydration_cosines(xyz, box, ions, o, 3.5 ** 2, cap=32, ctx=c)),
    ("angle_hist", 10, lambda c: B.angle_hist(xyz, box, types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges, ctx=c)[:3]),
    ("shell_members", 20, lambda c: B.shell_members(cxyz[None], cL[None, :], centres, cmol, 2.3 ** 2, ctx=c)),
    ("shell_coordination", 20, lambda c: B.shell_coordination(cxyz[None], cL[None, :], centres, cmol, seg_off, mol_type,
                                                              cls, 2.3 ** 2, 2.0 ** 2, passes=passes, ctx=c)),
]

first = {}
for rnd, p in enumerate(libs):
    ctx = ctxs[p]
    for name, reps, call in CALLS:
        ms, aux = [], []
        for _ in range(reps * scale + 1):
            out = call(ctx)
            ms.append(ctx.last_kernel_ms()[0])
            aux.append(ctx.last_aux_ms())
        blob = [np.ascontiguousarray(a).tobytes() for a in out]
        same = first.setdefault(name, blob) == blob
        ms, aux = np.array(ms[1:]), np.array(aux[1:])
        print("round %d %-22s %-20s median %8.4f ms  min %8.4f  max %8.4f  aux median %7.4f  (%s, %d arrays, %d bytes)"
              % (rnd, os.path.basename(p), name, np.median(ms), ms.min(), ms.max(), np.median(aux),
                 "identical to round 0" if same else "DIFFERENT FROM ROUND 0", len(blob), sum(map(len, blob))),
              flush=True)
        assert same, "results differ"
