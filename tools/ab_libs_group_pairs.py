#!/usr/bin/env python
"""tools/ab_libs_group_pairs.py LIB.so [LIB.so ...] [--reps 5] — the two-group pair sweeps (csrc/vanhove.hip,
csrc/vector_pairs.hip) through several BUILDS of libmdhip.so in one process, two rounds, on the shapes of
tools/bench_vanhove.py (2 x 500 entities x 5000 frames at 20 lags, 2 x 20 000 x 200 at 4 lags; the a != b jobs and the
same-species jobs) and of tools/bench_vector_pairs.py (10 000 three-site molecules and 20 ions, 64 frames; water-water
and ions-water): median and best kernel time of --reps calls after one warm-up call, and whether every output has the
bytes of the first library's."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench_vanhove as V  # noqa: E402
import bench_vector_pairs as P  # noqa: E402
from mdproptools_amd import _lib  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402

libs = [a for a in sys.argv[1:] if a.endswith(".so")]
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5


def ctx_of(path):
    _lib._lib = None
    _lib.STRICT = False
    _lib.LIB_PATH = os.path.abspath(path)
    return _lib.Context(0)


ctxs = [ctx_of(p) for p in libs]
first = {}


def run(label, call):
    """call(ctx) -> a tuple of arrays, through every library, two rounds"""
    for rnd in range(2):
        for p, ctx in zip(libs, ctxs):
            ms = []
            for _ in range(reps + 1):
                out = call(ctx)
                ms.append(ctx.last_kernel_ms()[0])
            h = hashlib.sha256()
            for a in out:
                h.update(repr(a.tolist()).encode() if a.dtype == object else np.ascontiguousarray(a).tobytes())
            same = first.setdefault(label, h.hexdigest()) == h.hexdigest()
            print("%-22s %-34s %-16s median %9.4f ms  best %9.4f ms  launches %d  outputs %s" % (
                os.path.basename(p), label, ctx.last_kernel_name().split("<")[0], float(np.median(ms[1:])), min(ms[1:]),
                ctx.last_kernel_ms()[1], "equal to first" if same else "DIFFER"), flush=True)


for n, frames in ((500, 5000), (20000, 200)):
    g = torch.Generator(device="cuda").manual_seed(n)
    xu = torch.randn((frames, 3, 2 * n), generator=g, device="cuda", dtype=torch.float64) * 0.05
    xu[0] = torch.rand((3, 2 * n), generator=g, device="cuda", dtype=torch.float64) * V.BOX
    xu.cumsum_(dim=0)
    x = torch.remainder(xu, V.BOX).contiguous()
    del xu
    box, off = np.full((frames, 3), V.BOX), np.array([0, n, 2 * n], dtype=np.int64)
    ab = [(0, 1, k, 1) for k in V.LAGS[frames]]
    same = [(s, s, k, 1) for s in (0, 1) for k in V.LAGS[frames]]
    run("van Hove %dx%d a-b" % (n, frames), lambda c: B.van_hove_distinct(x, box, off, ab, V.BIN, V.N_BINS, ctx=c))
    run("van Hove %dx%d a-a b-b" % (n, frames), lambda c: B.van_hove_distinct(x, box, off, same, V.BIN, V.N_BINS, ctx=c))
    del x
    torch.cuda.empty_cache()

n, F = 10000, 64
L = (n * P.VOLUME_PER_MOLECULE) ** (1.0 / 3.0)
n_bins = int(L / 2 / P.BIN)
g = torch.Generator(device="cuda").manual_seed(n)
site = torch.rand((F, 3, n + P.IONS), generator=g, device="cuda", dtype=torch.float64) * L
vec = torch.randn((F, 3, n + P.IONS), generator=g, device="cuda", dtype=torch.float64)
vec /= vec.norm(dim=1, keepdim=True)
box, off = np.full((F, 3), L), np.array([0, n, n + P.IONS], dtype=np.int64)
for label, job in (("vector pairs water-water", (0, 0)), ("vector pairs ions-water", (1, 0))):
    run(label, lambda c: B.vector_pair_hist(site, vec, box, off, [job], P.BIN, n_bins, ctx=c))
