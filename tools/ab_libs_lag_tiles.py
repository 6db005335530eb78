#!/usr/bin/env python
"""tools/ab_libs_lag_tiles.py LIB.so LIB.so [LIB.so ...] — the three direct lag sweeps of csrc/lag_tiles.h through several
BUILDS of libmdhip.so in one process, next to tools/ab_libs_xcorr.py: the direct correlation (three series of 10^6
samples, auto- and cross-correlation), mdhip_cross_msd on the shapes of tools/bench_einstein.py (n = 10 000 and 100 000,
G = 1, 3, 8, max_lag = n // 2, with and without the |term| sums) and mdhip_orient_corr on that of
tools/bench_reorientation.py (4096 series of 5000 frames, max_lag 2500, unit vectors drawn directly), all on
floating-point inputs. Witnesses whose code no build of this comparison touches: collective_kernel (20 000 entities x
2000 frames) and the FFT estimator. One round per LIB argument, in the order given (a path may repeat: P N P N); every
output array of a call is compared with the first round's, byte for byte; kernel time per call from the library's own
timer after a warm-up call (--reps N, default 5; --only NAME[,NAME...] runs those calls alone)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdproptools_amd import _lib  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402

args = sys.argv[1:]
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
only = args[args.index("--only") + 1].split(",") if "--only" in args else None
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

g = torch.Generator(device="cuda").manual_seed(0)
randn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
x, y = randn(3, 1_000_000), randn(3, 1_000_000)
series = {(n, G): randn(G, 3, n).cumsum_(dim=2) for n in (10_000, 100_000) for G in (1, 3, 8)}
U = randn(4096, 3, 5000)
U /= U.norm(dim=1, keepdim=True)
u_off = np.array([0, 4096], dtype=np.int64)
r = randn(2000, 3, 20_000)
w = np.where(np.arange(20_000) % 2 == 0, 1.0, -1.0) * 1.602e-19
r_off = np.array([0, 7000, 14_000, 20_000], dtype=np.int64)


def cross_msd(P, with_abs, c):
    n, G = P.shape[2], P.shape[0]
    out = torch.empty((n // 2 + 1, G, G), dtype=torch.float64, device="cuda")
    ab = torch.empty_like(out) if with_abs else None
    B.cross_msd(P, n // 2, out=out, abs_out=ab, ctx=c)
    return [out.cpu().numpy()] + ([ab.cpu().numpy()] if with_abs else [])


CALLS = [("xcorr_direct/auto", lambda c: [B.xcorr(x, None, method=B.XCORR_DIRECT, ctx=c)]),
         ("xcorr_direct/cross", lambda c: [B.xcorr(x, y, method=B.XCORR_DIRECT, ctx=c)])]
for (n_, G_), P_ in series.items():
    for abs_ in (False, True):
        CALLS.append(("cross_msd/n%d/G%d/%s" % (n_, G_, "abs" if abs_ else "plain"),
                      lambda c, P_=P_, abs_=abs_: cross_msd(P_, abs_, c)))
CALLS += [("orient_corr", lambda c: [B.orient_corr(U, u_off, 2500, ctx=c)]),
          ("witness/collective", lambda c: [B.collective_displacement(r, w, r_off, scale=1e-10, ctx=c)]),
          ("witness/xcorr_fft", lambda c: [B.xcorr(x, y, method=B.XCORR_FFT, ctx=c)])]
if only is not None:
    CALLS = [c for c in CALLS if c[0] in only]

first = {}
for rnd, p in enumerate(libs):
    ctx = ctxs[p]
    for name, call in CALLS:
        ms = []
        for _ in range(reps + 1):
            out = call(ctx)
            ms.append(ctx.last_kernel_ms()[0])
        blob = [np.ascontiguousarray(a).tobytes() for a in out]
        same = first.setdefault(name, blob) == blob
        ms = np.array(ms[1:])
        print("round %d %-22s %-28s median %9.4f ms  min %9.4f  max %9.4f  %-16s launches %d  (%s, %d arrays, %d bytes)"
              % (rnd, os.path.basename(p), name, np.median(ms), ms.min(), ms.max(), ctx.last_kernel_name()[:16],
                 ctx.last_kernel_ms()[1], "identical to round 0" if same else "DIFFERENT FROM ROUND 0", len(blob),
                 sum(map(len, blob))), flush=True)
        assert same, "results differ"
