#!/usr/bin/env python
"""tools/drain_trace.py [C2|C1] — how long the CUs empty out at the end of the persistent pair sweep.

Builds a variant of the library whose scalar-j kernel records, per block, when it started, when each of its waves ran
dry and when it flushed (pair_sj.hip, -DPAIR_DRAIN_TRACE; tools/_bin/libmdhip_drain.so — never the library's own
build), runs the synchronous C2 call through it and prints, for the last launch:

  span          first block start -> last block flush
  drain         first wave dry (anywhere on the chip) -> last block flush: from here on the chip is no longer full
  idle share    wave-time between a wave's running dry and the launch's end, as a share of all wave-time of the launch
                — what a second launch on the device could at most fill — split into the part a block's dry waves
                spend waiting for the block's last wave (their LDS and registers stay held) and the part after the flush
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mdproptools_amd import _lib, build  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd import synth  # noqa: E402

WORDS, TICK_US = 18, 0.01  # words per block; the wall clock runs at 100 MHz

which = sys.argv[1] if len(sys.argv) > 1 else "C2"
path = os.path.join(build.VARIANT_DIR, "libmdhip_drain.so")
if not os.path.exists(path):  # (build it where there is a compiler; it travels with the tree)
    path = build.build_variant("drain", "pair_sj.hip", ["-DPAIR_DRAIN_TRACE"])
_lib.LIB_PATH = os.path.abspath(path)
ctx = _lib.Context(0)
ctx.lib.mdhip_drain_trace.restype = C.c_int
ctx.lib.mdhip_drain_trace.argtypes = [C.c_void_p, C.c_int]

cfg = synth.rdf_config(which)
n, L, F = cfg["n_atoms"], cfg["box_len"], cfg["n_frames"]
xyz = torch.from_numpy(synth.rdf_frames(n, range(F), L, cfg["seed_offset"])).cuda()
ty = synth.rdf_types(n) if which == "C2" else synth.c1_types(False)
rel = np.array(synth.ALL_PAIRS_4 if which == "C2" else synth.C1_RELATIONS)
box = np.full((F, 3), L)
nb = int(cfg["r_cut"] / cfg["bin_size"])
for rep in range(4):
    trace = np.zeros((4096, WORDS), dtype=np.uint64)
    B.rdf_loop(xyz, ty, box, rel, cfg["r_cut"], cfg["bin_size"], nb, per_frame=False, ctx=ctx)
    ms, launches = ctx.last_kernel_ms()
    assert ctx.lib.mdhip_drain_trace(trace.ctypes.data, 4096) == 0
    t = trace.astype(np.int64)
    # blocks of the last launch: the device buffer is never cleared, so rows of earlier launches (3 ms or more older)
    # may be left where this launch had fewer blocks — a launch's blocks all start within a few tens of microseconds
    t0 = t[:, 0].max() - int(500 / TICK_US)
    used = (t[:, 0] >= t0) & (t[:, 1] >= t0)
    t = t[used]
    waves = t[:, 2:]
    waves = np.where(waves >= t0, waves, 0)
    has = waves > 0
    start, flush = t[:, 0], t[:, 1]
    end = flush.max()
    first_dry = waves[has].min()
    span = (end - start.min()) * TICK_US
    drain = (end - first_dry) * TICK_US
    held = ((flush[:, None] - waves) * has).sum()        # a dry wave waiting for its block's last wave
    after = ((end - flush[:, None]) * has).sum()         # ... and from the block's flush to the end of the launch
    total = float(has.sum()) * (end - start.min())
    q = np.percentile((end - flush) * TICK_US, [50, 90, 99])
    print("%s run %d: %s, %d launch(es), %.3f ms by events; %d blocks, %d waves" % (which, rep, ctx.last_kernel_name(), launches, ms, len(t), int(has.sum())))
    print("  span %.1f us   block starts spread over %.1f us   drain (first dry wave -> last flush) %.1f us" % (span, (start.max() - start.min()) * TICK_US, drain))
    print("  idle wave-time %.2f %% of the launch (= %.1f us of the whole chip): %.2f %% held behind a block's last wave, %.2f %% after the flush"
          % (100.0 * (held + after) / total, (held + after) / total * span, 100.0 * held / total, 100.0 * after / total))
    print("  block flush before the launch's end: median %.1f us, 90 %% %.1f us, 99 %% %.1f us" % (q[0], q[1], q[2]))
ctx.close()
