#!/usr/bin/env python
"""tools/lane_probe.py — is a kernel from ANOTHER stream placed while the persistent pair sweep runs?

Issues the asynchronous C2 call, and 0.8 ms into its 2.6 ms sweep launches a one-block kernel (a 64-element add, or a
64-element copy from page-locked host memory) on a stream of torch's own; prints the time from that launch to its
completion, against the same launch on an idle device. Then two calls back to back: when each completes."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from mdproptools_amd import backend as B, synth
from mdproptools_amd._lib import Context
cfg = synth.rdf_config("C2"); n, L, F = cfg["n_atoms"], cfg["box_len"], cfg["n_frames"]
xyz = torch.from_numpy(synth.rdf_frames(n, range(F), L, cfg["seed_offset"])).cuda()
ty = synth.rdf_types(n); rel = np.array(synth.ALL_PAIRS_4); box = np.full((F, 3), L)
ctx = Context(0)
def issue(): return B.rdf_loop(xyz, ty, box, rel, 20.0, 0.05, 400, per_frame=False, ctx=ctx, async_=True)
for _ in range(6): issue().wait()
side = torch.cuda.Stream()
t = torch.zeros(64, device="cuda")
pin = torch.zeros(64, pin_memory=True)
with torch.cuda.stream(side):
    for _ in range(5): t.add_(1.0)
torch.cuda.synchronize()
def tiny(kind):
    e = torch.cuda.Event()
    with torch.cuda.stream(side):
        if kind == "add": t.add_(1.0)
        else: t.copy_(pin, non_blocking=True)
        e.record()
    return e
for kind in ("add", "h2d"):
    for busy in (False, True):
        lat = []
        for rep in range(5):
            h = issue() if busy else None
            if busy: time.sleep(0.0008)   # well inside the 2.6 ms sweep
            t0 = time.perf_counter(); e = tiny(kind)
            while not e.query(): pass
            lat.append((time.perf_counter() - t0) * 1e6)
            if h: h.wait()
        print("tiny %s kernel on another stream, sweep %s: issue->done us %s" % (kind, "running" if busy else "idle", " ".join("%.0f" % v for v in lat)), flush=True)
# two calls in flight: when does the second complete relative to the first
for rep in range(3):
    t0 = time.perf_counter(); h0 = issue(); h1 = issue(); h0.wait(); t1 = time.perf_counter(); h1.wait(); t2 = time.perf_counter()
    print("two calls: first done %.0f us, second done %.0f us after issue" % ((t1 - t0) * 1e6, (t2 - t0) * 1e6))
ctx.close()
