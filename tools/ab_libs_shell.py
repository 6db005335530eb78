#!/usr/bin/env python
"""tools/ab_libs_shell.py LIB.so LIB.so [LIB.so ...] — the consumers of csrc/shell_search.h and csrc/shell_gather.h
through several BUILDS of libmdhip.so in one process: hydration_counts and hydration_cosines on the system of
tools/bench_hydration.py, angle_hist on that of tools/bench_angular.py, shell_members on that of tools/bench_clusters.py
and shell_coordination on the same atoms with classes and a pass mask; bond_order on the system of tools/bench_order.py
(the first 20 frames of the first trajectory), contact_components on the two cases of tools/bench_aggregates.py (the
same trajectory; the dense case on its first 100 frames), sdf_hist on the system of tools/bench_sdf.py, hbond_counts
and hbond_lifetime on that of tools/bench_hbonds.py. One round per LIB argument, in the order given (a path may repeat:
P N P N); every output array of a call is compared with the first round's, byte for byte; kernel time per call from
the library's own timer, after a warm-up call, with the repetitions of those tools (10, or 20 for the cluster calls;
--reps-scale multiplies them; --only NAME[,NAME...] runs those calls alone). Two copies of one build under two file
names (P P' P P') give that build's own spread between two contexts of one process."""
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

# tools/bench_order.py: every O a centre, 20 frames; tools/bench_aggregates.py: cations against O, nodes = molecules
xyz_o, box_o = xyz[:20].contiguous(), box[:20]
node_of = np.concatenate([ions, n_cat + np.repeat(np.arange(n_wat), 3)]).astype(np.int32)
zeros_i, zeros_o = np.zeros(n_cat, dtype=np.int32), np.zeros(n_wat, dtype=np.int32)
n_dense = min(100, frames)
xyz_d, box_d = xyz[:n_dense].contiguous(), box[:n_dense]

# tools/bench_sdf.py: 512 three-atom reference molecules, 20 000 observed atoms of two species, 500 frames
s_mols, s_obs, s_box, s_frames = 512, 20000, 50.0, 500
gs = torch.Generator(device="cuda").manual_seed(0)
sxyz = torch.rand((s_frames, 3, 3 * s_mols + s_obs + 2), generator=gs, device="cuda", dtype=torch.float64) * s_box
so = 3 * np.arange(s_mols)
sot = torch.as_tensor(so, device="cuda")
for k in (1, 2):
    sxyz[:, :, sot + k] = sxyz[:, :, sot] + 0.7 * torch.randn((s_frames, 3, s_mols), generator=gs, device="cuda",
                                                              dtype=torch.float64)
sbox = np.full((s_frames, 3), s_box)
scand = np.arange(3 * s_mols, 3 * s_mols + s_obs)
scls = (scand % 2).astype(np.int32)

# tools/bench_hbonds.py: 3000 waters that stay in place, 1000 frames
W, HF = 3000, 1000
HL = (W / 0.0334) ** (1.0 / 3.0)
gh = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *s: torch.randn(s, generator=gh, device="cuda", dtype=torch.float64)  # noqa: E731
place = torch.rand((1, 3, W), generator=gh, device="cuda", dtype=torch.float64) * HL
hxyz = torch.empty((HF, 3, 3 * W), device="cuda", dtype=torch.float64)
hxyz[:, :, 0::3] = place + 0.1 * rnd(HF, 3, W)
for h in (1, 2):
    u = rnd(1, 3, W) + 0.25 * rnd(HF, 3, W)
    hxyz[:, :, h::3] = hxyz[:, :, 0::3] + 0.96 * u / u.norm(dim=1, keepdim=True)
hbox = np.full((HF, 3), HL)
ho = (3 * np.arange(W)).astype(np.int32)
h_off = (2 * np.arange(W + 1)).astype(np.int32)
h_atoms = np.stack([ho + 1, ho + 2], axis=1).ravel().astype(np.int32)
hzeros = np.zeros(W, dtype=np.int32)
hmol = (np.arange(3 * W) // 3).astype(np.int32)
hr2, hcut = 3.5 ** 2, float(np.cos(np.radians(150.0)))


def arrays(out):
    """The arrays of a result that is a dict (bond_order) or holds plain integers (sdf_hist, the hydrogen-bond calls)"""
    vals = [out[k] for k in sorted(out)] if isinstance(out, dict) else list(out)
    return [np.asarray(v) for v in vals if v is not None]


CALLS = [
    ("hydration_counts", 10, lambda c: B.hydration_counts(xyz, box, ions, o, 3.5 ** 2, -0.72, 0.02, 100, ctx=c)),
    ("hydration_cosines", 10, lambda c: B.hydration_cosines(xyz, box, ions, o, 3.5 ** 2, cap=32, ctx=c)),
    ("angle_hist", 10, lambda c: B.angle_hist(xyz, box, types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges, ctx=c)[:3]),
    ("shell_members", 20, lambda c: B.shell_members(cxyz[None], cL[None, :], centres, cmol, 2.3 ** 2, ctx=c)),
    ("shell_coordination", 20, lambda c: B.shell_coordination(cxyz[None], cL[None, :], centres, cmol, seg_off, mol_type,
                                                              cls, 2.3 ** 2, 2.0 ** 2, passes=passes, ctx=c)),
    ("bond_order", 10, lambda c: arrays(B.bond_order(xyz_o, box_o, types, 2, [2], 3.5 ** 2, degrees=(4, 6),
                                                     tetrahedral=True, ctx=c))),
    ("sdf_hist", 10, lambda c: arrays(B.sdf_hist(sxyz, sbox, so, so + 1, so + 2, scand, scls, 2, 9.0, 0.5, ctx=c))),
    ("contact_components", 10, lambda c: B.contact_components(xyz, box, ions, zeros_i, o, zeros_o, [[3.5 ** 2]],
                                                              node_of, n_cat + n_wat, ctx=c)),
    ("contact_components/dense", 10, lambda c: B.contact_components(xyz_d, box_d, ions, zeros_i, o, zeros_o,
                                                                    [[12.0 ** 2]], node_of, n_cat + n_wat, ctx=c)),
    ("hbond_counts", 10, lambda c: arrays(B.hbond_counts(hxyz, hbox, ho, hzeros, h_off, h_atoms, ho, hzeros, hr2, hcut,
                                                         cos_edges=edges, mol_of=hmol, ctx=c))),
    ("hbond_lifetime", 10, lambda c: arrays(B.hbond_lifetime(hxyz, hbox, ho, h_off, h_atoms, ho, hr2, hcut, mol_of=hmol,
                                                             ctx=c))),
]

if only is not None:
    CALLS = [c for c in CALLS if c[0] in only]

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
        print("round %d %-22s %-24s median %8.4f ms  min %8.4f  max %8.4f  aux median %7.4f  (%s, %d arrays, %d bytes)"
              % (rnd, os.path.basename(p), name, np.median(ms), ms.min(), ms.max(), np.median(aux),
                 "identical to round 0" if same else "DIFFERENT FROM ROUND 0", len(blob), sum(map(len, blob))),
              flush=True)
        assert same, "results differ"
