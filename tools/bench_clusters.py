#!/usr/bin/env python
"""
tools/bench_clusters.py — the cluster-extraction path on the GPU (csrc/clusters.hip, structural/cluster_analysis.py).

    python tools/bench_clusters.py [--out profiles/clusters_bench.json] [--reps 20]

1. shell_hits_kernel + shell_sort_kernel (mdhip_shell_members) on a 4 x 4 x 4 replica of frame 50 of mg_tfsi_dme
   (tests/golden/clusters.npz: 670 656 atoms, 2 112 Mg centres, 1.42e9 centre-atom tests): device time of the call
   (both kernels), tests/s, and the fraction of the FP64 VALU issue roof at 15 f64 VALU operations per test
   (3 sub, 3 |d| - L, 3 min, 3 mul, 2 add, 1 compare; the |.| are source modifiers). Roof: 256 CUs x 64 f64 lanes per
   clock x 2.4 GHz = 39.3e12 operations/s (the 78.6 TFLOPS FP64 vector peak counts an FMA as two).
2. End to end, get_clusters (files written) and get_cluster_compositions on case A (frame 50, 33 Mg centres) and on
   100 jittered copies of frame 50 (full_trajectory, 3 300 clusters), next to the numpy restatement of
   tests/cluster_ref.py as the CPU baseline (timed on the first frames of the same trajectory and scaled per frame).
"""

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402

import cluster_ref as R  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402
from mdproptools_amd.io import write_dump  # noqa: E402
from mdproptools_amd.structural import cluster_analysis as CA  # noqa: E402

OPS_PER_TEST = 15
ROOF_OPS = 256 * 64 * 2.4e9


def replica(z, k=4):
    """Frame 50 tiled k x k x k: molecules of one type stay contiguous (every copy of the DME block, then TFSI, Mg)."""
    xyz, L = z["f50_xyz"], z["f50_bounds"][:, 1] - z["f50_bounds"][:, 0]
    mol_of, seg_off, mol_type = R.layout(R.NUM_MOLS, R.NUM_ATOMS)
    shifts = np.array([(i, j, l) for i in range(k) for j in range(k) for l in range(k)], dtype=np.float64) * L
    parts, types, mols = [], [], []
    for t in range(1, 4):
        atoms = np.flatnonzero(mol_type[mol_of] == t)
        for s in shifts:
            parts.append(xyz[:, atoms] + s[:, None])
            types.append(z["f50_type"][atoms])
    big = np.ascontiguousarray(np.concatenate(parts, axis=1))
    nm = [n * k ** 3 for n in R.NUM_MOLS]
    mol_big, _, _ = R.layout(nm, R.NUM_ATOMS)
    return big, L * k, np.concatenate(types), mol_big.astype(np.int32)


def kernel_bench(z, reps):
    xyz, L, types, mol_of = replica(z)
    centres = np.flatnonzero(types == 9).astype(np.int32)
    box = L[None, :]
    ctx = B.default_context()
    B.shell_members(xyz[None], box, centres, mol_of, 2.3 ** 2, ctx=ctx)  # warm-up (staging, code load)
    ms = []
    for _ in range(reps):
        mols, count = B.shell_members(xyz[None], box, centres, mol_of, 2.3 ** 2, ctx=ctx)
        ms.append(ctx.last_kernel_ms())
    tests = float(len(centres)) * xyz.shape[1]
    med = float(np.median(ms))
    return {
        "atoms": int(xyz.shape[1]), "centres": int(len(centres)), "tests_per_frame": tests,
        "kernel_ms_median": med, "kernel_ms_min": float(np.min(ms)), "reps": reps,
        "tests_per_s": tests / (med * 1e-3),
        "fp64_valu_fraction": tests * OPS_PER_TEST / (med * 1e-3) / ROOF_OPS,
        "roof_ms_at_15_ops": tests * OPS_PER_TEST / ROOF_OPS * 1e3,
        "mean_shell_molecules": float(count.mean()),
    }


def jittered_frames(z, n, seed=0):
    rng = np.random.default_rng(seed)
    L = z["f50_bounds"][:, 1] - z["f50_bounds"][:, 0]
    out = []
    for f in range(n):
        xyz = z["f50_xyz"] if f == 0 else np.mod(np.round(z["f50_xyz"] + rng.normal(0, 0.05, z["f50_xyz"].shape), 5)
                                                 - z["f50_bounds"][:, :1], L[:, None]) + z["f50_bounds"][:, :1]
        out.append(dict(ids=z["f50_id"].astype(np.int64), types=z["f50_type"].astype(np.int64), xyz=xyz,
                        force=z["f50_force"], bounds=z["f50_bounds"], timestep=50000 * f))
    return out


def e2e(frames, tmp, full, cpu_frames):
    src = os.path.join(tmp, "dumps")
    os.makedirs(src)
    for fr in frames:
        tab = np.column_stack([fr["ids"], fr["types"], fr["xyz"].T, fr["force"].T])
        write_dump(os.path.join(src, "dump.%d.dump" % fr["timestep"]), fr["timestep"], fr["bounds"], R.DUMP_COLS, tab)
    pattern = os.path.join(src, "dump.*.dump")
    sel = dict(full_trajectory=True) if full else dict(full_trajectory=False, frame=0)
    kw = dict(atom_type=9, r_cut=2.3, num_mols=R.NUM_MOLS, num_atoms_per_mol=R.NUM_ATOMS, max_force=0.75)
    out = os.path.join(tmp, "out")
    res = {}
    for rep in range(2):  # (the first run pays the library load and the first launches)
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        t0 = time.perf_counter()
        n = CA.get_clusters(pattern, elements=R.ELEMENTS, working_dir=out, **sel, **kw)
        t1 = time.perf_counter()
        clusters, _ = CA.get_cluster_compositions(pattern, **sel, **kw)
        t2 = time.perf_counter()
        res = {"frames": len(frames), "clusters": n, "get_clusters_s": t1 - t0, "get_cluster_compositions_s": t2 - t1}
    t0 = time.perf_counter()
    R.get_clusters(frames[:cpu_frames], elements=R.ELEMENTS, **{k: v for k, v in kw.items()})
    res["numpy_restatement_s"] = (time.perf_counter() - t0) * len(frames) / cpu_frames
    res["numpy_restatement_frames_timed"] = cpu_frames
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clusters_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    z = R.load()
    rec = {"device": B.default_context().name, "kernel_replica_4x4x4": kernel_bench(z, a.reps)}
    with tempfile.TemporaryDirectory() as tmp:
        rec["e2e_case_A"] = e2e(jittered_frames(z, 1), os.path.join(tmp, "a"), False, 1)
        rec["e2e_jittered_%d_frames" % a.frames] = e2e(jittered_frames(z, a.frames), os.path.join(tmp, "b"), True, 5)
    txt = json.dumps(rec, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
