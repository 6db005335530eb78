#!/usr/bin/env python
"""
tools/make_cluster_golden.py — tests/golden/clusters.npz from the REAL reference's get_clusters.

Build container only (the reference is not on the GPU box; what travels is this script's output, as data):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_cluster_golden.py

The reference is imported read-only with the stand-ins of oracle/shims (oracle/shims/README.md). Before anything is
saved, case A is checked byte for byte against the reference's own committed test outputs
(tests/structural/test_files/Cluster_0_*.xyz upstream).

Cases (frame 50 of the mg_tfsi_dme trajectory is dump.nvt.2500000.dump; elements O C H N S O C F Mg):
  A  frame 50, atom_type 9, r_cut 2.3, max_force 0.75 (upstream test_get_clusters)
  B  frame 50, alter_atom_types, atom_type 32 (the get_clusters call of upstream test_get_unique_configurations)
  C  frame 50, atom_type 9, r_cut 2.3, max_force -0.01 (about half the molecules fail the force filter)
  D  full_trajectory over a 12-frame sub-system (whole molecules around five Mg ions), r_cut 6.0, max_force 0.3
"""

import glob
import os
import sys
import tempfile

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
sys.path[:0] = [os.path.join(REPO, "oracle", "shims"), REPO, REF]

import numpy as np  # noqa: E402

from mdproptools.structural.cluster_analysis import get_clusters as ref_get_clusters  # noqa: E402
from pymatgen.io.lammps.outputs import parse_lammps_dumps  # noqa: E402  (the shim)

from mdproptools_amd.io import write_dump  # noqa: E402

DATA = os.path.join(REF, "data", "mg_tfsi_dme")
UPSTREAM = os.path.join(REF, "tests", "structural", "test_files")
OUT = os.environ.get("MDHIP_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden", "clusters.npz")
ELEMENTS = ["O", "C", "H", "N", "S", "O", "C", "F", "Mg"]
NUM_MOLS = [591, 66, 33]
NUM_ATOMS = [16, 15, 1]
COLS = ["id", "type", "x", "y", "z", "fx", "fy", "fz"]
SUB_FRAMES = 12
SUB_MG = 5
SUB_RADIUS = 5.0  # molecules with an atom this close to one of the chosen Mg in the first frame join the sub-system


def run_ref(pattern, **kw):
    with tempfile.TemporaryDirectory() as wd:
        n = ref_get_clusters(filename=pattern, elements=ELEMENTS, working_dir=wd, **kw)
        files = {}
        for p in sorted(glob.glob(os.path.join(wd, "Cluster_*.xyz"))):
            with open(p, "rb") as fh:
                files[os.path.basename(p)] = fh.read()
    return n, files


def pack(store, key, n, files):
    names = sorted(files)
    blobs = [files[k] for k in names]
    store[key + "_names"] = np.array(names)
    store[key + "_blob"] = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    store[key + "_off"] = np.concatenate(([0], np.cumsum([len(b) for b in blobs]))).astype(np.int64)
    store[key + "_return"] = np.int64(n)


def frame_arrays(dump):
    df = dump.data.sort_values(by=["id"])
    return df[COLS].to_numpy(dtype=np.float64), np.asarray(dump.box.bounds, dtype=np.float64)


def main():
    pattern = os.path.join(DATA, "dump.nvt.*.dump")
    dumps = list(parse_lammps_dumps(pattern))
    assert dumps[50].timestep == 2500000, dumps[50].timestep
    store = {}

    # frame 50 inputs
    t50, b50 = frame_arrays(dumps[50])
    store["f50_id"] = t50[:, 0].astype(np.int32)
    store["f50_type"] = t50[:, 1].astype(np.int8)
    store["f50_xyz"] = np.ascontiguousarray(t50[:, 2:5].T)
    store["f50_force"] = np.ascontiguousarray(t50[:, 5:8].T)
    store["f50_bounds"] = b50
    store["f50_timestep"] = np.int64(dumps[50].timestep)
    assert np.array_equal(store["f50_id"], np.arange(1, len(t50) + 1))

    base = dict(num_mols=NUM_MOLS, num_atoms_per_mol=NUM_ATOMS, full_trajectory=False, frame=50)
    n, files = run_ref(pattern, atom_type=9, r_cut=2.3, max_force=0.75, alter_atom_types=False, **base)
    upstream = {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(UPSTREAM, "Cluster_0_*.xyz"))}
    assert n == 33 and files == upstream, "case A differs from the upstream Cluster_0_*.xyz files"
    pack(store, "A", n, files)
    n, files = run_ref(pattern, atom_type=32, r_cut=2.3, max_force=0.75, alter_atom_types=True, **base)
    pack(store, "B", n, files)
    n, files = run_ref(pattern, atom_type=9, r_cut=2.3, max_force=-0.01, alter_atom_types=False, **base)
    pack(store, "C", n, files)

    # D: whole molecules around SUB_MG Mg ions, the first SUB_FRAMES frames
    sizes = np.repeat(NUM_ATOMS, NUM_MOLS)
    seg = np.concatenate(([0], np.cumsum(sizes)))
    mtype = np.repeat(np.arange(3), NUM_MOLS)
    t0, b0 = frame_arrays(dumps[0])
    L = b0[:, 1] - b0[:, 0]
    mg = np.flatnonzero(mtype == 2)[:SUB_MG]
    keep = []
    for m in range(len(sizes)):
        a = t0[seg[m]:seg[m + 1], 2:5]
        near = False
        for g in mg:
            d = a - t0[seg[g], 2:5]
            d -= np.round(d / L) * L
            near |= bool((np.sqrt((d ** 2).sum(axis=1)) < SUB_RADIUS).any())
        if near or m in mg:
            keep.append(m)
    keep = np.array(keep)
    rows = np.concatenate([np.arange(seg[m], seg[m + 1]) for m in keep])
    sub_mols = [int((mtype[keep] == t).sum()) for t in range(3)]
    sub = []
    with tempfile.TemporaryDirectory() as wd:
        for f in range(SUB_FRAMES):
            tab, bnd = frame_arrays(dumps[f])
            tab = tab[rows].copy()
            tab[:, 0] = np.arange(1, len(rows) + 1)
            sub.append(tab)
            write_dump(os.path.join(wd, "sub.%d.dump" % dumps[f].timestep), dumps[f].timestep, bnd, COLS, tab)
            store.setdefault("d_bounds", []).append(bnd)
            store.setdefault("d_timestep", []).append(dumps[f].timestep)
        n, files = run_ref(os.path.join(wd, "sub.*.dump"), atom_type=9, r_cut=6.0, num_mols=sub_mols,
                           num_atoms_per_mol=NUM_ATOMS, full_trajectory=True, max_force=0.3)
    sub = np.stack(sub)
    store["d_type"] = sub[0, :, 1].astype(np.int8)
    assert all(np.array_equal(s[:, 1], sub[0, :, 1]) for s in sub)
    store["d_xyz"] = np.ascontiguousarray(sub[:, :, 2:5].transpose(0, 2, 1))
    store["d_force"] = np.ascontiguousarray(sub[:, :, 5:8].transpose(0, 2, 1))
    store["d_bounds"] = np.array(store["d_bounds"])
    store["d_timestep"] = np.array(store["d_timestep"], dtype=np.int64)
    store["d_num_mols"] = np.array(sub_mols, dtype=np.int64)
    pack(store, "D", n, files)

    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; D:", sub_mols, "molecules,", n, "clusters")


if __name__ == "__main__":
    main()
