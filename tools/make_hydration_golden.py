#!/usr/bin/env python
"""
tools/make_hydration_golden.py — tests/golden/hydration.npz from the REAL reference's get_hydration_number.

Build container only (the reference is not on the GPU box; what travels is this script's output, as data):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_hydration_golden.py

The reference module is imported read-only with the stand-ins of oracle/shims (oracle/shims/README.md) and its own
directory on sys.path (its bare `from rdf_cn import`). Frame 50 and the case-D sub-system come from
tests/golden/clusters.npz and are not stored again.

Cases (tests/hydration_ref.py CASES):
  mg_dme   frame 50, Mg (type 3) against DME (type 1), r_cut 4.0
  mg_tfsi  frame 50, Mg against TFSI (type 2), r_cut 8.0
  sub_dme  the 12-frame case-D sub-system, Mg against DME, r_cut 6.0
  box      3 seeded frames of 20 ions and 600 3-site waters: an ion on an O (NaN cosine), an O at exactly r_cut, a
           water whose H1 lies across the boundary
  zero     the same frames at r_cut 0.5: an ion without water (ZeroDivisionError)
"""

import os
import sys
import tempfile

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
sys.path[:0] = [os.path.join(REPO, "oracle", "shims"), REPO, os.path.join(REPO, "tests"),
                os.path.join(REF, "mdproptools", "structural")]

import numpy as np  # noqa: E402

import hydration_number as ref  # noqa: E402  (the reference module)
import hydration_ref as R  # noqa: E402

OUT = os.environ.get("MDHIP_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden", "hydration.npz")
N_ION, N_WAT, L_BOX, N_FRAMES = 20, 600, 20.0, 3


def box_frames():
    rng = np.random.default_rng(20261016)
    n = N_ION + 3 * N_WAT
    frames = []
    for f in range(N_FRAMES):
        xyz = np.round(rng.uniform(0, L_BOX, (3, n)), 4)
        o = N_ION + 3 * np.arange(N_WAT)
        for h in (1, 2):  # hydrogens about 1 A from their O, raw coordinates (may lie outside the box)
            xyz[:, o + h] = np.round(xyz[:, o] + rng.normal(0, 0.6, (3, N_WAT)), 4)
        xyz[:, 0] = xyz[:, o[0]]  # ion 0 on the O of water 0: a zero vector, NaN
        xyz[:, 1] = [5.0, 5.0, 5.0]  # water 1's O at exactly r_cut = 3.5 from ion 1: excluded
        xyz[:, o[1]] = [8.5, 5.0, 5.0]
        xyz[:, 2] = [1.0, 10.0, 10.0]  # water 2 across the x boundary
        xyz[:, o[2]] = [0.05, 10.0, 10.0]
        xyz[:, o[2] + 1] = [19.95, 10.0, 10.8]
        xyz[:, o[2] + 2] = [0.6, 10.5, 10.0]
        frames.append(dict(ids=np.arange(1, n + 1), types=np.r_[np.ones(N_ION), np.full(3 * N_WAT, 2)].astype(np.int64),
                           xyz=xyz, bounds=np.array([[0.0, L_BOX]] * 3), timestep=1000 * f))
    return frames


def run_ref(frames, **kw):
    with tempfile.TemporaryDirectory() as wd:
        pattern = R.write_dumps(frames, wd)
        try:
            df = ref.get_hydration_number(pattern, working_dir=wd, **kw)
        except Exception as e:  # noqa: BLE001  (recorded: the drop-in must raise the same type)
            return None, None, type(e).__name__
        with open(os.path.join(wd, "angles_df.csv"), "rb") as fh:
            return df, fh.read(), ""


def main():
    z = dict(np.load(R.CLUSTERS))
    z = {"c_" + k: v for k, v in z.items() if k.startswith(("f50_", "d_"))}
    frames = box_frames()
    store = {"box_xyz": np.stack([f["xyz"] for f in frames]), "box_bounds": np.stack([f["bounds"] for f in frames]),
             "box_timestep": np.array([f["timestep"] for f in frames], dtype=np.int64),
             "box_type": frames[0]["types"].astype(np.int8), "box_num_mols": np.array([N_ION, N_WAT], dtype=np.int64)}
    z.update(store)
    for key in R.CASES:
        fr, kw = R.case_args(z, key)
        df, csv, err = run_ref(fr, **kw)
        store[key + "_error"] = np.array(err)
        if err:
            print(key, "raises", err)
            continue
        store[key + "_csv"] = np.frombuffer(csv, dtype=np.uint8)
        store[key + "_cos"] = df["angles_distribution"].to_numpy()
        store[key + "_factor"] = np.float64(df["hydration_factor"].iloc[0])
        print(key, len(df), "cosines, factor", df["hydration_factor"].iloc[0], "NaN:",
              int(np.isnan(store[key + "_cos"]).sum()))
    assert store["zero_error"] == "ZeroDivisionError" and not any(store[k + "_error"] for k in R.CASES if k != "zero")
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
