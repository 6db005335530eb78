"""
Cation-water orientation from LAMMPS dumps — drop-in for get_hydration_number of
the reference's structural/hydration_number.py:13-99 (same signature, defaults, CSV and return value), plus
calc_hydration_orientation, which counts the same cosines per cation and bins them without keeping them.

What runs where
  GPU (libmdhip.so, csrc/hydration.hip): every cation atom of a batch of frames against the O of every water with the
      reference's single-wrap rsq, and the cosine between the wrapped cation - O vector and the water's
      (H1 + H2) - 2 O vector (hydration_number.py:17-32, 69-71).
  Host (numpy, this file): parsing (the native reader), the molecule layout, the factors and the DataFrame.

The reference's per-cation pandas merges come down to these rules, reproduced exactly:
  * molecule types are 1-based indices over num_mols / num_atoms_per_mol in id order; every atom of a cation-type
    molecule is a cation; a water's O is its first atom, H1 and H2 the next two;
  * within a frame, cations in id order, and per cation the waters within r_cut in ascending molecule order;
  * per cation len(cos[cos < -0.72]) / len(cos) (ZeroDivisionError for a cation without water); per frame those
    summed left to right from 0 and divided by the cation count; overall the per-frame values summed with sum() in
    frame order and divided by the frame count;
  * angles_df.csv in working_dir, with the index; alter_atom_ids changes nothing (the reference recomputes a column
    it never reads); progress lines only with VERBOSE.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import molecule_layout
from ..common.trajectory import frame_batches

VERBOSE = False
COS_CUT = -0.72  # hydration_number.py:35
MAX_BATCH_BYTES = 1 << 28  # coordinates of the frames handed to the GPU in one call
_COLS = ["id", "x", "y", "z"]  # the planes of a batch


def _layout(cation_type, water_type, num_mols, num_atoms_per_mol):
    """(number of atoms, cation atom indices, first-atom index of every water) of the id-ordered molecule layout."""
    if num_mols is None or num_atoms_per_mol is None:
        raise ValueError("num_mols and num_atoms_per_mol are required (the molecule layout in id order)")
    seg_off, mol_type, _ = molecule_layout(num_mols, num_atoms_per_mol)
    sizes = np.diff(seg_off)
    atom_type = np.repeat(mol_type, sizes)
    cations = np.flatnonzero(atom_type == cation_type).astype(np.int32)
    water_mols = np.flatnonzero(mol_type == water_type)
    if len(water_mols) and int(sizes[water_mols[0]]) < 3:
        raise ValueError("a water molecule needs at least 3 atoms (O, H1, H2); type %d has %d"
                         % (water_type, int(sizes[water_mols[0]])))
    return int(seg_off[-1]), cations, seg_off[water_mols].astype(np.int32)


def _xyz(planes):
    return np.ascontiguousarray(planes[:, 1:4])


def get_hydration_number(dump_pattern, cation_type, water_type, r_cut, alter_atom_ids=False, num_mols=None,
                         num_atoms_per_mol=None, working_dir=None):
    """
    The cosines between every cation - water O vector within r_cut and the water's (H1 + H2) - 2 O vector, in frame,
    cation and water order, and the hydration factor (the mean over frames of the mean over cations of the fraction
    with cos < -0.72). Writes angles_df.csv to `working_dir` (default: the current directory) and returns the
    DataFrame (columns angles_distribution, hydration_factor). Arguments as in the reference.
    """
    if not working_dir:
        working_dir = os.getcwd()
    n_atoms, cations, waters = _layout(cation_type, water_type, num_mols, num_atoms_per_mol)
    rc2 = r_cut ** 2  # hydration_number.py:20
    cosines, factors = [], []
    for steps, boxes, planes in frame_batches(os.path.join(working_dir, dump_pattern), _COLS, MAX_BATCH_BYTES, n_atoms):
        _, cos, count = backend.hydration_cosines(_xyz(planes), boxes, cations, waters, rc2)
        for j in range(len(planes)):
            if VERBOSE:
                print(len(factors))
            factor = 0
            for c in range(len(cations)):
                row = cos[j, c, :count[j, c]]
                cosines.append(row)
                factor += len(row[row < COS_CUT]) / len(row)  # ZeroDivisionError for a cation without water
            factors.append(factor / len(cations))  # ZeroDivisionError without cations
    angles_df = pd.DataFrame(np.concatenate(cosines) if cosines else [], columns=["angles_distribution"])
    angles_df["hydration_factor"] = sum(factors) / len(factors)
    angles_df.to_csv(os.path.join(working_dir, "angles_df.csv"))
    return angles_df


def calc_hydration_orientation(filename, cation_type, water_type, r_cut, num_mols, num_atoms_per_mol,
                               cos_bin_size=0.02, cos_cut=COS_CUT):
    """
    The counts behind get_hydration_number without keeping the cosines.

    Returns (per_cation, distribution):
      per_cation: one row per (frame, cation) — frame (index), timestep, cation_id, n_water (waters within r_cut),
        n_away (those with cos < cos_cut) and factor = n_away / n_water (NaN for a cation without water);
      distribution: cos bin centre, count and fraction of all binned cosines, bins of width cos_bin_size from -1
        (int(2 / cos_bin_size) bins; bin trunc((cos + 1) / w), the last one closed; NaN cosines in none).
    """
    n_atoms, cations, waters = _layout(cation_type, water_type, num_mols, num_atoms_per_mol)
    w = float(cos_bin_size)
    n_bins = int(2 / w)
    hist = np.zeros(n_bins, dtype=np.uint64)
    meta, nw, na = [], [], []
    index = 0
    for steps, boxes, planes in frame_batches(filename, _COLS, MAX_BATCH_BYTES, n_atoms):
        n_water, n_away, h = backend.hydration_counts(_xyz(planes), boxes, cations, waters, r_cut ** 2, cos_cut, w,
                                                      n_bins)
        hist += h
        for j, ts in enumerate(steps):
            ids = planes[j][0][cations].astype(np.int64)
            meta += [(index, ts, int(i)) for i in ids]
            index += 1
        nw.append(n_water.ravel())
        na.append(n_away.ravel())
    per_cation = pd.DataFrame(meta, columns=["frame", "timestep", "cation_id"])
    per_cation["n_water"] = np.concatenate(nw).astype(np.int64) if nw else np.zeros(0, dtype=np.int64)
    per_cation["n_away"] = np.concatenate(na).astype(np.int64) if na else np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_cation["factor"] = np.where(per_cation["n_water"] > 0, per_cation["n_away"] / per_cation["n_water"],
                                        np.nan)
    total = int(hist.sum())
    distribution = pd.DataFrame({"cos": -1.0 + (np.arange(n_bins) + 0.5) * w, "count": hist.astype(np.int64)})
    distribution["fraction"] = distribution["count"] / total if total else np.nan
    return per_cation, distribution
