"""
Per-centre order parameters from LAMMPS dumps: the Steinhardt bond-orientational order parameters q_l of a centre's
shell (octahedral against tetrahedral coordination of a cation, a crystallising salt against its melt), the
Lechner-Dellago averaged qbar_l, and the tetrahedral order parameter q_tet of water with its translational companion
s_k. The reference has no such function; DESIGN.md (order parameters) holds the specification, and tests/order_ref.py
restates it in numpy.

What runs where
  GPU (libmdhip.so, csrc/bond_order.hip): per frame and centre the shell search, the selection of the nearest
      neighbours, the spherical harmonics and their sums in ascending atom index, q_l, q_tet and s_k per row, and the
      second pass over the neighbours' q_lm for qbar_l.
  Host (numpy, this file): parsing (the native reader), the atom types and the molecule layout, the binning of the
      per-centre values, the summary and the DataFrames.

The neighbours of a centre are the atoms of `neighbour_types` at rsq < r_cut**2 (the single-wrap rsq of the RDF
functions, strict), with `n_nearest` the k smallest by (rsq, atom index). q_lm is the mean of Y_lm over the neighbour
directions, q_l = sqrt(4 pi / (2l + 1) sum_m |q_lm|**2); qbar_l is the same of q_lm averaged over the centre and its
neighbours; q_tet = 1 - 3/8 sum_{j<k} (cos_jk + 1/3)**2 and s_k = 1 - 1/3 sum_k (r_k - rbar)**2 / (4 rbar**2) over the
four nearest. A row with too few neighbours is short, one with a neighbour ON the centre degenerate: both give NaN and
are counted in the summary.

Out of scope: the Wigner-3j invariants w_l, triclinic boxes, and sharding over torch.distributed.
"""

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import atom_molecules
from ..common.tables import density, write_csv
from ..common.trajectory import refuse_triclinic, typed_batches
from ..dist import is_writer


def _bin_counts(v, lo, bin_size, n_bins):
    """int64 [n_bins]: bin m holds m * bin_size <= v - lo < (m + 1) * bin_size, the last bin closed at the top (a value
    an ulp outside the range falls in the first or last bin); NaN in no bin."""
    v = v[~np.isnan(v)]
    m = np.clip(np.floor((v - lo) / bin_size).astype(np.int64), 0, n_bins - 1)
    return np.bincount(m, minlength=n_bins).astype(np.int64)


def calc_order_parameters(r_cut, centre_type, neighbour_types, filename, degrees=(4, 6), n_nearest=None,
                          averaged=False, tetrahedral=False, num_mols=None, num_atoms_per_mol=None,
                          exclude_same_molecule=False, bin_size=0.01, path_or_buff="order.csv", save_mode=True,
                          per_centre=False):
    """
    Order parameters of the atoms of `centre_type` from their neighbours of `neighbour_types` (atom types; with num_mols
    and num_atoms_per_mol the altered types of calc_atomic_rdf: the index of an atom inside its molecule type) within
    r_cut, over the frames of `filename` (dump file or '*' pattern). degrees: the l of q_l (1..12, at most 4, distinct);
    n_nearest: only the k nearest neighbours by (distance, atom index); averaged: also qbar_l (needs neighbour_types ==
    [centre_type]); tetrahedral: also q_tet and s_k of the four nearest; exclude_same_molecule leaves out neighbours of
    the centre's own molecule (needs the layout).

    Returns (dist, summary), with per_centre (dist, summary, values):
      dist: `value` (bin centres; bins of bin_size over [0, 1], over [-3, 1] with tetrahedral) and per quantity
        `p_<name>` = count / (count.sum() * bin_size) (NaN without counts) and `count_<name>` (int64); names q4, q6, ...,
        qbar4, ..., q_tet, s_k; written to `path_or_buff`;
      summary: one row per quantity: name, n_values, n_short, n_degenerate, mean, std;
      values: name -> float64 [F, C] (NaN where a row is short or degenerate) and `centres` [C] (atom indices).
    """
    deg = [int(l) for l in degrees]
    if len(deg) > backend.BOND_MAX_DEGREES:
        raise ValueError("at most %d degrees per call (%d given)" % (backend.BOND_MAX_DEGREES, len(deg)))
    if any(not 1 <= l <= backend.BOND_MAX_L for l in deg):
        raise ValueError("degrees must be in [1, %d]" % backend.BOND_MAX_L)
    if len(set(deg)) != len(deg):
        raise ValueError("degrees must be distinct")
    if not deg and not tetrahedral:
        raise ValueError("nothing to compute: no degrees and tetrahedral=False")
    nb_types = [int(t) for t in np.atleast_1d(neighbour_types)]
    if averaged and (not deg or sorted(set(nb_types)) != [int(centre_type)]):
        raise ValueError("averaged needs degrees and neighbour_types == [centre_type]: a neighbour's q_lm is a centre's")
    if n_nearest is not None and not 1 <= int(n_nearest) <= backend.BOND_MAX_CAP:
        raise ValueError("n_nearest must be in [1, %d]" % backend.BOND_MAX_CAP)
    bin_size = float(bin_size)
    if not bin_size > 0.0:
        raise ValueError("bin_size must be positive")
    layout = num_mols is not None and num_atoms_per_mol is not None
    altered = bool(num_mols and num_atoms_per_mol)
    if exclude_same_molecule and not layout:
        raise ValueError("exclude_same_molecule needs num_mols and num_atoms_per_mol (the molecule layout in id order)")
    mol_of = atom_molecules(num_mols, num_atoms_per_mol)[1] if layout else None  # (a bad layout raises here)
    refuse_triclinic(filename)

    B = backend
    names = ["q%d" % l for l in deg] + (["qbar%d" % l for l in deg] if averaged else []) \
        + (["q_tet", "s_k"] if tetrahedral else [])
    # per quantity: where it lives in bond_order's dict, and its short and degenerate bits
    where = [("q", d, B.BOND_Q_SHORT, B.BOND_Q_DEGENERATE) for d in range(len(deg))]
    if averaged:
        where += [("qbar", d, B.BOND_QBAR_SHORT, 0) for d in range(len(deg))]  # (every NaN qbar counts as short)
    if tetrahedral:
        where += [("tet", d, B.BOND_TET_SHORT, B.BOND_TET_DEGENERATE) for d in range(2)]
    chunks = {name: [] for name in names}
    n_short, n_degen = np.zeros(len(names), dtype=np.int64), np.zeros(len(names), dtype=np.int64)
    types, centres = None, np.zeros(0, dtype=np.int32)
    for steps, boxes, xyz, types in typed_batches(filename, num_mols, num_atoms_per_mol, altered):
        out = B.bond_order(xyz, boxes, types, int(centre_type), nb_types, backend.cutoff_sq(r_cut), degrees=deg,
                           n_nearest=n_nearest, averaged=averaged, tetrahedral=tetrahedral,
                           mol_of=mol_of if exclude_same_molecule else None)
        centres = out["centres"]
        for k, (name, (key, d, short, degen)) in enumerate(zip(names, where)):
            chunks[name].append(np.asarray(out[key][:, :, d], dtype=np.float64))
            n_short[k] += int(np.count_nonzero(out["flags"] & short))
            n_degen[k] += int(np.count_nonzero(out["flags"] & degen))

    lo = -3.0 if tetrahedral else 0.0
    n_bins = max(1, int(np.ceil((1.0 - lo) / bin_size - 1e-9)))
    dist = pd.DataFrame({"value": lo + (np.arange(n_bins) + 0.5) * bin_size})
    values, rows = {}, []
    for k, name in enumerate(names):
        v = np.concatenate(chunks[name]) if chunks[name] else np.zeros((0, len(centres)))
        values[name] = v
        cnt = _bin_counts(v.ravel(), lo, bin_size, n_bins)
        total = int(cnt.sum())
        dist["p_" + name] = density(cnt, bin_size)
        dist["count_" + name] = cnt
        good = v[~np.isnan(v)]
        rows.append((name, total, int(n_short[k]), int(n_degen[k]), float(good.mean()) if total else np.nan,
                     float(good.std()) if total else np.nan))
    summary = pd.DataFrame(rows, columns=["name", "n_values", "n_short", "n_degenerate", "mean", "std"])
    if save_mode and is_writer():
        write_csv(dist, path_or_buff)
    if per_centre:
        values["centres"] = np.asarray(centres)
        return dist, summary, values
    return dist, summary
