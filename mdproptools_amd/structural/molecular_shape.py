"""
The shape of flexible molecules from LAMMPS dumps — glymes, PEO oligomers, ionic-liquid cations with alkyl tails, polymer
electrolytes: the radius of gyration and its distribution, the end-to-end distance, the principal moments of the
mass-weighted gyration tensor, asphericity, acylindricity and the relative shape anisotropy kappa^2. The reference has
no such module; include/mdhip.h (mdhip_mol_shape) holds the specification of the device part and tests/shape_ref.py
restates it in numpy. Arguments follow `calc_molecular_rdf` and `calc_dihedral_distribution`.

What runs where
  GPU (libmdhip.so, csrc/mol_shape.hip): per frame and molecule the positions about the first atom (the chain followed
      bond by bond through the periodic box), the centre of mass, the gyration tensor, Rg^2, Ree^2, I2, kappa^2 and the
      principal moments by cyclic Jacobi; exact integer histograms of Rg, Ree and kappa^2 and per-frame totals in a fixed
      order of summation.
  Host: parsing (common/trajectory.py: the frames are never all resident), the molecule layout, the masses, adding the
      batches' integer histograms, putting the frames in time order, the means and the CSV files.

With unwrap="chain" (the default) every difference between CONSECUTIVE atoms of a molecule is wrapped once, which is
right whenever consecutive atoms lie within half a box edge of each other — bonded neighbours do —, however long the
molecule is. unwrap="first" wraps every atom against the molecule's first atom, the rule of `Reorientation`: right only
for molecules shorter than half a box edge. With coords="unwrapped" nothing is wrapped and the two agree.
"""

import math
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import mol_series
from ..common import trajectory as T
from ..common.tables import density
from ..dist import is_writer

MAX_BINS = backend.SHAPE_MAX_BINS
MAX_KAPPA_BINS = backend.SHAPE_MAX_KBINS
UNWRAP = {"chain": 1, "first": 0}
TABLES = ("summary", "rg", "ree", "kappa2", "frames")
SUMMARY = ["molecule", "n_mols", "<Rg>", "<Rg2>^1/2", "<Ree2>^1/2", "<Ree2>/<Rg2>", "<l1>", "<l2>", "<l3>", "asphericity",
           "acylindricity", "<k2>", "k2 (ratio of averages)", "beyond Rg", "beyond Ree", "degenerate"]


def _selection(num_mols, num_atoms_per_mol, mol_types, mol_names, ends):
    """(num_mols, per, types 0-based, names, ends 0-based [(e0, e1)]) of the arguments, or a ValueError."""
    num_mols, per = mol_series.layout(num_mols, num_atoms_per_mol)
    types = list(range(1, len(per) + 1)) if mol_types is None else [int(t) for t in mol_types]
    if not types:
        raise ValueError("mol_types must name at least one molecule type")
    for t in types:
        if not 1 <= t <= len(per):
            raise ValueError("mol_types: %d is not in [1, %d]" % (t, len(per)))
        if per[t - 1] < 1:
            raise ValueError("molecule type %d has no atoms" % t)
    if len(set(types)) != len(types):
        raise ValueError("mol_types names a molecule type twice")
    names = ["mol%d" % t for t in types] if mol_names is None else [str(n) for n in mol_names]
    if len(names) != len(types) or len(set(names)) != len(names):
        raise ValueError("mol_names must hold one name, all different, per entry of mol_types")
    if ends is None:
        ends = [None] * len(types)
    ends = list(ends)
    if len(ends) != len(types):
        raise ValueError("ends must hold one (first, last) or None per entry of mol_types")
    out = []
    for t, e in zip(types, ends):
        n = per[t - 1]
        if e is None:
            out.append((0, n - 1))
            continue
        try:
            e0, e1 = (int(v) for v in e)
        except (TypeError, ValueError):
            raise ValueError("ends: %r is not a pair (first, last) of atoms" % (e,)) from None
        if not (1 <= e0 <= n and 1 <= e1 <= n):
            raise ValueError("ends: the atoms of %r must be in [1, %d], the atoms of a molecule of type %d" % (e, n, t))
        out.append((e0 - 1, e1 - 1))
    return num_mols, per, [t - 1 for t in types], names, out


def default_r_max(lengths):
    """One Angstrom per bond of the longest selected molecule, and at least 2: half the length of a chain of 2 A bonds
    stretched out, which no radius of gyration and few end-to-end distances of a flexible chain reach. What does fall
    beyond is counted and reported (`beyond Rg`, `beyond Ree`), never dropped."""
    return max(2.0, float(max(lengths) - 1))


def _n_bins(r_max, bin_size):
    bin_size, r_max = float(bin_size), float(r_max)
    if not (bin_size > 0 and math.isfinite(bin_size) and r_max > 0 and math.isfinite(r_max)):
        raise ValueError("bin_size and r_max must be positive and finite")
    n = int(math.ceil(r_max / bin_size - 1e-9))
    if not 1 <= n <= MAX_BINS:
        raise ValueError("r_max / bin_size = %d bins; at most %d: take a larger bin_size" % (n, MAX_BINS))
    return n


def summary_row(totals, n_mols):
    """The means of one molecule type from its totals [9,F] (rows backend.SHAPE_TOTALS): every mean the sum over the
    frames divided once by molecules * frames; all NaN for a type without molecules."""
    n = float(n_mols * totals.shape[1])
    keys = SUMMARY[2:13]
    if not n:
        return dict.fromkeys(keys, np.nan)
    mean = {name: float(np.sum(totals[k])) / n for k, name in enumerate(backend.SHAPE_TOTALS)}
    return {"<Rg>": mean["Rg"], "<Rg2>^1/2": np.sqrt(mean["Rg2"]), "<Ree2>^1/2": np.sqrt(mean["Ree2"]),
            "<Ree2>/<Rg2>": mean["Ree2"] / mean["Rg2"] if mean["Rg2"] else np.nan,
            "<l1>": mean["l1"], "<l2>": mean["l2"], "<l3>": mean["l3"],
            "asphericity": mean["l1"] - (mean["l2"] + mean["l3"]) / 2, "acylindricity": mean["l2"] - mean["l3"],
            "<k2>": mean["k2"], "k2 (ratio of averages)": 1.0 - 3.0 * mean["I2"] / mean["Rg4"] if mean["Rg4"] else np.nan}


def tables(names, n_mols, steps, hist_rg, hist_ee, hist_k, beyond, degenerate, totals, bin_size):
    """The five DataFrames of calc_molecular_shape from the added counts (hist_rg, hist_ee [J,nbins], hist_k [J,nk],
    beyond [J,2], degenerate [J]) and the totals [J,9,F] with their timesteps [F], both in time order."""
    n_bins, n_kbins = hist_rg.shape[1], hist_k.shape[1]
    rows = []
    for j, name in enumerate(names):
        row = {"molecule": name, "n_mols": int(n_mols[j])}
        row.update(summary_row(totals[j], n_mols[j]))
        row.update({"beyond Rg": int(beyond[j, 0]), "beyond Ree": int(beyond[j, 1]), "degenerate": int(degenerate[j])})
        rows.append(row)
    r = (np.arange(n_bins) + 0.5) * float(bin_size)
    rg, ree = {"r (A)": r}, {"r (A)": r.copy()}
    kappa = {"kappa2": (np.arange(n_kbins) + 0.5) / n_kbins}
    frames = {"timestep": np.asarray(steps, dtype=np.int64)}
    index = {name: k for k, name in enumerate(backend.SHAPE_TOTALS)}
    for j, name in enumerate(names):
        rg["p_" + name] = density(hist_rg[j], float(bin_size))
        ree["p_" + name] = density(hist_ee[j], float(bin_size))
        kappa["p_" + name] = density(hist_k[j], 1.0 / n_kbins)
        with np.errstate(invalid="ignore", divide="ignore"):
            frames["Rg_" + name] = totals[j, index["Rg"]] / float(n_mols[j]) if n_mols[j] else np.full(len(steps), np.nan)
            frames["Ree2_" + name] = totals[j, index["Ree2"]] / float(n_mols[j]) if n_mols[j] else np.full(len(steps), np.nan)
    return {"summary": pd.DataFrame(rows, columns=SUMMARY), "rg": pd.DataFrame(rg), "ree": pd.DataFrame(ree),
            "kappa2": pd.DataFrame(kappa), "frames": pd.DataFrame(frames)}


def weight_rows(types_row, mass, a0, mols, length, names):
    """The masses of one molecule of every selected type from a frame's atom-type column [N] and the per-type `mass`
    list; the molecules of a type must all carry the same atom types."""
    if mass is None or not len(mass):
        raise ValueError("mass must hold the mass of every atom type")
    rows = []
    for start, m, n, name in zip(a0, mols, length, names):
        row = mol_series.same_rows(types_row, int(start), int(m), int(n), "atom types", name)
        if m and not (np.all(row >= 1) and np.all(row <= len(mass))):
            raise ValueError("molecule %s: an atom type is outside the %d entries of mass" % (name, len(mass)))
        w = T.masses(row, mass) if m else np.ones(int(n))
        if not (np.sum(w) > 0 and np.all(np.isfinite(w))):
            raise ValueError("molecule %s: its masses must be finite and add up to a positive mass" % name)
        rows.append(np.asarray(w, dtype=np.float64))
    return rows


def calc_molecular_shape(filename, num_mols, num_atoms_per_mol, mass, mol_types=None, mol_names=None, bin_size=0.05,
                         r_max=None, ends=None, kappa_bins=50, coords="wrapped", unwrap="chain", per_molecule=False,
                         save=False, working_dir=None, **how):
    """
    Gyration tensors and chain size of the molecules of `filename` (dump file or '*' pattern), per molecule type.
    num_mols / num_atoms_per_mol: molecules per type and atoms per molecule in id order; mass: the mass of every atom
    type (the atom types of a molecule type are read from the first frame and must be the same in all its molecules).
    mol_types: the 1-based molecule types to analyse (default: all), mol_names their names in the tables (default
    mol<type>). ends: per selected type (first, last), 1-based atoms inside the molecule between which the end-to-end
    distance is taken, or None for (1, last atom). bin_size (A) and r_max (A) set the bins of Rg and Ree; r_max defaults
    to `default_r_max`: 1 A per bond of the longest selected molecule, at least 2 A. kappa_bins: bins of kappa^2 over
    [0, 1]. coords="wrapped" reads `x y z` and the box, coords="unwrapped" `xu yu zu` (or x y z ix iy iz).
    unwrap="chain" follows every molecule bond by bond through the box, unwrap="first" wraps every atom against the
    molecule's first one. `how`: stream, batch_bytes of trajectory.attribute_batches. Triclinic boxes are not supported.

    Returns a dict of DataFrames:
      "summary": one row per molecule type: `molecule`, `n_mols`, `<Rg>`, `<Rg2>^1/2`, `<Ree2>^1/2`, `<Ree2>/<Rg2>`, the
        mean principal moments `<l1>` >= `<l2>` >= `<l3>` of the gyration tensor, `asphericity` = <l1> - (<l2> + <l3>)/2,
        `acylindricity` = <l2> - <l3>, `<k2>` (the mean of the per-molecule kappa^2 = 1 - 3 I2 / Rg^4), `k2 (ratio of
        averages)` = 1 - 3 <I2> / <Rg^4>, `beyond Rg` / `beyond Ree` (the molecule-frame pairs at or beyond r_max, or not
        finite: in no bin) and `degenerate` (Rg = 0: one atom, or all atoms on one point; no kappa^2);
      "rg", "ree": `r (A)` (bin centres) and per type `p_<name>` = counts / (total * bin_size); "kappa2": `kappa2` and
        `p_<name>` = counts * kappa_bins / total; a column is all NaN when there are no counts;
      "frames": `timestep` and per type `Rg_<name>`, `Ree2_<name>`: the means over the type's molecules per frame, in
        time order;
      and with per_molecule "per_molecule": per type an array [F,6,M] of Rg^2, Ree^2, kappa^2, l1, l2, l3 per frame (time
        order) and molecule.
    With `save` every DataFrame is written to shape_<table>.csv in working_dir (default: the current directory).
    """
    if coords not in ("wrapped", "unwrapped"):
        raise ValueError('coords must be "wrapped" or "unwrapped"')
    if unwrap not in UNWRAP:
        raise ValueError('unwrap must be "chain" or "first" (%r given)' % (unwrap,))
    num_mols, per, types, names, ends = _selection(num_mols, num_atoms_per_mol, mol_types, mol_names, ends)
    a0, mols, length = mol_series.type_jobs(types, num_mols, per)
    n_bins = _n_bins(default_r_max(length) if r_max is None else r_max, bin_size)
    n_kbins = int(kappa_bins)
    if not 1 <= n_kbins <= MAX_KAPPA_BINS:
        raise ValueError("kappa_bins must be in [1, %d]" % MAX_KAPPA_BINS)
    T.refuse_triclinic(filename)
    wrapped = coords == "wrapped"
    J = len(types)
    _, batches = T.attribute_batches(filename, ("id", "type"), ["x", "y", "z"] if wrapped else T.UNWRAPPED,
                                     n_atoms=int(np.dot(num_mols, per)), with_box=True, **how)
    hist_rg, hist_ee = (np.zeros((J, n_bins), dtype=np.uint64) for _ in range(2))
    hist_k = np.zeros((J, n_kbins), dtype=np.uint64)
    beyond, degenerate = np.zeros((J, 2), dtype=np.uint64), np.zeros(J, dtype=np.uint64)
    weights, steps, totals, values = None, [], [], []
    for ts, _ids, atom_types, xyz, box in batches:
        if weights is None:
            weights = weight_rows(np.asarray(atom_types[0]), mass, a0, mols, length, names)
        got = backend.mol_shape(xyz, box if wrapped else None, a0, mols, length, weights, ends=ends, unwrap=UNWRAP[unwrap],
                                bin_size=bin_size, n_bins=n_bins, n_kbins=n_kbins, per_mol=per_molecule)
        np.add(hist_rg, got["hist_rg"], out=hist_rg)
        np.add(hist_ee, got["hist_ee"], out=hist_ee)
        np.add(hist_k, got["hist_k"], out=hist_k)
        np.add(beyond, got["beyond"], out=beyond)
        np.add(degenerate, got["degenerate"], out=degenerate)
        totals.append(got["totals"])
        if per_molecule:
            values.append(np.array(got["per_mol"]))
        steps.extend(np.asarray(ts).tolist())
    if not steps:
        raise ValueError(f"no frames match {filename}")
    order = np.argsort(np.asarray(steps, dtype=np.int64), kind="stable")
    out = tables(names, mols, np.asarray(steps, dtype=np.int64)[order], hist_rg, hist_ee, hist_k, beyond, degenerate,
                 np.concatenate(totals, axis=2)[:, :, order], bin_size)
    if save and is_writer():
        where = working_dir or os.getcwd()
        for name in TABLES:
            out[name].to_csv(os.path.join(where, "shape_%s.csv" % name))
    if per_molecule:
        allv = np.concatenate(values, axis=0)[order]
        first = np.concatenate(([0], np.cumsum(mols)))
        out["per_molecule"] = [allv[:, :, first[j]:first[j + 1]] for j in range(J)]
    return out
