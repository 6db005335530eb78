"""
Hydrogen bonds from LAMMPS dumps: which D-H...A bonds exist in every frame, how many each donor gives and each acceptor
takes, the distribution of the angle, and how long a bond lives (water, alcohols, protic electrolytes). The reference
has no such function; DESIGN.md (hydrogen bonds) holds the specification, and tests/hbonds_ref.py restates it in numpy.

What runs where
  GPU (libmdhip.so, csrc/hbonds.hip): per frame the donor - acceptor search, the geometric test of every hydrogen of a
      donor in reach, the counts and the angle histogram; for the lifetime the presence mask of every (hydrogen,
      acceptor) pair over the trajectory and the exact integer lag sums. The final integrals run in scan.hip.
  Host (numpy, this file): parsing (the native reader), the topology from the altered atom types, the cosine table
      of the bin edges, the normalisation and the DataFrames.

Atoms are named by the altered types of calc_atomic_rdf (the index of an atom inside its molecule type, through
calc_atom_type with num_mols and num_atoms_per_mol). donors=[(d_type, h_type), ...]: in every molecule that holds both,
the atom of h_type is bonded to the atom of d_type. acceptors=[a_type, ...]. The donor class is the index of the
distinct d_type, the acceptor class the index in `acceptors`.

Hydrogen h of donor d is bonded to acceptor a when a is not d (and not of d's molecule under exclusion), the distance
D...A is below r_da (the single-wrap rsq of the RDF functions, strict), the distance H...A is below r_ha (when given)
and the angle D-H...A is at least angle_cut, decided on the cosine without an arccos.
"""

import numpy as np
import pandas as pd

from .. import backend
from .. import io as mio
from ..common.com_mols import atom_molecules, calc_atom_type
from ..common.tables import density, write_csv
from ..common.trajectory import refuse_triclinic, typed_batches
from ..dist import is_writer

_SAME_ATOMS = "every frame must hold the same atoms in id order"


def _layout(num_mols, num_atoms_per_mol):
    """(n_atoms, mol_of int32 [n_atoms]) of the mandatory molecule layout."""
    if not num_mols or not num_atoms_per_mol:
        raise ValueError("hydrogen bonds need num_mols and num_atoms_per_mol (the molecule layout in id order)")
    if len(num_mols) != len(num_atoms_per_mol):
        raise ValueError("num_mols and num_atoms_per_mol must have the same length")
    return atom_molecules(num_mols, num_atoms_per_mol)


def _topology(types, mol_of, donors, acceptors):
    """
    The atom lists of a call from the altered types [N] and mol_of [N]: a dict of donors [n_don] (ascending atoms),
    don_class, h_off [n_don + 1], h_atoms [n_h], acceptors [n_acc] (ascending atoms), acc_class, d_types (the
    distinct d_type in the order given: the donor classes) and a_types.
    """
    pairs = [tuple(p) for p in donors] if donors is not None else []
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError("donors must be a non-empty list of (d_type, h_type) atom types")
    a_types = [int(a) for a in acceptors] if acceptors is not None else []
    if not a_types:
        raise ValueError("acceptors must be a non-empty list of atom types")
    if len(set(a_types)) != len(a_types):
        raise ValueError("acceptors holds a type twice")
    types = np.asarray(types).astype(np.int64)
    mol_of = np.asarray(mol_of)
    d_types = []
    for d, _ in pairs:
        if int(d) not in d_types:
            d_types.append(int(d))
    bonded = {}  # donor atom -> its hydrogens
    cls = {}
    for d, h in pairs:
        d, h = int(d), int(h)
        d_at, h_at = np.flatnonzero(types == d), np.flatnonzero(types == h)
        if len(d_at) == 0:
            raise ValueError("donor type %d names no atom" % d)
        if len(h_at) == 0:
            raise ValueError("hydrogen type %d names no atom" % h)
        # altered types name one atom per molecule: both lists ascend with the molecule
        if len(d_at) != len(h_at) or not np.array_equal(mol_of[d_at], mol_of[h_at]):
            raise ValueError("hydrogen type %d has no donor of type %d in its molecule" % (h, d))
        for da, ha in zip(d_at, h_at):
            bonded.setdefault(int(da), []).append(int(ha))
            cls[int(da)] = d_types.index(d)
    don = np.array(sorted(bonded), dtype=np.int32)
    h_off = np.concatenate([[0], np.cumsum([len(bonded[int(d)]) for d in don])]).astype(np.int32)
    h_atoms = np.array([h for d in don for h in bonded[int(d)]], dtype=np.int32)
    acc = np.flatnonzero(np.isin(types, a_types)).astype(np.int32)
    if len(acc) == 0:
        raise ValueError("the acceptor types name no atom")
    acc_class = np.array([a_types.index(int(t)) for t in types[acc]], dtype=np.int32)
    return {"donors": don, "don_class": np.array([cls[int(d)] for d in don], dtype=np.int32), "h_off": h_off,
            "h_atoms": h_atoms, "acceptors": acc, "acc_class": acc_class, "d_types": d_types, "a_types": a_types}


def _geometry(r_da, angle_cut, r_ha):
    """(r_da_sq, r_ha_sq (0: off), cos_cut) of the public arguments."""
    r_da, angle_cut = float(r_da), float(angle_cut)
    if not r_da > 0.0:
        raise ValueError("r_da must be positive")
    if not 0.0 <= angle_cut <= 180.0:
        raise ValueError("angle_cut must be in [0, 180] degrees")
    if r_ha is not None and not float(r_ha) > 0.0:
        raise ValueError("r_ha must be positive (or None)")
    return r_da * r_da, 0.0 if r_ha is None else float(r_ha) * float(r_ha), float(np.cos(np.radians(angle_cut)))


def _altered_types(ids, num_mols, num_atoms_per_mol):
    return calc_atom_type(ids, num_mols, num_atoms_per_mol).astype(np.int32)


def calc_hydrogen_bonds(donors, acceptors, filename, num_mols, num_atoms_per_mol, r_da=3.5, angle_cut=150.0,
                        r_ha=None, bin_size=1.0, exclude_same_molecule=True, path_or_buff="hbonds.csv", save_mode=True):
    """
    Hydrogen bonds of every frame of `filename` (dump file or '*' pattern). donors: [(d_type, h_type), ...],
    acceptors: [a_type, ...] (altered atom types, see the module text); r_da, r_ha in the dump's length unit (r_ha=None:
    no H...A test), angle_cut and bin_size in degrees.

    Returns (per_frame, summary, angles):
      per_frame: `Timestep` and per class pair `hb_d-a` (int64), the bonds of that frame; written to `path_or_buff`;
      summary: one row per class pair: pair, n_bonds, bonds_per_donor_frame, bonds_per_acceptor_frame, mean_angle
        (degrees, over the bin centres of the pair's distribution) and, on the first row, n_degenerate of the call;
      angles: `angle` (bin centres, degrees) and per class pair `adf_d-a` = count / (count.sum() * bin_size) and
        `count_d-a` (int64): the angle D-H...A of every (hydrogen, acceptor) within the distance cutoffs, bonded or
        not: the distribution to choose angle_cut from.
    """
    _, mol_of = _layout(num_mols, num_atoms_per_mol)
    r_da_sq, r_ha_sq, cos_cut = _geometry(r_da, angle_cut, r_ha)
    if donors is None or acceptors is None or len(donors) == 0 or len(acceptors) == 0:
        raise ValueError("donors and acceptors must be non-empty lists")
    edges = backend.angle_cos_edges(bin_size)
    n_bins = len(edges)
    refuse_triclinic(filename)

    top = None
    steps_all, per = [], []
    hist = n_don = n_acc = None
    degen = 0
    for steps, boxes, xyz, types in typed_batches(filename, num_mols, num_atoms_per_mol, True, mismatch=_SAME_ATOMS):
        if top is None:
            top = _topology(types, mol_of, donors, acceptors)
            n_dc, n_ac = len(top["d_types"]), len(top["a_types"])
            if n_dc * n_ac > backend.HBOND_MAX_CLASSES or n_dc * n_ac * n_bins > backend.HBOND_MAX_CELLS:
                raise ValueError("%d donor x %d acceptor classes x %d bins: at most %d class pairs and %d "
                                 "histogram cells per call" % (n_dc, n_ac, n_bins, backend.HBOND_MAX_CLASSES,
                                                               backend.HBOND_MAX_CELLS))
            hist = np.zeros((n_dc, n_ac, n_bins), dtype=np.uint64)
            n_don = np.zeros(len(top["donors"]), dtype=np.uint64)
            n_acc = np.zeros(len(top["acceptors"]), dtype=np.uint64)
        nb, nd, na, h, dg = backend.hbond_counts(
            xyz, boxes, top["donors"], top["don_class"], top["h_off"], top["h_atoms"], top["acceptors"],
            top["acc_class"], r_da_sq, cos_cut, r_ha_sq=r_ha_sq, cos_edges=edges,
            mol_of=mol_of if exclude_same_molecule else None, n_dc=n_dc, n_ac=n_ac)
        per.append(nb)
        n_don += nd
        n_acc += na
        hist += h
        degen += dg
        steps_all.extend(steps)
    if top is None:
        raise ValueError("no frames in %r" % (filename,))

    n_frames = len(steps_all)
    counts = np.concatenate(per).astype(np.int64)  # [F, n_dc, n_ac]
    centres = (np.arange(n_bins) + 0.5) * float(bin_size)
    per_frame = pd.DataFrame({"Timestep": np.asarray(steps_all, dtype=np.int64)})
    angles = pd.DataFrame({"angle": centres})
    rows = []
    for dc, d in enumerate(top["d_types"]):
        for ac, a in enumerate(top["a_types"]):
            name = "%d-%d" % (d, a)
            per_frame["hb_" + name] = counts[:, dc, ac]
            cnt = hist[dc, ac].astype(np.int64)
            total_angles = int(cnt.sum())
            angles["adf_" + name] = density(cnt, float(bin_size))
            angles["count_" + name] = cnt
            total = int(counts[:, dc, ac].sum())
            n_d, n_a = int((top["don_class"] == dc).sum()), int((top["acc_class"] == ac).sum())
            rows.append((name, total, total / (n_d * n_frames), total / (n_a * n_frames),
                         float((cnt * centres).sum() / total_angles) if total_angles else np.nan))
    summary = pd.DataFrame(rows, columns=["pair", "n_bonds", "bonds_per_donor_frame", "bonds_per_acceptor_frame",
                                          "mean_angle"])
    summary["n_degenerate"] = [int(degen)] + [0] * (len(rows) - 1)
    summary.attrs["n_donated"], summary.attrs["n_accepted"] = n_don, n_acc
    if save_mode and is_writer():
        write_csv(per_frame, path_or_buff)
    return per_frame, summary, angles


def _load_compact(filename, num_mols, num_atoms_per_mol, donors, acceptors, dt):
    """The trajectory of only the donor, hydrogen and acceptor atoms: (xyz [F,3,n], box [F,3], the topology with its
    atom lists remapped into the compact array, mol_of of the compact atoms, the frame spacing in ps)."""
    n_layout, mol_of = _layout(num_mols, num_atoms_per_mol)
    steps, boxes, planes = [], [], []
    types = top = keep = None
    for ts, bounds, lengths, _, pl in mio.iter_native_frames(filename, ["id", "type", "x", "y", "z"], sort_by="id"):
        b = np.asarray(bounds, dtype=np.float64)
        ext = b[:, 1] - b[:, 0]
        if np.any(np.abs(np.asarray(lengths, dtype=np.float64) - ext) > 1e-12 * np.abs(ext)):
            raise ValueError("triclinic boxes are not supported")
        if pl.shape[1] != n_layout:
            raise ValueError("a frame of %d atoms does not match the layout's %d" % (pl.shape[1], n_layout))
        lab = _altered_types(pl[0], num_mols, num_atoms_per_mol)
        if types is None:
            types = lab
            top = _topology(types, mol_of, donors, acceptors)
            keep = np.unique(np.concatenate([top["donors"], top["h_atoms"], top["acceptors"]]))
        elif not np.array_equal(lab, types):
            raise ValueError(_SAME_ATOMS)
        steps.append(int(ts))
        boxes.append(ext)
        planes.append(pl[2:5][:, keep])
    if not steps:
        raise ValueError("no frames in %r" % (filename,))
    delta = 0.0
    if len(steps) > 1:
        d_step = np.diff(np.asarray(steps, dtype=np.int64))
        if d_step[0] <= 0 or np.any(d_step != d_step[0]):
            raise ValueError("the frames must be uniformly spaced in time")
        delta = float(d_step[0]) * dt
    new = np.full(n_layout, -1, dtype=np.int32)
    new[keep] = np.arange(len(keep), dtype=np.int32)
    for k in ("donors", "h_atoms", "acceptors"):
        top[k] = new[top[k]]
    xyz = np.ascontiguousarray(np.stack(planes), dtype=np.float64)
    return xyz, np.ascontiguousarray(np.stack(boxes)), top, np.ascontiguousarray(mol_of[keep]), delta


def _lifetime_table(c_int, c_cont, n_frames, delta):
    """(DataFrame of `Time (ps)`, `C_int`, `C_cont`; tau_int; tau_cont) from the exact numerators:
    C[k] = (c[k] / (F - k)) / (c[0] / F); tau: the trapezoid integral of C over the lags (backend.cumtrapz)."""
    k = np.arange(len(c_int), dtype=np.float64)
    cols = {"Time (ps)": k * delta}
    taus = []
    for name, c in (("C_int", c_int), ("C_cont", c_cont)):
        c = np.asarray(c).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            cols[name] = (c / (n_frames - k)) / (c[0] / n_frames)
        if len(c) > 1 and c[0] > 0:
            taus.append(float(np.asarray(backend.cumtrapz(np.ascontiguousarray(cols[name]), delta)).ravel()[-1]))
        else:
            taus.append(0.0 if c[0] > 0 else np.nan)
    return pd.DataFrame(cols), taus[0], taus[1]


def calc_hbond_lifetime(donors, acceptors, filename, num_mols, num_atoms_per_mol, dt=1, max_lag=None, r_da=3.5,
                        angle_cut=150.0, r_ha=None, exclude_same_molecule=True, path_or_buff="hbond_lifetime.csv",
                        save_mode=True):
    """
    Hydrogen-bond time correlation functions over the trajectory `filename` (uniformly spaced frames, at most 65 535):
    with h(t) = 1 while a (hydrogen, acceptor) pair is bonded, the intermittent C_int(t) = <h(0) h(t)> / <h> and the
    continuous C_cont(t) = <h(0) ... h(t)> / <h> (no break in between), each averaged over all pairs and time
    origins. dt: timestep in fs; max_lag in frames (None: all); the geometry as calc_hydrogen_bonds.

    Returns (table, info): table with `Time (ps)`, `C_int`, `C_cont` (written to `path_or_buff`); info with tau_int and
    tau_cont (ps, the trapezoid integrals of the two columns), n_pairs (distinct pairs ever bonded), bonds_per_frame
    and n_frames.
    """
    r_da_sq, r_ha_sq, cos_cut = _geometry(r_da, angle_cut, r_ha)
    xyz, box, top, mol_c, delta = _load_compact(filename, num_mols, num_atoms_per_mol, donors, acceptors,
                                                float(dt) * 1e-3)
    n_frames = len(xyz)
    if n_frames > backend.HBOND_MAX_FRAMES:
        raise ValueError("%d frames: at most %d per call" % (n_frames, backend.HBOND_MAX_FRAMES))
    max_lag = n_frames - 1 if max_lag is None else int(max_lag)
    if not 0 <= max_lag <= n_frames - 1:
        raise ValueError("max_lag must be in [0, %d]" % (n_frames - 1))
    c_int, c_cont, n_pairs, n_rec = backend.hbond_lifetime(
        xyz, box, top["donors"], top["h_off"], top["h_atoms"], top["acceptors"], r_da_sq, cos_cut, r_ha_sq=r_ha_sq,
        mol_of=mol_c if exclude_same_molecule else None, max_lag=max_lag)
    table, tau_int, tau_cont = _lifetime_table(c_int, c_cont, n_frames, delta)
    info = {"tau_int": tau_int, "tau_cont": tau_cont, "n_pairs": n_pairs, "bonds_per_frame": n_rec / n_frames,
            "n_frames": n_frames}
    if save_mode and is_writer():
        write_csv(table, path_or_buff)
    return table, info
