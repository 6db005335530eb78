"""
Molecular aggregates from LAMMPS dumps: which molecules (or atoms) hang together through contacts between named atom
types — free ions, contact ion pairs and larger aggregates of an electrolyte, the size distribution of the aggregates
and the largest one of every frame. The per-centre shell functions (get_clusters, get_configurations) cannot see that
an anion bridging two cations sits in two shells; this one merges the shells into connected components. The reference
has no such function; DESIGN.md (aggregates) holds the specification, and tests/aggregates_ref.py restates it in numpy.

What runs where
  GPU (libmdhip.so, csrc/aggregates.hip): per frame the sweep of the A atoms against the B atoms, the contact test of
      every class pair, the lock-free union of the two nodes of every contact and the label (smallest member) of every
      node, the number of components and of contacts.
  Host (numpy, this file): parsing (the native reader), the atom types, the molecule layout and the participating
      nodes, the composition of every aggregate (one bincount over (frame, label, node type)), the census and the
      DataFrames.

One contact (type_a, type_b, r_cut): an atom of type_a and an atom of type_b of two different nodes are in contact at
rsq < r_cut**2 (the single-wrap rsq of the RDF functions, strict). Nodes in contact are neighbours; an aggregate is a
connected component of that graph, a node without a contact an aggregate of one.
"""

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import atom_molecules, molecule_layout
from ..common.tables import write_csv
from ..common.trajectory import refuse_triclinic, typed_batches
from ..dist import is_writer


def _contact_table(contacts):
    """-> (the checked contacts, types_a sorted, types_b sorted, rsq_cut [n_ca, n_cb]: 0 where no contact names the
    pair)."""
    con = [tuple(c) for c in contacts] if contacts is not None else []
    if not con or any(len(c) != 3 for c in con):
        raise ValueError("contacts must be a non-empty list of (type_a, type_b, r_cut)")
    con = [(int(a), int(b), float(r)) for a, b, r in con]
    seen = set()
    for a, b, r in con:
        if not r > 0.0:
            raise ValueError("contact (%d, %d): r_cut must be positive" % (a, b))
        if (a, b) in seen or (b, a) in seen:
            raise ValueError("contact (%d, %d) is given twice" % (a, b))
        seen.add((a, b))
    ta, tb = sorted({c[0] for c in con}), sorted({c[1] for c in con})
    if max(len(ta), len(tb)) > backend.CONTACT_MAX_CLASSES:
        raise ValueError("at most %d atom types per side of the contacts" % backend.CONTACT_MAX_CLASSES)
    cut = np.zeros((len(ta), len(tb)))
    for a, b, r in con:
        cut[ta.index(a), tb.index(b)] = r * r
    return con, ta, tb, cut


class _Nodes:
    """The participating nodes of a call and the two atom lists, from the atom types of the first frame; `mol_of` [n]:
    the molecule of every atom where molecules are the nodes, None where atoms are."""

    def __init__(self, con, ta, tb, types, mol_of, num_mols, num_atoms_per_mol, mol_types):
        n = len(types)
        named = sorted(set(ta) | set(tb))
        keep = None if mol_types is None else {int(k) for k in mol_types}
        if mol_of is not None:
            mol_type = molecule_layout(num_mols, num_atoms_per_mol)[1]
            # (molecule type k holds the altered atom types upper[k - 2] + 1 .. upper[k - 1])
            upper = np.cumsum(np.asarray(num_atoms_per_mol, dtype=np.int64))
            holder = {t: int(np.searchsorted(upper, t, side="left")) + 1 for t in named if 1 <= t <= upper[-1]}
            part = {k for k in holder.values() if keep is None or k in keep}
            kind = "molecule"
            in_node = np.isin(mol_type, sorted(part))  # [M]
            node_type = mol_type[in_node]
            node_of_mol = np.cumsum(in_node) - 1
            listed = in_node[mol_of]  # [n]
            node_of = np.where(listed, node_of_mol[mol_of], 0)
            held = {t for t, k in holder.items() if k in part}
        else:
            part = {t for t in named if keep is None or t in keep}
            kind = "atom"
            listed = np.isin(types, sorted(part))
            node_type = types[listed].astype(np.int64)
            node_of = np.where(listed, np.cumsum(listed) - 1, 0)
            held = set(np.unique(node_type).tolist())
        for a, b, _ in con:
            for t in (a, b):
                if t not in held:
                    raise ValueError("contact (%d, %d): no participating %s holds atom type %d" % (a, b, kind, t))
        self.n_atoms = n
        self.n_nodes = int(len(node_type))
        self.node_type = np.asarray(node_type, dtype=np.int64)
        self.type_ids = sorted(part if mol_of is not None else held)
        self.node_of = node_of.astype(np.int32)
        self.atoms_a = np.flatnonzero(listed & np.isin(types, ta)).astype(np.int32)
        self.atoms_b = np.flatnonzero(listed & np.isin(types, tb)).astype(np.int32)
        self.class_a = np.searchsorted(ta, types[self.atoms_a]).astype(np.int32)
        self.class_b = np.searchsorted(tb, types[self.atoms_b]).astype(np.int32)


def _compositions(labels, node_type, type_ids):
    """labels [F, n] -> (comp int64 [n_agg, T]: the nodes of every type in every aggregate of every frame, frames in
    order and aggregates by label; frame int64 [n_agg]: the frame of each)."""
    F, n = labels.shape
    T = len(type_ids)
    tix = np.searchsorted(type_ids, node_type)
    key = (np.arange(F, dtype=np.int64)[:, None] * n + labels) * T + tix[None, :]
    comp = np.bincount(key.ravel(), minlength=F * n * T).reshape(F * n, T)
    roots = np.flatnonzero((labels == np.arange(n)[None, :]).ravel())
    return comp[roots], roots // max(n, 1)


def census_of_labels(labels, node_type, type_ids, names, steps=None, n_contacts=None):
    """(census, sizes, per_frame) of calc_aggregates from finished labels [F, n] (label = smallest member), the type of
    every node [n], the participating types (sorted) and their column names."""
    labels = np.asarray(labels, dtype=np.int64)
    F, n = labels.shape
    acc = _Census(len(type_ids))
    acc.add(labels, np.asarray(node_type), list(type_ids), np.arange(F) if steps is None else steps,
            np.zeros(F, dtype=np.int64) if n_contacts is None else n_contacts)
    return acc.tables(list(names), n)


class _Census:
    """The running census over the batches of a call."""

    def __init__(self, n_types):
        self.comps = np.zeros((0, n_types), dtype=np.int64)
        self.counts = np.zeros(0, dtype=np.int64)
        self.sizes = np.zeros(1, dtype=np.int64)
        self.rows = []
        self.n_frames = 0

    def add(self, labels, node_type, type_ids, steps, n_contacts):
        F = len(labels)
        comp, frame = _compositions(np.asarray(labels, dtype=np.int64), node_type, type_ids)
        uniq, inv = np.unique(np.concatenate([self.comps, comp]), axis=0, return_inverse=True)
        self.counts = np.bincount(np.asarray(inv).ravel(), weights=np.concatenate([self.counts, np.ones(len(comp))]),
                                  minlength=len(uniq)).astype(np.int64)
        self.comps = uniq
        size = comp.sum(axis=1)
        sc = np.bincount(size, minlength=len(self.sizes))
        sc[:len(self.sizes)] += self.sizes
        self.sizes = sc
        n_agg = np.bincount(frame, minlength=F)
        # (the aggregates come frame by frame, and a frame with nodes has at least one)
        largest = np.maximum.reduceat(size, np.cumsum(n_agg) - n_agg) if len(size) else np.zeros(F, dtype=np.int64)
        for f in range(F):
            self.rows.append((int(steps[f]), int(n_agg[f]), int(largest[f]), int(n_contacts[f])))
        self.n_frames += F

    def tables(self, names, n_nodes):
        """(census, sizes, per_frame): the distinct compositions by count descending, then composition ascending."""
        comps, counts, F = self.comps, self.counts, self.n_frames
        total = int(counts.sum())
        order = np.lexsort([comps[:, k] for k in range(comps.shape[1] - 1, -1, -1)] + [-counts])
        comps, counts = comps[order], counts[order]
        census = pd.DataFrame({name: comps[:, k] for k, name in enumerate(names)})
        census["n_aggregates"] = counts
        census["per_frame"] = counts / F if F else np.zeros(len(counts))
        census["fraction"] = counts / total if total else np.zeros(len(counts))
        size = np.flatnonzero(self.sizes)
        sizes = pd.DataFrame({"size": size, "n_aggregates": self.sizes[size],
                              "fraction_of_nodes": size * self.sizes[size] / (n_nodes * F) if n_nodes * F
                              else np.zeros(len(size))})
        per = pd.DataFrame(self.rows, columns=["step", "n_aggregates", "largest", "n_contacts"]).astype(np.int64)
        return census, sizes, per


def calc_aggregates(contacts, filename, num_mols=None, num_atoms_per_mol=None, mol_names=None, mol_types=None,
                    return_labels=False, path_or_buff="aggregates.csv", save_mode=True):
    """
    The aggregates of the frames of `filename` (dump file or '*' pattern) under `contacts` [(type_a, type_b, r_cut), ...].
    With num_mols and num_atoms_per_mol the types are the altered atom types of calc_atomic_rdf (the index of an atom
    inside its molecule type), the nodes are molecules and a node's type is its molecule type; the molecules of every
    molecule type that holds a named atom type take part. Without them the types are the dump's `type` column and the
    nodes are the atoms of the named types. mol_types (1-based) narrows the participating node types further. Node
    indices follow id order among the participants. (a, b, r) links the pairs that (b, a, r) links; naming a pair twice
    is an error.

    Returns (census, sizes, per_frame) and, with return_labels, labels int32 [F, n_nodes] (the smallest node of every
    node's aggregate):
      census: one row per distinct composition: one int column per participating node type (named by mol_names, else
        mol_<k>, or type_<k> without a layout), n_aggregates (over all frames), per_frame (n_aggregates / F) and
        fraction (of all aggregates); ordered by n_aggregates descending, then by the composition columns ascending;
        written to `path_or_buff`;
      sizes: size, n_aggregates, fraction_of_nodes = size * n_aggregates / (n_nodes * F);
      per_frame: step, n_aggregates, largest, n_contacts.
    """
    con, ta, tb, cut = _contact_table(contacts)
    layout = num_mols is not None and num_atoms_per_mol is not None
    mol_of = atom_molecules(num_mols, num_atoms_per_mol)[1] if layout else None  # (a bad layout raises here)
    refuse_triclinic(filename)

    nodes = acc = None
    all_labels = []
    for steps, boxes, xyz, types in typed_batches(filename, num_mols, num_atoms_per_mol, layout):
        if nodes is None:
            nodes = _Nodes(con, ta, tb, types, mol_of, num_mols, num_atoms_per_mol, mol_types)
            acc = _Census(len(nodes.type_ids))
        label, _, n_con = backend.contact_components(xyz, boxes, nodes.atoms_a, nodes.class_a, nodes.atoms_b,
                                                     nodes.class_b, cut, nodes.node_of, nodes.n_nodes)
        acc.add(label, nodes.node_type, nodes.type_ids, steps, n_con)
        if return_labels:
            all_labels.append(np.array(label, dtype=np.int32))
    if nodes is None:
        raise ValueError("no frames in %r" % (filename,))

    if mol_names is not None:
        names = [str(mol_names[k - 1]) for k in nodes.type_ids]
    else:
        names = [("mol_%d" if layout else "type_%d") % k for k in nodes.type_ids]
    census, sizes, per_frame = acc.tables(names, nodes.n_nodes)
    if save_mode and is_writer():
        write_csv(census, path_or_buff)
    if return_labels:
        return census, sizes, per_frame, np.concatenate(all_labels)
    return census, sizes, per_frame
