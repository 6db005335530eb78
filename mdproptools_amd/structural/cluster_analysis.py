"""
Solvation-shell clusters from LAMMPS dumps — drop-in for get_clusters of
/root/reference/mdproptools/structural/cluster_analysis.py:47-235 (same signature, defaults, files and return value),
plus get_cluster_compositions, which counts the same clusters without writing them; get_unique_configurations, the
drop-in for the census of those files (cluster_analysis.py:238-457; host only, no pymatgen), and get_configurations,
which takes the same census straight from the trajectory.

What runs where
  GPU (libmdhip.so, csrc/clusters.hip): the shell search — every centre of a batch of frames against every atom with
      the reference's single-wrap rsq (cluster_analysis.py:127-142) — and the per-molecule force sums of the filter
      (pandas' compensated groupby().sum(), cluster_analysis.py:146-152); for get_configurations
      (csrc/configurations.hip) the same search with, per shell molecule, its coordinating atoms counted by class,
      every row in one canonical order.
  Host (numpy, this file): parsing (the native reader; only the requested frame when full_trajectory is False), the
      molecule layout, the force threshold, the row order, the boundary shift and the text.

The reference's per-centre pandas merges come down to these rules, reproduced exactly:
  * rows: the centre, the other atoms of its molecule in id order, then the atoms of the other passing shell
    molecules, by (molecule type, molecule id) and then id;
  * a molecule passes when min(Sx, Sy, Sz) * 0.043363 / 16 < max_force (signed minimum); when the centre's own
    molecule fails, its atoms and the centre row itself are absent (the final inner merge, cluster_analysis.py:213-216);
  * coordinates are shifted once relative to the centre, x - sign(x - c) L when x - c > L/2 or < -L/2;
  * Cluster_{frame}_{centre}.xyz, both counters zero-padded to the width of their totals.
"""

import glob
import os
import shutil
import warnings
import zipfile
from collections import Counter

import numpy as np
import pandas as pd

from .. import backend
from .. import io as mio
from ..common.com_mols import atom_molecules, calc_atom_type, check_atom_count, molecule_layout
from ..common.trajectory import frame_refs, read_frame

FORCE_CONSTANT = 0.043363 / 16.0  # cluster_analysis.py:29
_COLS = ["id", "type", "x", "y", "z", "fx", "fy", "fz"]
MAX_BATCH_BYTES = 1 << 28  # coordinates + forces of the frames handed to the GPU in one call
_ROW_FMT = "%s\t%15.10f\t%15.10f\t%15.10f\n"  # to_csv(sep="\t", float_format="%15.10f"), cluster_analysis.py:226-229


def _padded(i, n):
    """str(i) with leading zeros to the width of str(n) (cluster_analysis.py:218-225)."""
    return "0" * (len(str(n)) - len(str(i))) + str(i)


def cluster_file_name(frame_index, n_frames, centre_index, n_centres):
    return "Cluster_{}_{}.xyz".format(_padded(frame_index, n_frames), _padded(centre_index, n_centres))


def _layout(num_mols, num_atoms_per_mol):
    seg_off, mol_type, _ = molecule_layout(num_mols, num_atoms_per_mol)
    return atom_molecules(num_mols, num_atoms_per_mol)[1], seg_off, mol_type


def _element_column(fname, k):
    """The dump's own `element` column of frame k, in id order (text: the pandas route)."""
    for j, lines in enumerate(mio._iter_frames(fname)):
        if j == k:
            df = mio.LammpsDump.from_lines(lines).data.sort_values(by=["id"])
            return df["element"].to_numpy()
    raise IndexError(k)


def _frames(filename, full_trajectory, frame, refs=None):
    """-> (number of frames processed, iterator of (file, frame in file, timestep, bounds, names, planes)); `refs`:
    frame_refs(filename) when the caller has it already."""
    refs = frame_refs(filename) if refs is None else refs
    if not full_trajectory:
        refs = [refs[frame]]  # dumps[frame] (cluster_analysis.py:104-107): Python indexing, its errors included

        def one():
            fname, k = refs[0]
            yield (fname, k) + read_frame(fname, k, _COLS)

        return 1, one()

    def every():
        it = mio.iter_native_frames(filename, _COLS, sort_by="id")
        for (fname, k), (ts, bounds, _, names, planes) in zip(refs, it):
            yield fname, k, ts, bounds, names, planes

    return len(refs), every()


def _row_index(starts, lens):
    """The concatenated ranges [starts[i], starts[i] + lens[i])."""
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    return np.repeat(starts - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(total)


def _cluster_text(xyz, lengths, p, own_ok, others, el, mol_of, seg_off):
    """The text of the cluster file of centre position p: its own molecule (when it passes), then `others`."""
    sizes = np.diff(seg_off)
    rows = _row_index(seg_off[others], sizes[others])
    if own_ok:
        own = np.arange(seg_off[mol_of[p]], seg_off[mol_of[p] + 1])
        rows = np.concatenate(([p], own[own != p], rows))
    pos = xyz[:, rows]
    d = pos - xyz[:, p][:, None]
    half = lengths / 2
    cond = (d > half[:, None]) | (d < -half[:, None])  # _remove_boundary_effects, cluster_analysis.py:32-44
    pos = np.where(cond, pos - np.sign(d) * lengths[:, None], pos)
    vals = np.empty((len(rows), 4), dtype=object)
    vals[:, 0] = el[rows]
    vals[:, 1:] = pos.T
    return "{}\n\n".format(len(rows)) + (_ROW_FMT * len(rows)) % tuple(vals.ravel())


class _Source:
    """
    The frames a call processes, prepared and batched for the GPU: frame selection, the element rule and its error,
    the centres. A prepared frame is (timestep, lengths [3], planes [8, N] of _COLS, element per atom or None, centre
    positions int32).
    """

    def __init__(self, filename, atom_type, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
                 alter_atom_types, max_force, need_elements):
        self.filename, self.atom_type, self.num_mols, self.num_atoms = filename, atom_type, num_mols, num_atoms_per_mol
        self.full_trajectory, self.frame, self.elements = full_trajectory, frame, elements
        self.alter_atom_types, self.max_force, self.need_elements = alter_atom_types, max_force, need_elements
        self.mol_of, self.seg_off, self.mol_type = _layout(num_mols, num_atoms_per_mol)
        self.n_atoms = int(self.seg_off[-1])
        self.el_map = np.asarray(elements, dtype=object) if elements else None

    def prepare(self, item):
        fname, k, ts, bounds, names, planes = item
        check_atom_count(self.n_atoms, planes.shape[1])
        if self.need_elements and "element" not in names and not self.elements:  # cluster_analysis.py:122-126
            raise ValueError(
                "The elements of the atoms in the system should be provided if they "
                "are not in the dump files."
            )
        el = None
        if self.need_elements:
            el = self.el_map[planes[1].astype(np.int64) - 1] if self.elements else _element_column(fname, k)
        types = calc_atom_type(planes[0], self.num_mols, self.num_atoms) if self.alter_atom_types else planes[1]
        lengths = np.asarray(bounds, dtype=np.float64)
        lengths = lengths[:, 1] - lengths[:, 0]
        return ts, lengths, planes, el, np.flatnonzero(types == self.atom_type).astype(np.int32)

    def reread(self, index):
        """The prepared frame of processed-frame index `index` (after batches()), read again on its own."""
        fname, k = self.refs[index if self.full_trajectory else self.frame]
        return self.prepare((fname, k) + read_frame(fname, k, _COLS))

    def batches(self, same=None):
        """
        -> (number of frames processed, iterator of (index of the batch's first frame, batch)), a batch a list of
        prepared frames with the same centres (and, when given, the same same(frame)) of at most MAX_BATCH_BYTES.
        """
        self.refs = frame_refs(self.filename)
        n_frames, frames = _frames(self.filename, self.full_trajectory, self.frame, self.refs)

        def it():
            batch, first, index = [], 0, 0
            per_frame = 6 * self.n_atoms * 8
            for item in frames:
                fr = self.prepare(item)
                if batch and (len(batch) * per_frame >= MAX_BATCH_BYTES or not np.array_equal(fr[4], batch[0][4])
                              or (same is not None and not np.array_equal(same(fr), same(batch[0])))):
                    yield first, batch
                    batch, first = [], index
                batch.append(fr)
                index += 1
            if batch:
                yield first, batch

        return n_frames, it()

    def staged(self, batch):
        """(xyz [B, 3, N], box [B, 3], pass mask [B, M] of the force filter) of a batch."""
        xyz = np.ascontiguousarray(np.stack([b[2][2:5] for b in batch]))
        force = np.ascontiguousarray(np.stack([b[2][5:8] for b in batch]))
        box = np.stack([b[1] for b in batch])
        passes = backend.mol_kahan_sums(force, self.seg_off).min(axis=1) * FORCE_CONSTANT < self.max_force  # [B, M]
        return xyz, box, passes


def _cluster_members(shell, passes, own):
    """(own molecule passes, the passing shell molecules other than it) of one centre: shell ascending, passes [M]."""
    passing = shell[passes[shell]]
    return bool((passing == own).any()), passing[passing != own]


def _iter_clusters(filename, atom_type, r_cut, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
                   alter_atom_types, max_force, need_elements):
    """
    Yields per processed frame: (frame index, number of frames, timestep, lengths [3], planes [8, N] of _COLS,
    element per atom or None, clusters), clusters a list over the frame's centres (id order) of (centre position,
    own molecule passes, passing shell molecules other than the centre's own, ascending).
    """
    src = _Source(filename, atom_type, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
                  alter_atom_types, max_force, need_elements)
    mol_of = src.mol_of
    rc2 = r_cut ** 2  # cluster_analysis.py:140
    n_frames, batches = src.batches()
    for first, batch in batches:
        centres = batch[0][4]
        xyz, box, passes = src.staged(batch)
        mols, count = backend.shell_members(xyz, box, centres, mol_of, rc2)
        for j, (ts, lengths, planes, el, _) in enumerate(batch):
            clusters = []
            for c, p in enumerate(centres):
                clusters.append((int(p),) + _cluster_members(mols[j, c, :count[j, c]], passes[j], mol_of[p]))
            yield first + j, n_frames, ts, lengths, planes, el, clusters


def get_clusters(
    filename,
    atom_type,
    r_cut,
    num_mols,
    num_atoms_per_mol,
    full_trajectory=False,
    frame=None,
    elements=None,
    alter_atom_types=False,
    max_force=0.75,
    working_dir=None,
):
    """
    Extracts the clusters within r_cut of every atom of type `atom_type` (the altered type when alter_atom_types) and
    writes each to Cluster_{frame}_{centre}.xyz in `working_dir` (default: the current directory). Arguments as in
    the reference (cluster_analysis.py:60-98). Returns the number of files written.
    """
    working_dir = working_dir or os.getcwd()
    mol_of, seg_off, _ = _layout(num_mols, num_atoms_per_mol)
    written = 0
    for index, n_frames, ts, lengths, planes, el, clusters in _iter_clusters(
            filename, atom_type, r_cut, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
            alter_atom_types, max_force, True):
        for c, (p, own_ok, others) in enumerate(clusters):
            text = _cluster_text(planes[2:5], lengths, p, own_ok, others, el, mol_of, seg_off)
            name = cluster_file_name(index, n_frames, c, len(clusters))
            with open(os.path.join(working_dir, name), "w") as fh:
                fh.write(text)
            written += 1
    return written


def get_cluster_compositions(
    filename,
    atom_type,
    r_cut,
    num_mols,
    num_atoms_per_mol,
    full_trajectory=False,
    frame=None,
    alter_atom_types=False,
    max_force=0.75,
    mol_names=None,
):
    """
    The clusters get_clusters would write, counted instead of written (no files, no elements needed).

    Returns (clusters, compositions):
      clusters: one row per (frame, centre) — frame (index among the processed frames), timestep, centre_id, and
        num_<name> for each molecule type: the passing shell molecules of that type other than the centre's own;
      compositions: the distinct num_* combinations with their count and % of all clusters, by count, descending.
    `mol_names` names the molecule types (default 1, 2, ...).
    """
    names = list(mol_names) if mol_names else [str(i + 1) for i in range(len(num_mols))]
    cols = ["num_%s" % n for n in names]
    _, _, mol_type = _layout(num_mols, num_atoms_per_mol)
    n_types = len(num_mols)
    meta, counts = [], []
    for index, _, ts, _, planes, _, clusters in _iter_clusters(
            filename, atom_type, r_cut, num_mols, num_atoms_per_mol, full_trajectory, frame, None,
            alter_atom_types, max_force, False):
        for p, _, others in clusters:
            meta.append((index, ts, int(planes[0][p])))
            counts.append(np.bincount(mol_type[others] - 1, minlength=n_types))
    clusters = pd.DataFrame(meta, columns=["frame", "timestep", "centre_id"])
    num = np.array(counts, dtype=np.int64).reshape(-1, n_types)
    for k, c in enumerate(cols):
        clusters[c] = num[:, k]
    conf = clusters.groupby(cols).size().rename("count").reset_index()
    conf = conf.sort_values("count", ascending=False, kind="stable").reset_index(drop=True)
    conf["%"] = conf["count"] * 100 / conf["count"].sum()
    return clusters, conf


# ---- the configuration census (cluster_analysis.py:238-457) ----


def _census_columns(n_types, mol_names):
    names = list(mol_names) if mol_names else [str(i + 1) for i in range(n_types)]  # cluster_analysis.py:399-404
    return ["num_%s" % n for n in names], ["atoms_%s" % n for n in names]


TWO_PERCENTAGES = "Two percentage types are provided for determining the top configurations; using cum_perc"
NO_PERCENTAGE = "No percentage type is provided for determining the top configurations"


def _census_frame(names, nums, atoms, num_cols, atoms_cols):
    """One row per cluster: its file name, then the molecules per type, then the coordinating atoms per type."""
    nums = np.asarray(nums, dtype=np.int64).reshape(-1, len(num_cols))
    atoms = np.asarray(atoms, dtype=object).reshape(-1, len(atoms_cols))
    cols = {"cluster": names}
    cols.update((c, nums[:, k]) for k, c in enumerate(num_cols))
    cols.update((c, atoms[:, k]) for k, c in enumerate(atoms_cols))
    return pd.DataFrame(cols, columns=["cluster"] + num_cols + atoms_cols)


def _census_tables(clusters, num_cols, atoms_cols, find_top, perc, cum_perc):
    """
    clusters (name order) -> (configurations, top configurations or None).
    configurations: the distinct (num_*, atoms_*) rows with their count and share of all clusters, most frequent
    first; equal counts fall as pandas' default sort leaves them (what upstream's published CSVs show).
    top configurations (find_top): the leading rows whose running share stays within cum_perc, or, without cum_perc,
    the rows with a share of at least perc; of rows with equal atoms_* only the first stays, and each gets the first
    cluster in name order that shows those atoms_* as its sample.
    """
    conf = clusters.groupby(num_cols + atoms_cols).size().rename("count").reset_index()
    conf = conf.sort_values("count", ascending=False)
    conf["%"] = conf["count"] * 100 / len(clusters)
    if not find_top:
        return conf, None
    if cum_perc and perc:
        warnings.warn(TWO_PERCENTAGES)
    if not (cum_perc or perc):
        raise ValueError(NO_PERCENTAGE)
    chosen = conf["%"].cumsum() <= cum_perc if cum_perc else conf["%"] >= perc
    sample = clusters.drop_duplicates(atoms_cols).set_index(atoms_cols)["cluster"]
    return conf, conf[chosen].drop_duplicates(atoms_cols).join(sample, on=atoms_cols)


def _write_census(working_dir, clusters, conf, top):
    for name, frame in (("top_conf", top), ("clusters", clusters), ("configurations", conf)):
        if frame is not None:
            frame.to_csv(os.path.join(working_dir, name + ".csv"), index=False)


def _read_xyz(path):
    """(element per atom, coordinates [n, 3]) of an xyz file."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    n = int(lines[0])
    rows = [ln.split() for ln in lines[2:2 + n]]
    if len(rows) != n or any(len(r) < 4 for r in rows):
        raise ValueError("%s is not an xyz file of %d atoms" % (path, n))
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:4]] for r in rows], dtype=np.float64).reshape(n, 3)


def _site_string(elements):
    """'1N2O' for N, O, O: the count of every first letter, letters ascending."""
    letters = Counter(e[0] for e in elements)
    return "".join("%d%s" % (letters[ch], ch) for ch in sorted(letters))


def _file_census(path, r_cut, sequences, skip, type_coord_atoms):
    """
    (molecules per type, coordinating-atom strings per type) of one cluster file. The file's first atom is the atom of
    interest and its first `skip` atoms are that atom's molecule; what follows must be whole molecules, each told by
    the first of `sequences` (element lists, one per type) that the atoms at that position spell out.
    """
    els, xyz = _read_xyz(path)
    # coordinating: another atom no farther than r_cut (the bound included) and, when given, of a listed element
    near = np.linalg.norm(xyz - xyz[:1], axis=1) <= r_cut
    near[:1] = False
    if type_coord_atoms:
        near &= np.isin(np.array(els, dtype=object), list(type_coord_atoms))
    strings = [[] for _ in sequences]
    at = skip
    while at < len(els):
        kind = next((k for k, seq in enumerate(sequences) if seq and els[at:at + len(seq)] == seq), None)
        if kind is None:
            raise ValueError(
                "%s: atom %d on (%s ...) starts none of the molecules; the file's first %d atoms are taken for the "
                "molecule of the atom of interest" % (path, at + 1, " ".join(els[at:at + 4]), skip))
        end = at + len(sequences[kind])
        strings[kind].append(_site_string(e for e, hit in zip(els[at:end], near[at:end]) if hit))
        at = end
    return [len(s) for s in strings], [":".join(sorted(s)) for s in strings]


def get_unique_configurations(
    cluster_pattern,
    r_cut,
    molecules,
    mol_num,
    type_coord_atoms=None,
    working_dir=None,
    find_top=True,
    perc=None,
    cum_perc=90,
    mol_names=None,
    zip=True,
):
    """
    The configuration of every cluster file written by get_clusters: per molecule type, how many molecules surround
    the atom of interest (the file's first atom) and which of their atoms are within r_cut of it. Arguments, files
    (clusters.csv, configurations.csv, top_conf.csv, conf_*.xyz, Clusters.zip) and return value as in the reference
    (cluster_analysis.py:238-457); `molecules` may be objects with `.species` or lists of element strings. Host only.

    Unlike the reference, a file whose atoms match no molecule raises ValueError (before anything is written) and the
    files are read in name order.
    """
    working_dir = working_dir or os.getcwd()
    paths = sorted(glob.glob(os.path.join(working_dir, cluster_pattern)))
    sequences = [[str(e) for e in getattr(mol, "species", mol)] for mol in molecules]
    num_cols, atoms_cols = _census_columns(len(sequences), mol_names)
    rows = [_file_census(p, r_cut, sequences, len(sequences[mol_num]), type_coord_atoms) for p in paths]
    clusters = _census_frame([os.path.basename(p) for p in paths], [r[0] for r in rows], [r[1] for r in rows],
                             num_cols, atoms_cols)
    conf, top = _census_tables(clusters, num_cols, atoms_cols, find_top, perc, cum_perc)
    if top is not None:
        for k, name in enumerate(top["cluster"], start=1):
            shutil.copy(os.path.join(working_dir, name), os.path.join(working_dir, "conf_%d.xyz" % k))
    _write_census(working_dir, clusters, conf, top)
    if zip:  # the cluster files end up in Clusters.zip, at its top level, and nowhere else
        with zipfile.ZipFile(os.path.join(working_dir, "Clusters.zip"), "w", zipfile.ZIP_DEFLATED) as archive:
            for p in paths:
                archive.write(p, os.path.basename(p))
        for p in paths:
            os.remove(p)
    return clusters, conf


def _coordination_classes(el, type_coord_atoms):
    """(class letters, sorted; class per atom uint8, 0xFF for an element that is not counted)."""
    uniq, inv = np.unique(np.asarray(el, dtype=str), return_inverse=True)
    counted = [str(e) for e in uniq if not type_coord_atoms or e in type_coord_atoms]
    letters = sorted({e[0] for e in (type_coord_atoms if type_coord_atoms else counted)})
    per_el = np.array([letters.index(e[0]) if e in counted else backend.COORD_NO_CLASS for e in uniq])
    if len(letters) > backend.COORD_CLASSES:
        raise ValueError("%d coordination classes (%s): at most %d first letters can be told apart" % (
            len(letters), " ".join(letters), backend.COORD_CLASSES))
    return letters, per_el.astype(np.uint8)[inv]


def _sample_text(src, index, c, r_shell_sq):
    """The text get_clusters writes for centre c of processed frame `index`: the frame read and searched again."""
    fr = src.reread(index)
    p = int(fr[4][c])
    xyz, box, passes = src.staged([fr])
    mols, count = backend.shell_members(xyz, box, fr[4][c:c + 1], src.mol_of, r_shell_sq)
    own_ok, others = _cluster_members(mols[0, 0, :count[0, 0]], passes[0], src.mol_of[p])
    return _cluster_text(fr[2][2:5], fr[1], p, own_ok, others, fr[3], src.mol_of, src.seg_off)


def get_configurations(
    filename,
    atom_type,
    r_cut,
    num_mols,
    num_atoms_per_mol,
    elements=None,
    coord_r_cut=None,
    type_coord_atoms=None,
    full_trajectory=False,
    frame=None,
    alter_atom_types=False,
    max_force=0.75,
    find_top=True,
    perc=None,
    cum_perc=90,
    mol_names=None,
    working_dir=None,
):
    """
    get_clusters and get_unique_configurations in one pass over the trajectory, without a cluster file in between: the
    clusters within r_cut of every atom of type `atom_type` (arguments as get_clusters), and per cluster the atoms of
    its molecules within coord_r_cut (default r_cut) of the centre, of the elements `type_coord_atoms` (default all).

    Returns (clusters, configurations) with the columns, dtypes and order of get_unique_configurations; `cluster` is
    the name get_clusters gives the cluster's file. With `working_dir`, writes clusters.csv and configurations.csv
    and, with find_top, top_conf.csv and the conf_k.xyz of the chosen samples (the text get_clusters writes).

    Distances are the dump's doubles against strict <, where the file route compares 10-decimal text with <=; the
    molecules are known by layout, not matched by element sequence, and a centre whose own molecule fails the force
    filter is counted like any other.
    """
    src = _Source(filename, atom_type, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
                  alter_atom_types, max_force, True)
    n_types = len(num_mols)
    num_cols, atoms_cols = _census_columns(n_types, mol_names)
    rs2 = r_cut ** 2
    rc2 = (r_cut if coord_r_cut is None else coord_r_cut) ** 2
    names, keys, where, letters_of = [], [], [], []
    n_frames, batches = src.batches(same=lambda fr: fr[3])
    for first, batch in batches:
        centres = batch[0][4]
        letters, cls = _coordination_classes(batch[0][3], type_coord_atoms)
        xyz, box, passes = src.staged(batch)
        mols, words, count = backend.shell_coordination(xyz, box, centres, src.mol_of, src.seg_off, src.mol_type, cls,
                                                        rs2, rc2, passes=passes)
        B, C_, K = mols.shape
        f_part = np.char.zfill(np.arange(first, first + B).astype(str), len(str(n_frames)))
        c_part = np.char.zfill(np.arange(C_).astype(str), len(str(C_)))
        names.append(np.char.add(np.char.add(np.char.add("Cluster_", f_part)[:, None], "_"),
                                 np.char.add(c_part, ".xyz")[None, :]).ravel())
        types = np.where(mols >= 0, src.mol_type[np.maximum(mols, 0)], 0).astype(np.uint64)
        keys.append((np.concatenate([types, words], axis=2).reshape(B * C_, 2 * K), len(letters_of)))
        letters_of.append(letters)
        where.append(np.stack([np.repeat(np.arange(first, first + B), C_), np.tile(np.arange(C_), B)], axis=1))
    names = np.concatenate(names) if names else np.zeros(0, dtype=str)
    where = np.concatenate(where) if where else np.zeros((0, 2), dtype=np.int64)

    # the distinct canonical rows, their strings built once each
    nums, atoms = np.zeros((len(names), n_types), dtype=np.int64), np.empty((len(names), n_types), dtype=object)
    at = 0
    for key, b in keys:
        K = key.shape[1] // 2
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = np.asarray(inv).ravel()
        u_num = np.stack([(uniq[:, :K] == t + 1).sum(axis=1) for t in range(n_types)], axis=1)
        u_atoms = np.empty((len(uniq), n_types), dtype=object)
        for i, row in enumerate(uniq):
            per_type = [[] for _ in range(n_types)]
            for t, w in zip(row[:K], row[K:]):
                if t:
                    per_type[int(t) - 1].append("".join(
                        "%d%s" % ((int(w) >> (8 * k)) & 0xFF, ch) for k, ch in enumerate(letters_of[b])
                        if (int(w) >> (8 * k)) & 0xFF))
            u_atoms[i] = [":".join(sorted(s)) for s in per_type]
        nums[at:at + len(inv)] = u_num[inv]
        atoms[at:at + len(inv)] = u_atoms[inv]
        at += len(inv)
    clusters = _census_frame(names, nums, atoms, num_cols, atoms_cols)
    conf, top = _census_tables(clusters, num_cols, atoms_cols, find_top, perc, cum_perc)
    if working_dir:
        if top is not None:
            for k, name in enumerate(top["cluster"], start=1):
                index, c = where[int(np.flatnonzero(names == name)[0])]
                with open(os.path.join(working_dir, "conf_%d.xyz" % k), "w") as fh:
                    fh.write(_sample_text(src, int(index), int(c), rs2))
        _write_census(working_dir, clusters, conf, top)
    return clusters, conf
