"""
Solvation-shell clusters from LAMMPS dumps — drop-in for get_clusters of
/root/reference/mdproptools/structural/cluster_analysis.py:47-235 (same signature, defaults, files and return value),
plus get_cluster_compositions, which counts the same clusters without writing them.

What runs where
  GPU (libmdhip.so, csrc/clusters.hip): the shell search — every centre of a batch of frames against every atom with
      the reference's single-wrap rsq (cluster_analysis.py:127-142) — and the per-molecule force sums of the filter
      (pandas' compensated groupby().sum(), cluster_analysis.py:146-152).
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

import os

import numpy as np
import pandas as pd

from .. import backend
from .. import io as mio
from ..common.com_mols import check_atom_count, molecule_layout
from .rdf_cn import _calc_atom_type

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
    mol_of = np.repeat(np.arange(len(mol_type), dtype=np.int32), np.diff(seg_off))
    return mol_of, seg_off, mol_type


def _frame_refs(filename):
    """(file, frame within the file) of every frame, in parse_lammps_dumps order."""
    refs = []
    for fname in mio._sorted_matches(filename):
        if str(fname).endswith(".gz"):
            n = sum(1 for _ in mio._iter_frames(fname))
        else:
            nd = mio.NativeDumpFile(fname)
            n = nd.n_frames
            nd.close()
        refs += [(fname, k) for k in range(n)]
    return refs


def _read_frame(fname, k):
    """(timestep, bounds [3,2], column names, planes [8, N] of _COLS sorted by id) of frame k of one file."""
    if str(fname).endswith(".gz"):
        ts, bounds, _, names, planes = mio._pandas_file_frames(fname, _COLS, "id")[k]
        return ts, bounds, names, planes
    nd = mio.NativeDumpFile(fname)
    try:
        ts, _, bounds, _, names = nd.header(k)
        return ts, bounds, names, nd.read(k, _COLS, sort_by="id")
    finally:
        nd.close()


def _element_column(fname, k):
    """The dump's own `element` column of frame k, in id order (text: the pandas route)."""
    for j, lines in enumerate(mio._iter_frames(fname)):
        if j == k:
            df = mio.LammpsDump.from_lines(lines).data.sort_values(by=["id"])
            return df["element"].to_numpy()
    raise IndexError(k)


def _frames(filename, full_trajectory, frame):
    """-> (number of frames processed, iterator of (file, frame in file, timestep, bounds, names, planes))."""
    refs = _frame_refs(filename)
    if not full_trajectory:
        refs = [refs[frame]]  # dumps[frame] (cluster_analysis.py:104-107): Python indexing, its errors included

        def one():
            fname, k = refs[0]
            yield (fname, k) + _read_frame(fname, k)

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


def _iter_clusters(filename, atom_type, r_cut, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
                   alter_atom_types, max_force, need_elements):
    """
    Yields per processed frame: (frame index, number of frames, timestep, lengths [3], planes [8, N] of _COLS,
    element per atom or None, clusters), clusters a list over the frame's centres (id order) of (centre position,
    own molecule passes, passing shell molecules other than the centre's own, ascending).
    """
    mol_of, seg_off, _ = _layout(num_mols, num_atoms_per_mol)
    n_atoms = int(seg_off[-1])
    el_map = np.asarray(elements, dtype=object) if elements else None
    n_frames, frames = _frames(filename, full_trajectory, frame)
    rc2 = r_cut ** 2  # cluster_analysis.py:140

    def prepare(item):
        fname, k, ts, bounds, names, planes = item
        check_atom_count(n_atoms, planes.shape[1])
        if need_elements and "element" not in names and not elements:  # cluster_analysis.py:122-126
            raise ValueError(
                "The elements of the atoms in the system should be provided if they "
                "are not in the dump files."
            )
        el = None
        if need_elements:
            el = el_map[planes[1].astype(np.int64) - 1] if elements else _element_column(fname, k)
        types = _calc_atom_type(planes[0], num_mols, num_atoms_per_mol) if alter_atom_types else planes[1]
        lengths = np.asarray(bounds, dtype=np.float64)
        lengths = lengths[:, 1] - lengths[:, 0]
        return ts, lengths, planes, el, np.flatnonzero(types == atom_type).astype(np.int32)

    def run(batch, first):
        centres = batch[0][4]
        xyz = np.ascontiguousarray(np.stack([b[2][2:5] for b in batch]))
        force = np.ascontiguousarray(np.stack([b[2][5:8] for b in batch]))
        box = np.stack([b[1] for b in batch])
        mols, count = backend.shell_members(xyz, box, centres, mol_of, rc2)
        passes = backend.mol_kahan_sums(force, seg_off).min(axis=1) * FORCE_CONSTANT < max_force  # [B, M]
        for j, (ts, lengths, planes, el, _) in enumerate(batch):
            clusters = []
            for c, p in enumerate(centres):
                shell = mols[j, c, :count[j, c]]
                passing = shell[passes[j, shell]]
                own = mol_of[p]
                own_ok = bool((passing == own).any())
                clusters.append((int(p), own_ok, passing[passing != own]))
            yield first + j, n_frames, ts, lengths, planes, el, clusters

    batch, first, index = [], 0, 0
    per_frame = 6 * n_atoms * 8
    for item in frames:
        fr = prepare(item)
        if batch and (len(batch) * per_frame >= MAX_BATCH_BYTES or not np.array_equal(fr[4], batch[0][4])):
            yield from run(batch, first)
            batch, first = [], index
        batch.append(fr)
        index += 1
    if batch:
        yield from run(batch, first)


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
    sizes = np.diff(seg_off)
    written = 0
    for index, n_frames, ts, lengths, planes, el, clusters in _iter_clusters(
            filename, atom_type, r_cut, num_mols, num_atoms_per_mol, full_trajectory, frame, elements,
            alter_atom_types, max_force, True):
        xyz = planes[2:5]
        half = lengths / 2
        for c, (p, own_ok, others) in enumerate(clusters):
            rows = _row_index(seg_off[others], sizes[others])
            if own_ok:
                own = np.arange(seg_off[mol_of[p]], seg_off[mol_of[p] + 1])
                rows = np.concatenate(([p], own[own != p], rows))
            pos = xyz[:, rows]
            d = pos - xyz[:, p][:, None]
            cond = (d > half[:, None]) | (d < -half[:, None])  # _remove_boundary_effects, cluster_analysis.py:32-44
            pos = np.where(cond, pos - np.sign(d) * lengths[:, None], pos)
            vals = np.empty((len(rows), 4), dtype=object)
            vals[:, 0] = el[rows]
            vals[:, 1:] = pos.T
            text = "{}\n\n".format(len(rows)) + (_ROW_FMT * len(rows)) % tuple(vals.ravel())
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
