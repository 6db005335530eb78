"""
Radial distribution functions and coordination numbers from LAMMPS dumps —
drop-in for /root/reference/mdproptools/structural/rdf_cn.py (same public
functions, positional order, defaults, return types, CSV side effects and
exception types: rdf_cn.py:385-396, 533-544, 654-665, 759-770).

What runs where
  GPU (libmdhip.so): every pair loop — `_rdf_loop`, `_cn_loop`,
      `_rdf_mol_loop`, `_cn_mol_loop` (rdf_cn.py:72-162) — and the molecule
      centres of mass (`_define_mol_cols`, rdf_cn.py:218-241), for all frames
      of a batch in one call; integer histograms come back per frame.
  Host (numpy, this file): parsing, id sorting, the altered-id remap
      (rdf_cn.py:197-215, vectorised), densities and the per-frame
      normalisation in the reference's operation order (rdf_cn.py:288-291,
      312-328), the frame average and the CSV. Because the histograms are
      exact integers and the normalisation repeats the reference's float
      operations in order, g(r) and CN come out bit-identical.

Differences, all deliberate:
  * pairs whose bin index would be == num_bins (reachable when r_cut/bin_size
    rounds up, e.g. 20/0.05) are dropped and reported instead of written out of
    bounds (the numba build corrupts memory there; plain numpy raises);
  * progress lines are printed only when `rdf_cn.VERBOSE` is true.
"""

from timeit import default_timer as timer

import numpy as np
import pandas as pd

from .. import backend
from ..common import sayer
from ..common.com_mols import calc_atom_type, check_atom_count, molecule_layout
from ..common.tables import write_csv as _write_csv
from ..common.trajectory import all_frames, batches, lengths_block, load_frames, same_labels, xyz_block
from ..dist import is_writer

CON_CONSTANT = 1.660538921  # amu/A^3 -> g/cm^3 (rdf_cn.py:30)
VERBOSE = False
MAX_BATCH_BYTES = 1 << 30  # coordinates staged per library call
STREAM = True  # parse the next batch of frames (into page-locked staging buffers) while the GPU runs the current one;
               # the frames of a trajectory are then never all resident on the host (mdproptools_amd/stream.py)

_R_LABEL = "r ($\\AA$)"


_say = sayer(globals())


# ------------------------------------------------------------------------------------------------
# host-side pieces
# ------------------------------------------------------------------------------------------------


def _initialize(r_cut, bin_size, filename, partial_relations):
    """Parsed frames, bins, radii and relation count (rdf_cn.py:165-180)."""
    if isinstance(r_cut, list):
        num_bins = [int(rc / bin_size) for rc in r_cut]
        radii = [(np.arange(nb) + 0.5) * bin_size for nb in num_bins]
    else:
        num_bins = int(r_cut / bin_size)
        radii = (np.arange(num_bins) + 0.5) * bin_size
    dumps = load_frames(filename, shard=True, stream=STREAM,
                        on_frame=lambda ts: _say("The timestep of the current file is: " + str(ts)))
    return dumps, num_bins, radii, len(partial_relations[0])


def _type_counts(labels):
    """{label: number of atoms} — what `np.unique(..., return_counts=True)` gives (rdf_cn.py:253-256), by a counting
    pass when the labels are small non-negative integers (always, for LAMMPS types and altered ids): O(n), no sort."""
    lab = np.asarray(labels).astype(np.int64)
    if lab.size and lab.min() >= 0 and lab.max() < (1 << 20):
        cnt = np.bincount(lab)
        vals = np.flatnonzero(cnt)
        return {int(v): int(cnt[v]) for v in vals}
    vals, cnt = np.unique(lab, return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, cnt)}


def _calc_props(box_lengths, ref_labels, obj_labels, num_types, mass, partial_relations, altered,
                num_atoms_per_mol=None, atom_types=None):
    """
    Densities and consistency checks of one frame (rdf_cn.py:244-294). `atom_types`: the `_type_counts` of ref_labels
    when the caller has them already. Returns (rho, rho_pairs, atom_types, object_types).
    """
    n_objects = len(obj_labels)
    volume = np.prod(box_lengths)
    if atom_types is None:
        atom_types = _type_counts(ref_labels)
    object_types = atom_types if obj_labels is ref_labels else _type_counts(obj_labels)
    expected = np.sum(num_atoms_per_mol) if altered else num_types
    if expected != len(atom_types):
        raise ValueError(
            "Consistency check failed: Number of specified atomic types is different from the "
            f"calculated value specified= {num_atoms_per_mol if altered else num_types}, "
            f"calculated= {len(atom_types)}")
    # rdf_cn.py:280-282 — needs the labels 1..num_types to be present (KeyError otherwise)
    total_mass = np.sum([float(mass[i]) * float(atom_types[i + 1]) for i in range(num_types)])
    total_density = float((total_mass / volume) * CON_CONSTANT)
    _say("{0:s}{1:10.8f}".format("Average density=", total_density))
    rho = n_objects / volume
    rho_pairs = np.zeros(len(partial_relations[1]))
    for k, obj in enumerate(partial_relations[1]):
        rho_pairs[k] = object_types[obj] / volume
        if rho_pairs[k] < 1.0e-22:
            raise ValueError("Error: Density is zero for mol type: " + str(obj))
    return rho, rho_pairs, atom_types, object_types


def _shell_volume(bin_size, num_bins):
    edges3 = np.arange(1, num_bins + 1) ** 3 - np.arange(num_bins) ** 3
    return 4 / 3 * np.pi * bin_size ** 3 * edges3  # rdf_cn.py:312-318


def _normalize_rdf_batch(bin_size, props, partial_relations, num_relations, num_bins, part, full=None, num_atoms=None):
    """The normalisation of all B frames of a batch in ONE numpy expression per output, each element through the
    reference's operations in the reference's order (rdf_cn.py:297-329):
        g_full[k][b]    = h / ((num_atoms_k * rho_k) * shell[b])
        g_part[k][r][b] = h / ((n_ref[k][r] * rho_pair[k][r]) * shell[b])
    (the reference tiles n_ref, rho_pair and the shell volumes to [R, nb] and multiplies left to right: the same two
    products per element, so the doubles are the same: tests/test_dropin_host_cpu.py keeps the per-frame restatement).
    part uint64 [B,R,nb], full uint64 [B,nb] or None. Returns rows [B, (1 + R) * nb]: g_full | g_part (or [B, R * nb]
    without `full`)."""
    B = len(props)
    sv = _shell_volume(bin_size, num_bins)
    n_ref = np.array([[p[2][a] for a in partial_relations[0]] for p in props]).reshape(B, num_relations)
    rho_b = np.stack([p[1] for p in props]).reshape(B, num_relations)
    g_part = np.asarray(part).astype(np.float64) / ((n_ref * rho_b)[:, :, None] * sv[None, None, :])
    if full is None:
        return g_part.reshape(B, num_relations * num_bins)
    na_rho = np.array([n * p[0] for n, p in zip(num_atoms, props)])
    g_full = np.asarray(full).astype(np.float64) / (na_rho[:, None] * sv[None, :])
    return np.concatenate([g_full, g_part.reshape(B, num_relations * num_bins)], axis=1)


def _normalize_cn_batch(props, partial_relations, raw):
    """Coordination numbers of all B frames of a batch: raw counts uint64 [B,R] over the number of reference atoms of
    each frame and relation (rdf_cn.py:332-338). Returns rows [B, R]."""
    n_ref = np.array([[p[2][a] for a in partial_relations[0]] for p in props])
    return np.asarray(raw).astype(np.float64) / n_ref


def _sum_frames(rows):
    """Sum of the per-frame rows in FRAME ORDER, one addition per frame and element as the reference's
    `rdf_full_sum += ...` loop (rdf_cn.py:514-515; numpy's own sum would add pairwise: other roundings)."""
    acc = np.zeros(rows.shape[1])
    for row in rows:
        acc += row
    return acc


class _PropsCache:
    """What one public call remembers from one frame to the next — the frames of a trajectory nearly always carry the
    same labels, and NVT ones the same box: the type counts of the last labels, the `_calc_props` of the last (box,
    labels) and the int32 copy of the stream's `types_ref`. One per public call: nothing survives it."""

    def __init__(self):
        self.counted = self.counts = None
        self.key = self.ref = self.val = None
        self.i32_of = self.i32 = None

    def type_counts(self, labels):
        """`_type_counts`; the comparison with the last labels (a memcmp) is several times cheaper than the count."""
        lab = np.asarray(labels)
        if self.counted is None or self.counted.shape != lab.shape or not np.array_equal(self.counted, lab):
            self.counted, self.counts = lab.copy(), _type_counts(lab)
        return self.counts

    def props(self, box_lengths, ref_labels, obj_labels, num_types, mass, partial_relations, altered,
              num_atoms_per_mol=None):
        """`_calc_props`, computed once for consecutive frames with the same box and the same labels: the densities are
        functions of exactly those. Not remembered with VERBOSE (the density line is printed per frame there, as the
        reference does)."""
        def fresh():
            return _calc_props(box_lengths, ref_labels, obj_labels, num_types, mass, partial_relations, altered,
                               num_atoms_per_mol, atom_types=self.type_counts(ref_labels))

        if VERBOSE:
            return fresh()
        key = (tuple(float(x) for x in box_lengths), num_types, tuple(float(x) for x in mass),
               tuple(map(tuple, partial_relations)), altered, None if num_atoms_per_mol is None else tuple(num_atoms_per_mol))
        # (the SAME array object as last time — the stream hands `types_ref` to every batch whose frames the reader
        # threads found unchanged — needs no comparison; another array is compared value by value)
        if (self.key is not None and self.key[0] == key
                and (self.ref is ref_labels
                     or (self.key[1].shape == np.shape(ref_labels) and np.array_equal(self.key[1], ref_labels)))
                and (obj_labels is ref_labels or (self.key[2] is not None and np.array_equal(self.key[2], obj_labels)))):
            return self.val
        self.val = fresh()
        self.key = (key, np.array(ref_labels, copy=True),
                    None if obj_labels is ref_labels else np.array(obj_labels, copy=True))
        self.ref = ref_labels
        return self.val

    def int32(self, labels):
        if self.i32_of is not labels:
            self.i32_of, self.i32 = labels, labels.astype(np.int32)
        return self.i32


def _labels_and_props(cache, batch, altered, num_mols, num_atoms_per_mol, num_types, mass, partial_relations):
    """(labels for the library — int32 [N], or [F, N] when they change —, the per-frame `_calc_props` tuples) of one
    batch (rdf_cn.py:462-482). A streamed batch whose frames all carry the first frame's types (the reader threads
    compared them while the text was in their caches) takes one label array and, with a constant box, one set of
    densities for all its frames."""
    if not altered and getattr(batch, "uniform_types", False) and batch.types_ref is not None:
        lab = batch.types_ref
        return cache.int32(lab), [cache.props(f.lengths, lab, lab, num_types, mass, partial_relations, altered,
                                              num_atoms_per_mol) for f in batch]
    labels = [(calc_atom_type(f.ids, num_mols, num_atoms_per_mol) if altered else f.types) for f in batch]
    props = [cache.props(f.lengths, lab, lab, num_types, mass, partial_relations, altered, num_atoms_per_mol)
             for f, lab in zip(batch, labels)]
    return same_labels(labels).astype(np.int32), props


def _save_rdf(radii, relation_matrix, path_or_buf, save_mode, rdf_part_sum, rdf_full_sum=None):
    """Same columns and CSV behaviour as rdf_cn.py:341-365."""
    cols = [_R_LABEL] + (["g_full(r)"] if rdf_full_sum is not None else [])
    cols += [f"g_{pair[0]}-{pair[1]}" for pair in relation_matrix]
    blocks = (radii, rdf_full_sum, rdf_part_sum) if rdf_full_sum is not None else (radii, rdf_part_sum)
    final_df = pd.DataFrame(np.vstack(blocks).transpose(), columns=cols)
    if save_mode:
        _write_csv(final_df, path_or_buf)
        _say("Results are written to pd.DataFrame and csv file")
    else:
        _say(final_df)
    return final_df


def _save_cn(relation_matrix, path_or_buff, cn_sum, save_mode):
    cols = [f"cn_{pair[0]}-{pair[1]}" for pair in relation_matrix]
    final_df = pd.DataFrame(np.vstack(cn_sum).transpose(), columns=cols)
    if save_mode:
        _write_csv(final_df, path_or_buff)
        _say("CN results are written to pd.DataFrame and csv file")
    else:
        _say(final_df)
    return final_df


# ------------------------------------------------------------------------------------------------
# the frame pipeline: batches -> normalised rows per frame -> mean over the frames
# ------------------------------------------------------------------------------------------------


def _mean_over_frames(frames, per_batch, width):
    """The loop every public function runs: `per_batch(batch)` makes the backend call of one batch and returns the
    normalised rows [B, width] of its frames — every frame with ITS box and densities (rdf_cn.py:502-513). Then every
    rank's rows in frame order, summed in that order, over their number (rdf_cn.py:514-521)."""
    rows = all_frames([per_batch(batch) for batch in batches(frames, MAX_BATCH_BYTES)])  # (identity in one process)
    return (_sum_frames(rows) if len(rows) else np.zeros(width)) / len(rows)


def _joined(blocks):
    """The per-run blocks of a batch as one array; the usual single run is handed on as it is."""
    return blocks[0] if len(blocks) == 1 else np.concatenate(blocks)


def _finished(batch, what):
    for f in batch:
        _say("Finished computing " + what + " for timestep", f.timestep)


def _report_dropped(name, dropped, num_bins):
    if dropped:
        print(f"{name}: {dropped} pair(s) fell in bin index {num_bins} (== num_bins) and were dropped")


def _type_runs(batch):
    """(start, stop) of the maximal runs of consecutive frames of a batch that carry the same types."""
    cuts = [k for k in range(1, len(batch)) if not np.array_equal(batch[k].types, batch[k - 1].types)]
    return list(zip([0] + cuts, cuts + [len(batch)]))


def _molecule_sites(batch, runs, num_mols, num_atoms_per_mol, mass):
    """(wrapped coordinates [B,3,N], their per-molecule centres of mass [B,3,M] from the device, molecule types int32
    [M]) of a batch (rdf_cn.py:218-241): the masses go with the types, so one call per run of equal types, each on its
    slice of the batch's coordinate block."""
    seg_off, seg_type, _ = molecule_layout(num_mols, num_atoms_per_mol)  # (rdf_cn.py:222-230)
    check_atom_count(seg_off[-1], batch[0].xyz.shape[1])
    xyz = xyz_block(batch)
    sites = [backend.segment_com(xyz[a:b], np.asarray(mass, dtype=np.float64)[batch[a].types.astype(np.int64) - 1],
                                 seg_off)[0] for a, b in runs]
    return xyz, _joined(sites), seg_type.astype(np.int32)


# ------------------------------------------------------------------------------------------------
# public functions
# ------------------------------------------------------------------------------------------------


def calc_atomic_rdf(r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols=None,
                    num_atoms_per_mol=None, path_or_buff="rdf.csv", save_mode=True):
    """
    Full and partial atom-atom g(r) averaged over the frames of `filename` (rdf_cn.py:385-530).

    Args follow the reference: r_cut (float), bin_size (float), num_types (int), mass (list of
    float, one per atom type), partial_relations ([[reference types], [other types]]), filename
    (dump file or '*' pattern), num_mols / num_atoms_per_mol (give both to use altered atom ids:
    the index of an atom inside its molecule type), path_or_buff, save_mode.
    Returns a DataFrame with columns r, g_full(r), g_a-b ...
    """
    dumps, num_bins, radii, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    altered = bool(num_mols and num_atoms_per_mol)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache, dropped = _PropsCache(), 0

    def per_batch(batch):
        nonlocal dropped
        start = timer()
        lab_arg, props = _labels_and_props(cache, batch, altered, num_mols, num_atoms_per_mol, num_types, mass,
                                           partial_relations)
        full, part, ov = backend.rdf_loop(xyz_block(batch), lab_arg, lengths_block(batch), relation_matrix, r_cut,
                                          bin_size, num_bins, per_frame=True)
        dropped += ov
        rows = _normalize_rdf_batch(bin_size, props, partial_relations, num_relations, num_bins, part, full,
                                    [f.xyz.shape[1] for f in batch])
        _finished(batch, "RDF")
        _say("Trajectory loop took:", timer() - start, "s")
        return rows

    mean = _mean_over_frames(dumps, per_batch, (1 + num_relations) * num_bins)
    _report_dropped("calc_atomic_rdf", dropped, num_bins)
    return _save_rdf(radii, relation_matrix, path_or_buff, save_mode and is_writer(),
                     mean[num_bins:].reshape(num_relations, num_bins), rdf_full_sum=mean[:num_bins])


def calc_atomic_cn(r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols=None,
                   num_atoms_per_mol=None, path_or_buff="cn.csv", save_mode=True):
    """
    Atom-atom coordination numbers, one cutoff per relation (rdf_cn.py:533-651). r_cut is a list.
    Returns a one-row DataFrame with columns cn_a-b.
    """
    dumps, _, _, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    altered = bool(num_mols and num_atoms_per_mol)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache = _PropsCache()

    def per_batch(batch):
        lab_arg, props = _labels_and_props(cache, batch, altered, num_mols, num_atoms_per_mol, num_types, mass,
                                           partial_relations)
        raw = backend.cn_loop(xyz_block(batch), lab_arg, lengths_block(batch), relation_matrix, list(r_cut),
                              per_frame=True)
        _finished(batch, "CN")
        return _normalize_cn_batch(props, partial_relations, raw)

    mean = _mean_over_frames(dumps, per_batch, num_relations)
    return _save_cn(relation_matrix, path_or_buff, mean, save_mode and is_writer())


def calc_atomic_rdf_cn(r_cut, cn_r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols=None,
                       num_atoms_per_mol=None, rdf_path_or_buff="rdf.csv", cn_path_or_buff="cn.csv", save_mode=True):
    """
    `calc_atomic_rdf(r_cut, ...)` and `calc_atomic_cn(cn_r_cut, ...)` (rdf_cn.py:385-651) of the same trajectory in
    ONE pass: the dump files are read once and every frame goes through one pair sweep that yields the histograms and
    the coordination counts (mdhip_rdf_cn_atomic). Returns (rdf DataFrame, cn DataFrame) — bit for bit the frames the
    two separate calls return, and the same two CSV files. (Not in the reference, which runs the two functions one
    after the other over the same pairs: BASELINE config 3 asks for both.)
    """
    dumps, num_bins, radii, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    if len(cn_r_cut) != num_relations:
        raise ValueError("one coordination cutoff per relation is required")
    altered = bool(num_mols and num_atoms_per_mol)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache, dropped = _PropsCache(), 0

    def per_batch(batch):
        nonlocal dropped
        lab_arg, props = _labels_and_props(cache, batch, altered, num_mols, num_atoms_per_mol, num_types, mass,
                                           partial_relations)
        full, part, ov, raw = backend.rdf_cn_loop(xyz_block(batch), lab_arg, lengths_block(batch), relation_matrix,
                                                  r_cut, bin_size, num_bins, list(cn_r_cut), per_frame=True)
        dropped += ov
        _finished(batch, "RDF and CN")
        g = _normalize_rdf_batch(bin_size, props, partial_relations, num_relations, num_bins, part, full,
                                 [f.xyz.shape[1] for f in batch])
        return np.concatenate([g, _normalize_cn_batch(props, partial_relations, raw)], axis=1)  # g_full | g_part | cn

    split = (1 + num_relations) * num_bins
    mean = _mean_over_frames(dumps, per_batch, split + num_relations)
    _report_dropped("calc_atomic_rdf_cn", dropped, num_bins)
    g = _save_rdf(radii, relation_matrix, rdf_path_or_buff, save_mode and is_writer(),
                  mean[num_bins:split].reshape(num_relations, num_bins), rdf_full_sum=mean[:num_bins])
    c = _save_cn(relation_matrix, cn_path_or_buff, mean[split:], save_mode and is_writer())
    return g, c


def calc_molecular_rdf(r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols,
                       num_atoms_per_mol, path_or_buff="rdf_mol.csv", save_mode=True):
    """
    Partial g(r) between atoms (first list of partial_relations) and molecule centres of mass
    (second list: molecule type numbers) (rdf_cn.py:654-756).
    """
    dumps, num_bins, radii, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache, dropped = _PropsCache(), 0

    def per_batch(batch):
        nonlocal dropped
        runs = _type_runs(batch)
        xyz, sites, seg_type = _molecule_sites(batch, runs, num_mols, num_atoms_per_mol, mass)
        props = [cache.props(f.lengths, f.types, seg_type, num_types, mass, partial_relations, False) for f in batch]
        box = lengths_block(batch)
        parts = []
        for a, b in runs:
            part, ov = backend.rdf_mol_loop(xyz[a:b], batch[a].types.astype(np.int32), sites[a:b], seg_type, box[a:b],
                                            relation_matrix, r_cut, bin_size, num_bins, per_frame=True)
            parts.append(part)
            dropped += ov
        _finished(batch, "RDF")
        return _normalize_rdf_batch(bin_size, props, partial_relations, num_relations, num_bins, _joined(parts))

    mean = _mean_over_frames(dumps, per_batch, num_relations * num_bins)
    _report_dropped("calc_molecular_rdf", dropped, num_bins)
    return _save_rdf(radii, relation_matrix, path_or_buff, save_mode and is_writer(),
                     mean.reshape(num_relations, num_bins))


def calc_molecular_cn(r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols,
                      num_atoms_per_mol, path_or_buff="cn_mol.csv", save_mode=True):
    """Atom - molecule-COM coordination numbers, one cutoff per relation (rdf_cn.py:759-855)."""
    dumps, _, _, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache = _PropsCache()

    def per_batch(batch):
        runs = _type_runs(batch)
        xyz, sites, seg_type = _molecule_sites(batch, runs, num_mols, num_atoms_per_mol, mass)
        props = [cache.props(f.lengths, f.types, seg_type, num_types, mass, partial_relations, False) for f in batch]
        box = lengths_block(batch)
        raw = [backend.cn_mol_loop(xyz[a:b], batch[a].types.astype(np.int32), sites[a:b], seg_type, box[a:b],
                                   relation_matrix, list(r_cut)) for a, b in runs]
        _finished(batch, "CN")
        return _normalize_cn_batch(props, partial_relations, _joined(raw))

    mean = _mean_over_frames(dumps, per_batch, num_relations)
    return _save_cn(relation_matrix, path_or_buff, mean, save_mode and is_writer())


def calc_intermolecular_rdf(r_cut, bin_size, num_types, mass, partial_relations, filename, num_mols,
                            num_atoms_per_mol, path_or_buff="rdf_mol.csv", save_mode=True):
    """
    Molecule-COM to molecule-COM partial g(r) (rdf_cn.py:857-903; undocumented upstream, a molecule is
    paired with itself as there). partial_relations holds molecule type numbers on both sides.
    """
    dumps, num_bins, radii, num_relations = _initialize(r_cut, bin_size, filename, partial_relations)
    relation_matrix = np.asarray(partial_relations).transpose()
    cache = _PropsCache()

    def per_batch(batch):
        _, sites, seg_type = _molecule_sites(batch, _type_runs(batch), num_mols, num_atoms_per_mol, mass)
        props = [cache.props(f.lengths, seg_type, seg_type, num_types, mass, partial_relations, False) for f in batch]
        # (no atom types in this sweep: one call for the batch, whatever the runs)
        part, _ = backend.rdf_mol_loop(sites, seg_type, sites, seg_type, lengths_block(batch), relation_matrix, r_cut,
                                       bin_size, num_bins, per_frame=True)
        return _normalize_rdf_batch(bin_size, props, partial_relations, num_relations, num_bins, part)

    mean = _mean_over_frames(dumps, per_batch, num_relations * num_bins)
    return _save_rdf(radii, relation_matrix, path_or_buff, save_mode and is_writer(),
                     mean.reshape(num_relations, num_bins))
