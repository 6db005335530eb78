"""
Orientational pair correlations: how the orientations of DIFFERENT molecules are correlated in space — the
distance-resolved dipole-dipole correlation <cos theta>(r) and <P2(cos theta)>(r), its running sum, the Kirkwood factor
G_K(R), and the orientation of a molecule's vector against the direction to an ion or to another molecule, for any pair
of species. The reference has no such module; include/mdhip.h (mdhip_mol_moments, mdhip_vector_pair_hist) holds the
specification and tests/dipole_ref.py restates it in numpy. Arguments follow `calc_atomic_rdf` and `Reorientation`.

What runs where
  GPU (libmdhip.so): per batch of frames `mdhip_mol_moments` (csrc/moments.hip) reduces every molecule of a species to a
      site and a unit vector, which stay on the device; `mdhip_vector_pair_hist` (csrc/vector_pairs.hip) sweeps all pairs
      of a job's two species: the bin of the site-site distance and, per bin, the pair count and the exact fixed-point
      sums of cos theta, cos^2 theta and of the cosine against the pair direction.
  Host: parsing (common/trajectory.py: the frames are never all resident), the species and their term lists, adding the
      batches' integers (exactly: Python integers), the divisions and the CSV files.
"""

import math
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import mol_series
from ..common import trajectory as T
from ..dist import is_writer

# True: the dumps are parsed into page-locked staging batches and each is reduced on the GPU while the next one is
# being parsed (mdproptools_amd/stream.py). False: every frame is parsed first and reduced in one call.
STREAM = True
BATCH_BYTES = None  # bytes of coordinates per streamed batch (None: the stream's own default)

ONE = backend.VECTOR_PAIR_ONE  # the fixed-point unit of the sums


def species_label(sp):
    mol_type, vector, site = sp
    vec = "-" if vector is None else ("dipole" if vector == "dipole" else "%d-%d" % vector)
    return "%d:%s@%s" % (mol_type, vec, site)


def checked_species(sp, atoms_per_mol, mass=None):
    """(mol_type, vector, site) with vector None, "dipole" or (tail, head) and site "first", "com" or an atom index, all
    1-based, or a ValueError that names the species."""
    try:
        mol_type, vector, site = tuple(sp)
    except (TypeError, ValueError):
        raise ValueError("a species is (mol_type, vector, site): %r" % (sp,)) from None
    mol_type = int(mol_type)
    if not 1 <= mol_type <= len(atoms_per_mol):
        raise ValueError("species %r: mol_type must be in [1, %d]" % (sp, len(atoms_per_mol)))
    n = atoms_per_mol[mol_type - 1]
    if vector is not None and vector != "dipole":
        try:
            tail, head = (int(v) for v in vector)
        except (TypeError, ValueError):
            raise ValueError("species %r: vector must be (tail, head), 'dipole' or None" % (sp,)) from None
        if not (1 <= tail <= n and 1 <= head <= n):
            raise ValueError("species %r: tail and head must be in [1, %d], the atoms of a molecule of type %d"
                             % (sp, n, mol_type))
        if tail == head:
            raise ValueError("species %r: tail and head are the same atom" % (sp,))
        vector = (tail, head)
    if vector == "dipole" and n < 2:
        raise ValueError("species %r: a dipole needs a molecule of at least two atoms" % (sp,))
    if site == "com":
        if not mass:
            raise ValueError("species %r: the site 'com' needs mass (one entry per atom type)" % (sp,))
    elif site != "first":
        if isinstance(site, str) or int(site) != site or not 1 <= int(site) <= n:
            raise ValueError("species %r: site must be an atom index in [1, %d], 'com' or 'first'" % (sp, n))
        site = int(site)
    return mol_type, vector, site


def checked_pairs(pairs, atoms_per_mol, mass=None):
    """(species: the different ones in order of appearance, jobs [(index a, index b)]) of `pairs`."""
    pairs = list(pairs)
    if not pairs:
        raise ValueError("pairs must name at least one (species_a, species_b)")
    species, jobs = [], []
    for p in pairs:
        try:
            a, b = p
        except (TypeError, ValueError):
            raise ValueError("a pair is (species_a, species_b): %r" % (p,)) from None
        ends = []
        for sp in (a, b):
            sp = checked_species(sp, atoms_per_mol, mass)
            if sp not in species:
                species.append(sp)
            ends.append(species.index(sp))
        jobs.append(tuple(ends))
    return species, jobs


def species_terms(species, num_mols, atoms_per_mol, q=None, types=None, mass=None):
    """(site_terms, vec_terms) of the species, as backend.mol_moments takes them; q, types: per-atom columns [N] of a
    frame (charges for a dipole, atom types for a centre of mass)."""
    a0, mols, length = mol_series.type_jobs([sp[0] - 1 for sp in species], num_mols, atoms_per_mol)
    site_terms, vec_terms = [], []
    for sp, start, m, n in zip(species, a0, mols, length):
        _, vector, site = sp
        if vector is None:
            vec_terms.append([])
        elif vector == "dipole":
            row = mol_series.same_rows(q, start, m, n, "charges", species_label(sp))
            vec_terms.append([(k, float(row[k])) for k in range(1, n)])
        else:
            pair = [(vector[0] - 1, -1.0), (vector[1] - 1, 1.0)]
            vec_terms.append(sorted(t for t in pair if t[0] > 0))
        if site == "first" or site == 1:
            site_terms.append([])
        elif site == "com":
            row = T.masses(mol_series.same_rows(types, start, m, n, "atom types", species_label(sp)), mass)
            total = float(np.sum(row))
            site_terms.append([(k, float(row[k]) / total) for k in range(1, n)])
        else:
            site_terms.append([(site - 1, 1.0)])
    return site_terms, vec_terms


class PairSums:
    """The integer outputs of backend.vector_pair_hist over batches of frames, added exactly, and the volumes of the
    frames."""

    def __init__(self, n_jobs, n_bins):
        self.hist = np.zeros((n_jobs, n_bins), dtype=object)
        self.sums = np.zeros((n_jobs, 3, n_bins), dtype=object)
        self.beyond, self.unsummed, self.pairs = (np.zeros(n_jobs, dtype=object) for _ in range(3))
        self.volumes = []

    def add(self, hist, sums, beyond, unsummed, pairs, box):
        self.hist += np.asarray(hist).astype(object)
        self.sums += sums
        self.beyond += np.asarray(beyond).astype(object)
        self.unsummed += np.asarray(unsummed).astype(object)
        self.pairs += np.asarray(pairs).astype(object)
        box = np.asarray(box, dtype=np.float64)
        self.volumes.extend((box[:, 0] * box[:, 1] * box[:, 2]).tolist())

    @property
    def n_frames(self):
        return len(self.volumes)


def pair_columns(hist, sums, n_frames, n_a, n_b, same, mean_volume, bin_size):
    """The columns of one pair from its integers: hist [n_bins] and sums [3, n_bins] of Python int (fixed point, ONE =
    2^32). Every mean is ONE correctly rounded division of two integers (Python's int / int):
      <cos> = S1 / (ONE count), <P2> = 1.5 (S2 / (ONE count)) - 0.5, <cos_r> = S3 / (ONE count), NaN where count is 0;
      G_K(R) = (same ? 1 : 0) + (S1 summed over the bins up to R) / (ONE n_frames n_a);
      g(r) = count / ((n_frames n_a) rho_b shell), rho_b = n_b / mean_volume, shell = 4/3 pi bin_size^3 ((k+1)^3 - k^3):
      the normalisation of calc_atomic_rdf, with the mean of the frames' volumes since the counts are summed over them."""
    n_bins = len(hist)
    k_bin = np.arange(n_bins, dtype=np.float64)
    shell = 4.0 / 3.0 * math.pi * bin_size ** 3 * ((k_bin + 1.0) ** 3 - k_bin ** 3)
    count = np.array([float(h) for h in hist], dtype=np.float64)
    rho_b = n_b / mean_volume if n_frames else float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        g = count / ((n_frames * n_a) * rho_b * shell)

    def mean(s):
        return np.array([int(v) / (ONE * int(h)) if h else float("nan") for v, h in zip(s, hist)], dtype=np.float64)

    running, g_k = 0, []
    for v in sums[0]:
        running += int(v)
        g_k.append((1.0 if same else 0.0) + (running / (ONE * n_frames * n_a) if n_frames * n_a else float("nan")))
    return {"r": (k_bin + 0.5) * bin_size, "g(r)": g, "<cos>": mean(sums[0]), "<P2>": 1.5 * mean(sums[1]) - 0.5,
            "<cos_r>": mean(sums[2]), "G_K": np.array(g_k, dtype=np.float64)}


def calc_orientational_correlation(r_cut, bin_size, pairs, filename, num_mols, num_atoms_per_mol, mass=None,
                                   coords="wrapped", save=False, working_dir=None):
    """
    Distance-resolved orientational correlations between the molecules of `pairs` over the frames of `filename` (dump
    file or '*' pattern).
    pairs: a list of (species_a, species_b); a species is (mol_type, vector, site) — mol_type the 1-based index into
    num_mols; vector (tail, head), 1-based atoms inside the molecule (the vector points from tail to head), "dipole"
    (sum_k q_k (r_k - r_1) from the dump's `q` column, as `Reorientation`) or None: no vector, e.g. a monatomic ion; site
    where the molecule sits: a 1-based atom index, "com" (needs `mass`, one entry per atom type) or "first". Vectors are
    always unit vectors here. A pair of the same species leaves out every molecule with itself; two DIFFERENT species of
    one molecule type are two sets of entities, and their pair takes every molecule with itself too. r_cut, bin_size: the distance range and bin width, int(r_cut / bin_size) bins (at most
    4096); r_cut should not exceed half the shortest box edge: the nearest image is taken.
    num_mols / num_atoms_per_mol: molecules per type and atoms per molecule in id order. coords="wrapped" reads `x y z`
    (every named atom is wrapped once against the first atom of its molecule), coords="unwrapped" `xu yu zu` (or x y z
    ix iy iz); the sites need not lie inside the box either way. Triclinic boxes are not supported.

    Returns one DataFrame per pair, in the order of `pairs`, with the columns
      `r` (bin centres), `g(r)` of the sites (normalised as calc_atomic_rdf does, with the mean volume of the frames),
      `<cos>` = <u_a . u_b>, `<P2>` = 1.5 <(u_a . u_b)^2> - 0.5, `<cos_r>` = <u_b . r_ab / |r_ab|> (the vector of the
      SECOND species against the direction from the first to the second) over the pairs of the bin, NaN where there is
      none, and `G_K` = (a is b ? 1 : 0) + (sum of u_a . u_b over the pairs within the bin's outer edge) / (frames N_a):
      the distance-dependent Kirkwood factor. A species without a vector gives zeros in the columns that need it.
    With `save` they are written to orientational_correlation_<n>.csv (n from 0) and the pairs' labels, counts and
    pairs beyond r_cut to orientational_correlation_pairs.csv in working_dir (default: the current directory).
    A molecule whose vector vanishes has no direction, and a pair whose sites coincide no pair direction: ValueError.
    """
    if coords not in ("wrapped", "unwrapped"):
        raise ValueError('coords must be "wrapped" or "unwrapped"')
    num_mols, per = mol_series.layout(num_mols, num_atoms_per_mol)
    species, jobs = checked_pairs(pairs, per, mass)
    if not (float(bin_size) > 0.0 and float(r_cut) > 0.0):
        raise ValueError("r_cut and bin_size must be positive")
    n_bins = int(r_cut / bin_size)
    if not 1 <= n_bins <= backend.VECTOR_PAIR_MAX_BINS:
        raise ValueError("int(r_cut / bin_size) must be in [1, %d] (%d)" % (backend.VECTOR_PAIR_MAX_BINS, n_bins))
    T.refuse_triclinic(filename)
    wrapped = coords == "wrapped"
    dipole = any(sp[1] == "dipole" for sp in species)
    labels = [species_label(sp) for sp in species]
    a0, mols, length = mol_series.type_jobs([sp[0] - 1 for sp in species], num_mols, per)
    group_off = np.concatenate(([0], np.cumsum(mols))).astype(np.int64)
    unit = np.ones(len(species), dtype=np.int32)

    def missing(lacking, _names):
        what = " (a dipole needs the charges)" if lacking[0] == "q" else ""
        raise ValueError(f"Missing column '{lacking[0]}' in dump file{what}.")

    _, batches = T.attribute_batches(filename, ("q" if dipole else "id", "type"), ["x", "y", "z"] if wrapped else T.UNWRAPPED,
                                     n_atoms=int(np.dot(num_mols, per)), with_box=True, stream=STREAM,
                                     batch_bytes=BATCH_BYTES, missing=missing)
    acc = PairSums(len(jobs), n_bins)
    degenerate = np.zeros(len(species), dtype=np.uint64)
    terms = None
    for ts, first, types, xyz, box in batches:
        import torch

        if terms is None:
            terms = species_terms(species, num_mols, per, first[0] if dipole else None, types[0], mass)
        ctx = backend.default_context()
        S, B = int(group_off[-1]), len(ts)
        site, vec = (torch.empty((B, 3, S), dtype=torch.float64, device=torch.device("cuda", ctx.device)) for _ in range(2))
        got = backend.mol_moments(xyz, box if wrapped else None, a0, mols, length, terms[0], terms[1], unit,
                                  site_out=site, vec_out=vec, ctx=ctx)
        degenerate += got["degenerate"]
        acc.add(*backend.vector_pair_hist(site, vec, box, group_off, jobs, float(bin_size), n_bins, ctx=ctx), box)
    if not acc.n_frames:
        raise ValueError(f"no frames match {filename}")
    mol_series.refuse_degenerate(labels, degenerate, "zero-length vectors",
                                 "Tail and head coincide there, or the dipole vanishes")
    names = ["%s -- %s" % (labels[a], labels[b]) for a, b in jobs]
    bad = ", ".join("%s (%d)" % (n, u) for n, u in zip(names, acc.unsummed) if u)
    if bad:
        raise ValueError("pairs that could not be summed (in brackets: how many; coincident sites, or a vector that is "
                         "not finite): %s" % bad)
    mean_volume = math.fsum(acc.volumes) / acc.n_frames  # (correctly rounded sum: the order of the frames does not matter)
    frames = []
    for j, (a, b) in enumerate(jobs):
        frames.append(pd.DataFrame(pair_columns(acc.hist[j], acc.sums[j], acc.n_frames, int(mols[a]), int(mols[b]), a == b,
                                                mean_volume, float(bin_size))))
    if save and is_writer():
        where = working_dir or os.getcwd()
        for j, df in enumerate(frames):
            df.to_csv(where + "/orientational_correlation_%d.csv" % j)
        pd.DataFrame({"pair": names, "frames": acc.n_frames, "pairs": [int(v) for v in acc.pairs],
                      "beyond r_cut": [int(v) for v in acc.beyond]}).to_csv(where + "/orientational_correlation_pairs.csv")
    return frames
