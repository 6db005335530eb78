"""
Bond-angle distributions from LAMMPS dumps: the distribution of the angle A-C-B at a centre atom C between two of its
shell neighbours (O-Mg-O for octahedral against tetrahedral coordination, O-O-O for the tetrahedrality of water, anion
bite angles). The reference has no such function; DESIGN.md (angular distribution) holds the specification, and
tests/angular_ref.py restates it in numpy.

What runs where
  GPU (libmdhip.so, csrc/angles.hip): per frame and centre the shell search, every pair of shell neighbours, its cosine
      and exact integer histograms per triplet.
  Host (numpy, this file): parsing (the native reader), the atom types and the molecule layout, the cosine table of
      the bin edges, the normalisation and the DataFrames.

One triplet (a, c, b) with cutoffs (r_ca, r_cb): the neighbours of a centre of type c in role A are the atoms of type a
at rsq < r_ca**2 (the single-wrap rsq of the RDF functions, strict), in role B those of type b at rsq < r_cb**2; with
a == b and r_ca == r_cb every unordered pair of neighbours is counted once, else every ordered pair (j in role A, k in
role B, j != k). The angle theta of a pair falls in bin m when m * bin_size <= theta < (m + 1) * bin_size, decided on the
cosine against cos(m * bin_size) without an arccos; the last bin is closed at 180 degrees. A pair with a neighbour ON
the centre has no angle: it is counted in `n_degenerate`.
"""

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import atom_molecules
from ..common.tables import density, write_csv
from ..common.trajectory import refuse_triclinic, typed_batches
from ..dist import is_writer


def _cutoffs(r_cut, n_triplets):
    """[T, 2] (r_ca, r_cb) from a scalar, or from one scalar or pair per triplet."""
    if np.ndim(r_cut) == 0:
        return np.full((n_triplets, 2), float(r_cut))
    if len(r_cut) != n_triplets:
        raise ValueError("r_cut must be a scalar or hold one (r_ca, r_cb) per triplet: %d given for %d triplets"
                         % (len(r_cut), n_triplets))
    out = np.empty((n_triplets, 2))
    for t, rc in enumerate(r_cut):
        out[t] = (rc, rc) if np.ndim(rc) == 0 else tuple(rc)
    return out


def calc_angular_distribution(r_cut, bin_size, triplets, filename, num_mols=None, num_atoms_per_mol=None,
                              exclude_same_molecule=False, path_or_buff="adf.csv", save_mode=True):
    """
    Angular distribution functions of the `triplets` [(a, c, b), ...] (atom types; with num_mols and num_atoms_per_mol
    the altered types of calc_atomic_rdf: the index of an atom inside its molecule type) over the frames of `filename`
    (dump file or '*' pattern). r_cut: one (r_ca, r_cb) per triplet, or a scalar for all; bin_size in degrees;
    exclude_same_molecule leaves out neighbours of the centre's own molecule (needs the layout).

    Returns (adf, summary):
      adf: `angle` (bin centres, degrees) and per triplet `adf_a-c-b` = count / (count.sum() * bin_size) (integrates to
        1 over degrees; NaN for a triplet without counts) and `count_a-c-b` (int64); written to `path_or_buff`;
      summary: one row per triplet: triplet, n_angles, n_degenerate, mean_angle (degrees, over bin centres) and
        angles_per_centre_frame.
    """
    trip = [tuple(int(v) for v in t) for t in triplets]
    if not trip or any(len(t) != 3 for t in trip):
        raise ValueError("triplets must be a non-empty list of (a, c, b) atom types")
    T = len(trip)
    if T > backend.ANGLE_MAX_TRIPLETS:
        raise ValueError("at most %d triplets per call (%d given)" % (backend.ANGLE_MAX_TRIPLETS, T))
    rc = _cutoffs(r_cut, T)
    layout = num_mols is not None and num_atoms_per_mol is not None
    altered = bool(num_mols and num_atoms_per_mol)
    if exclude_same_molecule and not layout:
        raise ValueError("exclude_same_molecule needs num_mols and num_atoms_per_mol (the molecule layout in id order)")
    edges = backend.angle_cos_edges(bin_size)
    n_bins = len(edges)
    if T * n_bins > backend.ANGLE_MAX_CELLS:
        raise ValueError("%d triplets x %d bins: at most %d histogram cells per call (larger bin_size, or fewer "
                         "triplets)" % (T, n_bins, backend.ANGLE_MAX_CELLS))
    mol_of = atom_molecules(num_mols, num_atoms_per_mol)[1] if layout else None  # (a bad layout raises here)
    refuse_triclinic(filename)

    hist = np.zeros((T, n_bins), dtype=np.uint64)
    degen = np.zeros(T, dtype=np.uint64)
    types, n_frames = None, 0
    for steps, boxes, xyz, types in typed_batches(filename, num_mols, num_atoms_per_mol, altered):
        h, d, _, _ = backend.angle_hist(xyz, boxes, types, trip, rc ** 2, edges,
                                        mol_of=mol_of if exclude_same_molecule else None)
        hist += h
        degen += d
        n_frames += len(steps)

    centres = (np.arange(n_bins) + 0.5) * float(bin_size)
    adf = pd.DataFrame({"angle": centres})
    rows = []
    for t, (a, c, b) in enumerate(trip):
        name = "%d-%d-%d" % (a, c, b)
        cnt = hist[t].astype(np.int64)
        total = int(cnt.sum())
        adf["adf_" + name] = density(cnt, float(bin_size))
        adf["count_" + name] = cnt
        n_cen = int((types == c).sum()) if types is not None else 0
        rows.append((name, total, int(degen[t]), float((cnt * centres).sum() / total) if total else np.nan,
                     total / (n_cen * n_frames) if n_cen * n_frames else np.nan))
    summary = pd.DataFrame(rows, columns=["triplet", "n_angles", "n_degenerate", "mean_angle",
                                          "angles_per_centre_frame"])
    if save_mode and is_writer():
        write_csv(adf, path_or_buff)
    return adf, summary
