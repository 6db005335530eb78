"""
Spatial distribution functions from LAMMPS dumps: where around a reference molecule its neighbours sit — the
three-dimensional histogram of observed atoms in the molecule's body-fixed frame, normalised by the bulk density and
viewed as an isosurface (on top of a ring or in its plane, at which oxygen of an anion). The reference has no such
function; DESIGN.md (spatial distribution) holds the specification, and tests/sdf_ref.py restates it in numpy.

What runs where
  GPU (libmdhip.so, csrc/sdf.hip): per frame and reference molecule the body frame, the shell search, every hit's
      projection and the exact integer grid.
  Host (numpy, this file): parsing (the native reader), the atom types and the molecule layout, the sum over the
      batches, the normalisation, the DataFrame and the files.

The body frame of a molecule with origin atom o, x-axis atom p and xy-plane atom q: e1 along o -> p, e2 the part of
o -> q orthogonal to e1, e3 = e1 x e2 (right-handed); all three under the single wrap of the RDF functions. An observed
atom within r_cut of o (the single-wrap rsq, strict) falls in the cell floor((d . e_k + r_cut) / bin_size) per axis. A
molecule whose frame does not exist in some frame (p on o, q on the line o-p) is a degenerate row: its hits are
counted in `n_degenerate`, not in the grid.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import atom_molecules, molecule_layout
from ..common.constants import BOHR_RADIUS
from ..common.trajectory import refuse_triclinic, typed_batches
from ..dist import is_writer

_ANGSTROM_PER_BOHR = BOHR_RADIUS * 1e10


def _reference_atoms(reference, num_mols, num_atoms_per_mol):
    """(origin, x_atom, xy_atom) [M] each, 0-based atom indices in id order, of every molecule of the reference type."""
    try:
        ref = tuple(int(v) for v in reference)
    except TypeError:
        ref = ()
    if len(ref) != 4:
        raise ValueError("reference must be (mol_type, origin, x_atom, xy_atom), all 1-based")
    mt, atoms = ref[0], ref[1:]
    if not 1 <= mt <= len(num_mols):
        raise ValueError("reference molecule type %d: the layout has %d molecule types" % (mt, len(num_mols)))
    n_at = int(num_atoms_per_mol[mt - 1])
    for a in atoms:
        if not 1 <= a <= n_at:
            raise ValueError("reference atom %d: molecule type %d has %d atoms" % (a, mt, n_at))
    if len(set(atoms)) != 3:
        raise ValueError("the origin, x-axis and xy-plane atoms of reference must be three distinct atoms")
    seg_off, mol_type, _ = molecule_layout(num_mols, num_atoms_per_mol)
    first = seg_off[:-1][mol_type == mt]
    return tuple((first + a - 1).astype(np.int32) for a in atoms)


def write_cube(path, grid, r_cut, bin_size, title, voxel=None, comment=None):
    """`grid` [G,G,G] (body-frame axes e1, e2, e3) as a Gaussian cube file: lengths in Bohr, the first voxel centred at
    -r_cut + bin_size / 2 on every axis, one dummy atom at the origin of the body frame.
    With `voxel` = (vx, vy, vz) in Angstrom instead (r_cut and bin_size are then not read): a grid [Gx,Gy,Gz] over a
    cell whose lower corner is the origin, voxel (i, j, k) centred at ((i + 1/2) vx, (j + 1/2) vy, (k + 1/2) vz);
    `comment` replaces the second line."""
    shape = tuple(grid.shape)
    if voxel is None:
        o = (-float(r_cut) + 0.5 * float(bin_size)) / _ANGSTROM_PER_BOHR
        origin, v = (o, o, o), (float(bin_size) / _ANGSTROM_PER_BOHR,) * 3
    else:
        v = tuple(float(x) / _ANGSTROM_PER_BOHR for x in voxel)
        origin = tuple(0.5 * x for x in v)
    with open(path, "w") as fh:
        fh.write("%s\n" % title)
        fh.write("%s\n" % (comment or "body-frame axes e1 e2 e3; outer loop e1, inner loop e3"))
        fh.write("%5d %12.6f %12.6f %12.6f\n" % ((1,) + origin))
        for k in range(3):
            fh.write("%5d %12.6f %12.6f %12.6f\n" % ((shape[k],) + tuple(v[k] if j == k else 0.0 for j in range(3))))
        fh.write("%5d %12.6f %12.6f %12.6f %12.6f\n" % (0, 0.0, 0.0, 0.0, 0.0))
        flat = np.nan_to_num(np.asarray(grid, dtype=np.float64)).reshape(shape[0] * shape[1], shape[2])
        for row in flat:  # (a new line after every run along e3, six values to a line)
            for i in range(0, shape[2], 6):
                fh.write(" ".join("%13.5E" % x for x in row[i:i + 6]) + "\n")


def calc_spatial_distribution(r_cut, bin_size, reference, observed, filename, num_mols, num_atoms_per_mol,
                              exclude_same_molecule=True, path_or_buff="sdf.npz", cube=False, save_mode=True,
                              compute=None):
    """
    Spatial distribution functions of the `observed` atom types (the altered types of calc_atomic_rdf: the index of an
    atom inside its molecule type) around the molecules of `reference` = (mol_type, origin, x_atom, xy_atom) — the
    molecule type and three distinct atoms of it, all 1-based like Reorientation's vectors — over the frames of
    `filename` (dump file or '*' pattern). r_cut: the radius around the origin atom; bin_size: the cell edge; both in
    the dump's length unit. exclude_same_molecule leaves out atoms of the reference molecule itself. `compute`: a
    callable with the signature of backend.sdf_hist to use in its place.

    Returns (sdf, counts, axes, summary):
      sdf float64 [S,G,G,G]: g_s = count_s / (n_valid_rows * bin_size**3 * rho_s), rho_s = N_s * mean over the frames
        of 1 / V; n_valid_rows = frames x molecules - degenerate rows; NaN without valid rows;
      counts int64 [S,G,G,G]; axes float64 [G]: the cell centres -r_cut + (i + 0.5) * bin_size of every axis;
      summary: one row per species: species, n_hits, n_degenerate, max_g and hits_per_centre_frame.
    With save_mode the arrays go to `path_or_buff` (.npz: sdf, counts, axes, species, n_degenerate, n_valid_rows); with
    `cube` also one Gaussian cube file per species beside it (<stem>_<type>.cube).
    """
    origin, x_atom, xy_atom = _reference_atoms(reference, num_mols, num_atoms_per_mol)
    species = [int(v) for v in observed]
    if not species or len(set(species)) != len(species):
        raise ValueError("observed must be a non-empty list of distinct atom types")
    S = len(species)
    if S > backend.SDF_MAX_SPECIES:
        raise ValueError("at most %d observed species per call (%d given)" % (backend.SDF_MAX_SPECIES, S))
    G = backend.sdf_grid(r_cut, bin_size)
    if G > backend.SDF_MAX_GRID or S * G ** 3 > backend.SDF_MAX_CELLS:
        raise ValueError("%d species x %d**3 cells: at most %d cells per axis and %d cells per call (larger bin_size, "
                         "or fewer species)" % (S, G, backend.SDF_MAX_GRID, backend.SDF_MAX_CELLS))
    mol_of = atom_molecules(num_mols, num_atoms_per_mol)[1] if exclude_same_molecule else None
    refuse_triclinic(filename)
    compute = compute or backend.sdf_hist

    hist = np.zeros((S, G, G, G), dtype=np.uint64)
    degen = np.zeros(S, dtype=np.uint64)
    cand = cand_class = None
    n_frames, bad_rows, inv_vol = 0, 0, 0.0
    for steps, boxes, xyz, types in typed_batches(filename, num_mols, num_atoms_per_mol, True):
        if cand is None:
            cand = np.flatnonzero(np.isin(types, species)).astype(np.int32)
            slot = {ty: s for s, ty in enumerate(species)}
            cand_class = np.array([slot[ty] for ty in types[cand]], dtype=np.int32)
        h, d, _, bad = compute(xyz, boxes, origin, x_atom, xy_atom, cand, cand_class, S, r_cut, bin_size, mol_of=mol_of)
        hist += np.asarray(h).astype(np.uint64, copy=False)  # (a `compute` may hand back signed counts)
        degen += np.asarray(d).astype(np.uint64, copy=False)
        bad_rows += int(bad)
        n_frames += len(steps)
        inv_vol += float((1.0 / np.prod(boxes, axis=1)).sum())

    counts = hist.astype(np.int64)
    n_valid = n_frames * len(origin) - bad_rows
    axes = -float(r_cut) + (np.arange(G) + 0.5) * float(bin_size)
    sdf = np.full((S, G, G, G), np.nan)
    rows = []
    for s, ty in enumerate(species):
        n_s = int((cand_class == s).sum()) if cand_class is not None else 0
        rho = n_s * inv_vol / n_frames if n_frames else 0.0
        if n_valid > 0 and rho > 0.0:
            sdf[s] = counts[s] / (n_valid * float(bin_size) ** 3 * rho)
        total = int(counts[s].sum())
        rows.append((ty, total + int(degen[s]), int(degen[s]), float(np.nanmax(sdf[s])) if n_valid > 0 and rho > 0.0
                     else np.nan, total / n_valid if n_valid > 0 else np.nan))
    summary = pd.DataFrame(rows, columns=["species", "n_hits", "n_degenerate", "max_g", "hits_per_centre_frame"])
    if save_mode and is_writer():
        np.savez(path_or_buff, sdf=sdf, counts=counts, axes=axes, species=np.array(species), n_degenerate=degen,
                 n_valid_rows=np.int64(n_valid))
        if cube:
            stem = os.path.splitext(str(path_or_buff))[0]
            for s, ty in enumerate(species):
                write_cube("%s_%d.cube" % (stem, ty), sdf[s], r_cut, bin_size,
                           "spatial distribution function of atom type %d" % ty)
    return sdf, counts, axes, summary
