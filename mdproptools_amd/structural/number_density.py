"""
Number density along the axis normal to a surface from LAMMPS dumps — drop-in for calc_number_density of the
reference's structural/number_density.py:30-139 (same signature, defaults, column names, CSV and return value), plus
calc_density_profile, the profile over a signed distance from the surface that nothing wraps into.

What runs where
  GPU (libmdhip.so, csrc/density.hip): per frame the extent of the surface atoms along the axis and the count of every
      chosen atom type per bin (number_density.py:76-105), for a batch of frames per call.
  Host (numpy, this file): parsing (the native reader; only id, type and the axis column), the atom labels, the
      normalisation by the bin volume and the mean over the frames, from the integer counts.

The reference's loop comes down to these rules, reproduced exactly:
  * the label of an atom is its type, or with num_mols and num_atoms_per_mol the per-molecule-type atom index of
    com_mols.calc_atom_type; lo, hi = min, max of the axis coordinate over the atoms labelled surface_atom;
  * dist_from_interface > 0: the atoms of each type with x - lo < dist_from_interface are binned on
    (x - lo) - (hi - lo); otherwise those with x - lo > dist_from_interface on x - lo;
  * bin k = trunc(b / bin_size), counted with Python indexing: -num_bins <= k < 0 lands in bin k + num_bins (atoms
    inside the slab wrap into the top bins), any other k outside [0, num_bins) raises IndexError;
  * a frame without surface atoms adds zeros; every frame's counts are divided by the product of the two box lengths
    across the axis times bin_size, summed in frame order and divided by the number of frames.
Unlike the reference this module needs neither np.int nor np.product (both gone from numpy), raises the IndexError
once the batch that holds the offending frame has been counted (nothing is written, as upstream), and prints
progress lines only with VERBOSE.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common.com_mols import calc_atom_type, molecule_layout
from ..common.trajectory import frame_batches, same_labels
from .rdf_cn import _save_rdf

VERBOSE = False
MAX_BATCH_BYTES = 1 << 28  # coordinates of the frames handed to the GPU in one call
AXES = ("x", "y", "z")


def _axis_index(axis):
    if axis not in AXES:
        raise KeyError(axis)  # (pandas' error upstream, for a column the frame does not have)
    return AXES.index(axis)


def _unique_rows(atom_types):
    """(unique types in order of first appearance, row of every entry of atom_types among them): a repeated type is
    counted once and its row copied."""
    uniq, row_of = [], []
    for t in atom_types:
        for u, v in enumerate(uniq):
            if v == t:
                row_of.append(u)
                break
        else:
            row_of.append(len(uniq))
            uniq.append(t)
    return uniq, np.asarray(row_of, dtype=np.int64)


def _codes(labels, surface_atom, uniq):
    """The uint16 code of every atom (backend.axis_profile_codes): its row among `uniq` (or none) and whether it is
    a surface atom. `labels` [N] or [F,N]; comparison by ==, as the reference selects."""
    labels = np.asarray(labels)
    row = np.full(labels.shape, -1, dtype=np.int64)
    for u, t in enumerate(uniq):
        row[labels == t] = u
    return backend.axis_profile_codes(row, labels == surface_atom)


def _labels(planes, num_mols, num_atoms_per_mol):
    """Atom labels of a batch, [N] when every frame carries the same ones, else [B,N]."""
    if num_mols and num_atoms_per_mol:
        lab = calc_atom_type(planes[:, 0], num_mols, num_atoms_per_mol)
    else:
        lab = planes[:, 1]
    return same_labels(lab)


def _cross_section(box, ax):
    """The product of the two box lengths across the axis, as np.prod of the two-element list gives it."""
    return np.prod([box[j] for j in range(3) if j != ax])


def calc_number_density(dump_pattern, surface_atom, atom_types, bin_size, dist_from_interface, axis_norm_interface,
                        num_mols=None, num_atoms_per_mol=None, working_dir=None, results_file="number_density.csv",
                        save_mode=True):
    """
    The number density of every entry of `atom_types` along `axis_norm_interface` ("x", "y" or "z"), measured from
    the atoms labelled `surface_atom`, averaged over the frames matching `dump_pattern` in `working_dir` (default:
    the current directory). Returns a DataFrame (r, then g_{surface_atom}-{type} per entry) and writes it to
    `results_file` in `working_dir` when `save_mode`. Arguments and quirks as in the reference (see the module text).
    """
    if not working_dir:
        working_dir = os.getcwd()
    ax = _axis_index(axis_norm_interface)
    n_bins = int(abs(dist_from_interface) / bin_size)
    if n_bins < 1:
        raise ValueError("abs(dist_from_interface) / bin_size gives no bin")
    centres = (np.arange(n_bins) + 0.5) * bin_size
    # the (surface, type) pairs behind the column names: the surface label as an integer, both rows of one dtype
    pairs = np.array([[int(surface_atom)] * len(atom_types), list(atom_types)]).T
    uniq, row_of = _unique_rows(list(atom_types))
    mode = backend.AP_REF_POS if dist_from_interface > 0 else backend.AP_REF_NEG
    total = np.zeros((len(atom_types), n_bins))
    n_frames = 0
    # batches of planes [B,3,N]: id, type and the axis coordinate
    for steps, boxes, planes in frame_batches(os.path.join(working_dir, dump_pattern),
                                              ["id", "type", axis_norm_interface], MAX_BATCH_BYTES):
        codes = _codes(_labels(planes, num_mols, num_atoms_per_mol), surface_atom, uniq)
        counts, _, outside = backend.axis_profile(np.ascontiguousarray(planes[:, 2]), codes, mode, bin_size,
                                                  dist_from_interface, n_bins, len(uniq))
        if outside.any():
            f = int(np.flatnonzero(outside)[0])
            raise IndexError("timestep %d: %d atom(s) fall outside the %d bins" % (steps[f], int(outside[f]), n_bins))
        for j, ts in enumerate(steps):
            # the reference's order of operations: counts over (area * bin_size), added frame by frame
            total += counts[j][row_of].astype(np.float64) / (_cross_section(boxes[j], ax) * bin_size)
            if VERBOSE:
                print("number_density: timestep", ts, "counted")
        n_frames += len(steps)
    return _save_rdf(centres, pairs, os.path.join(working_dir, results_file), save_mode, total / n_frames)


def calc_density_profile(filename, surface_atom, atom_types, bin_size, axis, s_min, s_max, origin="top",
                         num_mols=None, num_atoms_per_mol=None, mass=None, position="atom", per_frame=False):
    """
    The density profile of `atom_types` over the signed distance s from a surface, bins of `bin_size` over
    [s_min, s_max): s = x - origin along `axis`, origin "top" (the largest coordinate of the atoms labelled
    `surface_atom`, per frame), "bottom" (the smallest) or a fixed coordinate (a number). Nothing wraps and nothing
    raises for an atom out of range: such atoms (and NaN coordinates) are counted per frame in attrs["outside"].

    position="atom": labels as in calc_number_density (types, or per-molecule-type atom indices with num_mols and
    num_atoms_per_mol). position="com": `atom_types` names 1-based molecule types of the num_mols / num_atoms_per_mol
    layout and the binned coordinate is the molecule's mass-weighted centre of mass along the axis (`mass` per atom
    type, as calc_com takes it); `surface_atom` is then an atom type, and the surface extent still comes from atoms.

    Returns a DataFrame: s (bin centres), per entry t of atom_types rho_{t} (the mean over frames of
    count / (cross-section * bin_size), each frame with its own box) and std_{t} (the population standard deviation
    over frames); attrs: "outside" [F], "extent" [F,2] (lo, hi of the surface), "timesteps" [F], and with
    per_frame=True "counts" [F, len(atom_types), n_bins] (and "com" [F,M] in com mode).
    Periodic images are not unwrapped: a slab or a molecule that straddles the boundary along the axis is out of scope.
    """
    ax = _axis_index(axis)
    w = float(bin_size)
    n_bins = int((s_max - s_min) / w)
    if n_bins < 1:
        raise ValueError("(s_max - s_min) / bin_size gives no bin")
    if position not in ("atom", "com"):
        raise ValueError('position must be "atom" or "com"')
    if isinstance(origin, str) and origin not in ("top", "bottom"):
        raise ValueError('origin must be "top", "bottom" or a coordinate')
    uniq, row_of = _unique_rows(list(atom_types))
    com = position == "com"
    if com:
        if num_mols is None or num_atoms_per_mol is None or not mass:
            raise ValueError('position="com" needs num_mols, num_atoms_per_mol and mass')
        seg_off, mol_type, _ = molecule_layout(num_mols, num_atoms_per_mol)
        mol_codes = _codes(mol_type, None, uniq)
    counts_all, extent_all, outside_all, steps_all, box_all, com_all = [], [], [], [], [], []
    for steps, boxes, planes in frame_batches(filename, ["id", "type", axis], MAX_BATCH_BYTES,
                                              int(seg_off[-1]) if com else None):
        x = np.ascontiguousarray(planes[:, 2])
        if com:
            counts, extent, outside, sites = _com_batch(x, planes[:, 1], surface_atom, origin, mass, seg_off,
                                                        mol_codes, w, s_min, n_bins, len(uniq), per_frame)
            com_all.append(sites)
        else:
            codes = _codes(_labels(planes, num_mols, num_atoms_per_mol), surface_atom, uniq)
            counts, extent, outside = backend.axis_profile(x, codes, backend.AP_PROFILE, w, s_min, n_bins, len(uniq),
                                                           origin=_origin_arg(origin))
        counts_all.append(counts[:, row_of])
        extent_all.append(extent)
        outside_all.append(outside)
        steps_all += steps
        box_all.append(boxes)
    R = len(row_of)
    counts = np.concatenate(counts_all) if counts_all else np.zeros((0, R, n_bins), dtype=np.uint32)
    boxes = np.concatenate(box_all) if box_all else np.zeros((0, 3))
    volume = np.array([_cross_section(b, ax) * w for b in boxes])
    rho = counts.astype(np.float64) / volume[:, None, None]
    with np.errstate(invalid="ignore"):
        mean = rho.mean(axis=0) if len(rho) else np.full((R, n_bins), np.nan)
        std = rho.std(axis=0) if len(rho) else np.full((R, n_bins), np.nan)
    names = ["s"] + ["rho_%s" % (t,) for t in atom_types] + ["std_%s" % (t,) for t in atom_types]
    df = pd.DataFrame(np.vstack((s_min + (np.arange(n_bins) + 0.5) * w, mean, std)).transpose(), columns=names)
    df.attrs["outside"] = np.concatenate(outside_all).astype(np.int64) if outside_all else np.zeros(0, dtype=np.int64)
    df.attrs["extent"] = np.concatenate(extent_all) if extent_all else np.zeros((0, 2))
    df.attrs["timesteps"] = np.asarray(steps_all, dtype=np.int64)
    if per_frame:
        df.attrs["counts"] = counts
        if com:
            df.attrs["com"] = np.concatenate(com_all) if com_all else np.zeros((0, len(mol_type)))
    return df


def _origin_arg(origin):
    return {"top": "hi", "bottom": "lo"}[origin] if isinstance(origin, str) else float(origin)


def _com_batch(x, types, surface_atom, origin, mass, seg_off, mol_codes, w, s_min, n_bins, n_rows, keep_com):
    """COM mode of one batch: the atom plane goes to the device once; the surface extent from the atoms (one pass
    with nothing to bin), the centres of mass on the device (backend.segment_com) and their counts measured from the
    per-frame origin. Returns (counts, extent, outside, the centres of mass [B,M] on the host when keep_com else None)."""
    import torch

    ctx = backend.default_context()
    lab = same_labels(types)
    x = torch.from_numpy(x).to("cuda:%d" % ctx.device)
    _, extent, _ = backend.axis_profile(x, _codes(lab, surface_atom, []), backend.AP_PROFILE, w, s_min, 1, 1, ctx=ctx)
    org = {"top": extent[:, 1], "bottom": extent[:, 0]}[origin] if isinstance(origin, str) \
        else np.full(x.shape[0], float(origin))
    B, M = x.shape[0], len(seg_off) - 1
    sites = torch.empty((B, 1, M), dtype=torch.float64, device="cuda:%d" % ctx.device)
    table = np.asarray(mass, dtype=np.float64)
    if lab.ndim == 1:
        backend.segment_com(x.view(x.shape[0], 1, -1), table[lab.astype(np.int64) - 1], seg_off, out=sites, ctx=ctx)
    else:  # per-frame masses: one call per frame
        for j in range(B):
            backend.segment_com(x[j:j + 1].view(1, 1, -1), table[lab[j].astype(np.int64) - 1], seg_off, out=sites[j:j + 1],
                                ctx=ctx)
    counts, _, outside = backend.axis_profile(sites.view(B, M), mol_codes, backend.AP_PROFILE, w, s_min, n_bins, n_rows,
                                              origin=org, ctx=ctx)
    return counts, extent, outside, (sites.view(B, M).cpu().numpy() if keep_com else None)
