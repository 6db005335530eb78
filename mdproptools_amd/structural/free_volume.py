"""
Free volume and cavity sizes from LAMMPS dumps — polymer and glyme electrolytes, ionic liquids, concentrated salts: the
fractional free volume as a function of probe radius, the distribution of cavity sizes and which species line the
cavities. The reference has no such module; include/mdhip.h (mdhip_free_volume) holds the specification of the device
part and tests/free_volume_ref.py restates it in numpy. Arguments follow `calc_molecular_shape`.

Atoms are hard spheres of the radius of their type. A regular grid of probe points is laid over the periodic cell; for
every point, s is the distance to the nearest sphere SURFACE: negative inside an atom, else the radius of the largest
probe sphere centred there that touches no atom — the local cavity size. A point is free for a probe of radius r when
s >= r.

What runs where
  GPU (libmdhip.so, csrc/free_volume.hip): per frame a cell grid over the atoms, per grid point the minimum of s over
      the atoms of the neighbouring cells and the atom that attains it; exact integer histograms of s by the class of
      that atom, the free points per frame and probe, the per-point occupancy map.
  Host: parsing (common/trajectory.py: the frames are never all resident), radii and classes, adding the batches'
      integers, putting the frames in time order, the tables and the files.

The grid is fractional: g_a = ceil(L_a / grid_spacing) points along axis a of the FIRST frame, the same count in every
frame, at ((i + 0.5) / g_a) * L_a. It is anchored at coordinate 0 of the wrapped cell: the dump's lower bounds are not
carried, only the lattice of images matters, and a rigid shift of the grid changes no statistic. The cube file of
`map_file` therefore has its origin at the cell's lower corner taken as 0.
"""

import math
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import trajectory as T
from ..dist import is_writer
from .spatial_distribution import write_cube

MAX_BINS = backend.FREE_VOLUME_MAX_BINS
MAX_CLASSES = backend.FREE_VOLUME_MAX_CLASSES
MAX_PROBES = backend.FREE_VOLUME_MAX_PROBES
MAX_POINTS = backend.FREE_VOLUME_MAX_POINTS
MAX_FIELD_FRAMES = 8       # frames of a call with return_field: s and nearest are 12 bytes per point and frame
DEFAULT_S_MAX = 4.0        # A: the largest cavity radius that gets a bin unless the box is too small for it
TABLES = ("summary", "distribution", "frames")


def classes_of(types_row, radii, exclude_types=None, type_names=None):
    """(atom_class int32 [N], radius [C], names [C]) from a frame's atom-type column and the `radii` map {type: radius}:
    the classes are the types of `radii` that occur and are not excluded, ascending; an atom of an excluded type has the
    class -1. A type that occurs, has no radius and is not excluded is a ValueError that names it."""
    types_row = np.asarray(types_row)
    excluded = set(int(t) for t in (exclude_types or ()))
    try:
        given = {int(t): float(r) for t, r in dict(radii).items()}
    except (TypeError, ValueError):
        raise ValueError("radii must map every atom type to a radius in Angstrom") from None
    present = sorted(set(int(t) for t in np.unique(types_row)))
    lacking = [t for t in present if t not in given and t not in excluded]
    if lacking:
        raise ValueError("radii has no radius for atom type %d (give one, or name the type in exclude_types)" % lacking[0])
    kept = [t for t in present if t not in excluded]
    if len(kept) > MAX_CLASSES:
        raise ValueError("%d atom types; at most %d: exclude some" % (len(kept), MAX_CLASSES))
    for t in kept:
        if not (given[t] >= 0 and math.isfinite(given[t])):
            raise ValueError("radii: the radius of atom type %d must be finite and not negative" % t)
    cls = np.full(len(types_row), -1, dtype=np.int32)
    for k, t in enumerate(kept):
        cls[types_row == t] = k
    names = [str((type_names or {}).get(t, "type%d" % t)) for t in kept]
    if len(set(names)) != len(names):
        raise ValueError("type_names must give different names")
    return cls, np.array([given[t] for t in kept], dtype=np.float64), names


def grid_of(L, grid_spacing):
    """g_a = ceil(L_a / grid_spacing) of the first frame's edges."""
    h = float(grid_spacing)
    if not (h > 0 and math.isfinite(h)):
        raise ValueError("grid_spacing must be positive and finite")
    g = tuple(max(1, int(math.ceil(float(v) / h - 1e-9))) for v in L)
    if g[0] * g[1] * g[2] > MAX_POINTS:
        raise ValueError("the grid %s holds more than 2^27 points: take a larger grid_spacing" % (g,))
    return g


def default_s_max(L, r_max_atom, bin_size):
    """min(DEFAULT_S_MAX, min(L) / 2 - the largest radius), cut down to whole bins (at least one): the search radius
    s_max + the largest radius then stays within half the shortest edge of the first frame."""
    s = min(DEFAULT_S_MAX, 0.5 * float(min(L)) - float(r_max_atom))
    return max(math.floor(s / float(bin_size) + 1e-9), 1) * float(bin_size)


def bins_of(s_max, bin_size, L, r_max_atom):
    """(edges [nbins+1] = k * bin_size, r_search = edges[-1] + the largest radius); r_search must stay below the
    shortest edge of the first frame."""
    bin_size, s_max = float(bin_size), float(s_max)
    if not (bin_size > 0 and math.isfinite(bin_size) and s_max > 0 and math.isfinite(s_max)):
        raise ValueError("bin_size and s_max must be positive and finite")
    n = int(math.ceil(s_max / bin_size - 1e-9))
    if not 1 <= n <= MAX_BINS:
        raise ValueError("s_max / bin_size = %d bins; at most %d: take a larger bin_size" % (n, MAX_BINS))
    edges = np.arange(n + 1, dtype=np.float64) * bin_size
    r_search = float(edges[-1]) + float(r_max_atom)
    if not r_search < float(min(L)):
        raise ValueError("s_max + the largest radius = %g A reaches the shortest box edge %g A: take a smaller s_max"
                         % (r_search, float(min(L))))
    return edges, r_search


def probes_of(probe_radii, top):
    p = np.atleast_1d(np.asarray(probe_radii, dtype=np.float64)).ravel()
    if not 1 <= len(p) <= MAX_PROBES:
        raise ValueError("probe_radii must hold 1 to %d radii" % MAX_PROBES)
    if not (np.all(np.isfinite(p)) and np.all(p >= 0) and np.all(p <= top)):
        raise ValueError("probe_radii must be finite and lie in [0, s_max = %g]" % top)
    return p


def tables(names, probe, edges, G, steps, volume, n_free, hist, beyond):
    """The three DataFrames of calc_free_volume from the added integers: n_free int64 [F,P], hist [C,nbins], beyond (a
    number); steps [F] and volume [F] (A^3) in time order like n_free."""
    probe, edges = np.asarray(probe, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    hist = np.asarray(hist).astype(np.int64)
    n_free, volume = np.asarray(n_free, dtype=np.int64), np.asarray(volume, dtype=np.float64)
    F = len(steps)
    ffv = n_free / float(G)
    summary = pd.DataFrame({
        "probe_radius (A)": probe, "FFV": ffv.mean(axis=0), "FFV_std": ffv.std(axis=0),
        "free_volume (A^3)": (ffv * volume[:, None]).mean(axis=0), "box_volume (A^3)": np.full(len(probe), volume.mean())})
    width = np.diff(edges)
    total = int(hist.sum()) + int(beyond)            # the free points: s >= 0, or no atom within reach
    points = F * int(G)
    per_bin = hist.sum(axis=0)
    at_least = int(beyond) + np.cumsum(per_bin[::-1])[::-1]      # the points with s >= the bin's lower edge
    dist = {"s (A)": 0.5 * (edges[:-1] + edges[1:]), "s_lo (A)": edges[:-1],
            "p_total": per_bin / (total * width) if total else np.full(len(width), np.nan)}
    for c, name in enumerate(names):
        dist["p_" + name] = hist[c] / (total * width) if total else np.full(len(width), np.nan)
    dist["accessible_fraction"] = at_least / float(points)
    frames = {"timestep": np.asarray(steps, dtype=np.int64), "volume (A^3)": volume}
    for k, r in enumerate(probe):
        frames["FFV_%g" % r] = ffv[:, k]
    return {"summary": summary, "distribution": pd.DataFrame(dist), "frames": pd.DataFrame(frames)}


def calc_free_volume(filename, radii, num_mols=None, num_atoms_per_mol=None, grid_spacing=0.5, probe_radii=(0.0,),
                     bin_size=0.05, s_max=None, exclude_types=None, type_names=None, map_file=None, return_field=False,
                     working_dir=None, save=False, **how):
    """
    Free volume and cavity sizes of the frames of `filename` (dump file or '*' pattern; wrapped coordinates x y z).
    radii: {atom type: radius in A} (common.constants.BONDI_RADII helps to build it), required for every type that is
    not in exclude_types; atoms of excluded types are ignored — leave the mobile ion out to get the volume it sees.
    num_mols / num_atoms_per_mol: when both are given, every frame must hold that many atoms. grid_spacing (A): the grid
    has g_a = ceil(L_a / grid_spacing) points along axis a of the first frame. probe_radii: 1 to 8 probe radii in
    [0, s_max]. bin_size (A) and s_max (A) set the bins of s; s_max defaults to `default_s_max`: min(4 A, half the shortest
    edge of the first frame - the largest radius) cut down to whole bins, so that the search radius s_max + the largest
    radius stays within half that edge; a given s_max must keep it below the shortest edge. type_names: {type: name} for
    the columns (default type<t>). `how`: stream, batch_bytes of trajectory.attribute_batches. Triclinic boxes are not
    supported.

    Returns a dict of DataFrames:
      "summary": one row per probe radius: `probe_radius (A)`, `FFV` and `FFV_std` (mean and standard deviation over
        the frames of n_free / G), `free_volume (A^3)` (the mean of FFV * V) and `box_volume (A^3)` (the mean of V);
      "distribution": per bin `s (A)` (mid-point), `s_lo (A)`, `p_total` and per lining class `p_<name>`: counts /
        (free points * bin width), the free points being those with s >= 0 in all frames, so that p_total integrates to the
        share of them below s_max and the p_<name> add up to it; `accessible_fraction` = P(s' >= s_lo) over ALL points:
        the fractional free volume against probe radius at bin resolution;
      "frames": `timestep`, `volume (A^3)` and `FFV_<r>` per probe radius, in time order.
    With `save` they are written to free_volume_<table>.csv in working_dir (default: the current directory). map_file:
    the share of the frames in which a point is free for probe_radii[0], as a Gaussian cube file. return_field (at most
    MAX_FIELD_FRAMES frames): also "s" float64 and "nearest" int32 (atom index in id order, -1: none), [F,gx,gy,gz] in
    time order.
    """
    T.refuse_triclinic(filename)
    n_atoms = None
    if num_mols is not None and num_atoms_per_mol is not None:
        n_atoms = int(np.dot(np.asarray(num_mols, dtype=np.int64), np.asarray(num_atoms_per_mol, dtype=np.int64)))
    _, batches = T.attribute_batches(filename, ("id", "type"), ["x", "y", "z"], n_atoms=n_atoms, with_box=True, **how)
    setup = None
    steps, volume, n_free, fields, edges_seen = [], [], [], [], []
    hist = fmap = None
    beyond = 0
    for ts, _ids, atom_types, xyz, box in batches:
        box = np.asarray(box, dtype=np.float64)
        types_now = np.asarray(atom_types).astype(np.int64)
        if setup is None:
            cls, radius, names = classes_of(types_now[0], radii, exclude_types, type_names)
            if not len(radius):
                raise ValueError("every atom type is excluded")
            g = grid_of(box[0], grid_spacing)
            r_big = float(radius.max())
            top = default_s_max(box[0], r_big, bin_size) if s_max is None else s_max
            edges, r_search = bins_of(top, bin_size, box[0], r_big)
            probe = probes_of(probe_radii, float(edges[-1]))
            setup = types_now[0].copy()
            hist = np.zeros((len(radius), len(edges) - 1), dtype=np.uint64)
            fmap = np.zeros(g, dtype=np.uint64) if map_file else None
        if not np.array_equal(types_now, np.broadcast_to(setup, types_now.shape)):
            raise ValueError("the atom types change between frames")
        if return_field and len(steps) + len(ts) > MAX_FIELD_FRAMES:
            raise ValueError("return_field is for at most %d frames" % MAX_FIELD_FRAMES)
        got = backend.free_volume(xyz, box, cls, radius, g, r_search, edges, probe, want_map=bool(map_file),
                                  field=bool(return_field))
        np.add(hist, got["hist"], out=hist)
        beyond += got["beyond"]
        n_free.append(got["n_free"])
        if fmap is not None:
            np.add(fmap, got["free_map"], out=fmap)
        if return_field:
            fields.append((np.array(got["s"]), np.array(got["nearest"])))
        steps.extend(np.asarray(ts).tolist())
        edges_seen.append(box.copy())
        volume.extend((box[:, 0] * box[:, 1] * box[:, 2]).tolist())
    if not steps:
        raise ValueError(f"no frames match {filename}")
    order = np.argsort(np.asarray(steps, dtype=np.int64), kind="stable")
    G = g[0] * g[1] * g[2]
    out = tables(names, probe, edges, G, np.asarray(steps, dtype=np.int64)[order], np.asarray(volume)[order],
                 np.concatenate(n_free, axis=0)[order], hist, beyond)
    where = working_dir or os.getcwd()
    if save and is_writer():
        for name in TABLES:
            out[name].to_csv(os.path.join(where, "free_volume_%s.csv" % name))
    if map_file:
        out["free_map"] = fmap / float(len(steps))
        if is_writer():  # the voxel of the cube file: the mean edges over the frames, divided by the grid
            path = map_file if os.path.isabs(str(map_file)) else os.path.join(where, str(map_file))
            write_cube(path, out["free_map"], None, None, "free-volume occupancy, probe radius %g A" % probe[0],
                       voxel=np.mean(np.concatenate(edges_seen, axis=0), axis=0) / np.asarray(g, dtype=np.float64),
                       comment="cell axes x y z from the lower corner; outer loop x, inner loop z")
    if return_field:
        out["s"] = np.concatenate([f[0] for f in fields], axis=0)[order]
        out["nearest"] = np.concatenate([f[1] for f in fields], axis=0)[order]
    return out
