"""
Plain-numpy restatement of the reference's calc_number_density (structural/number_density.py:30-139) and of the
PROFILE mode next to it: the test oracle of mdproptools_amd.structural.number_density and of backend.axis_profile.
Every step in the reference's arithmetic (float64):

- label of an atom: its type, or the per-molecule-type atom index (rdf_cn.py:197-215) with num_mols / num_atoms_per_mol;
- lo, hi = min, max of the axis coordinate over the atoms labelled surface_atom (pandas' min / max: NaN skipped, NaN
  without any; here -0.0 orders below +0.0 so that the pair is unique), s = x - lo, range = hi - lo;
- d > 0: the atoms of type t with s < d, b = s - range; else those with s > d, b = s;
- k = trunc(b / w); -nb <= k < 0 counts in bin k + nb; any other k outside [0, nb) is an IndexError ("outside");
- frame counts / (prod of the two box lengths across the axis * w), summed in frame order, / number of frames;
- PROFILE: s = x - origin, t = (s - s_lo) / w, bin trunc(t) when t >= 0 and trunc(t) < nb, else outside; no wrap.

A frame is a dict: xyz [3, N] (ascending id order), types [N], bounds [3, 2], timestep (and ids).
"""

import io
import os

import numpy as np
import pandas as pd

REF_POS, REF_NEG, PROFILE = 0, 1, 2
SURFACE, NONE = 0x4000, 0x3FFF
R_LABEL = "r ($\\AA$)"


def altered_labels(ids, num_mols, num_atoms_per_mol):
    """rdf_cn.py:197-215, one id at a time."""
    cut = np.cumsum(np.multiply(num_mols, num_atoms_per_mol))
    out = []
    for v in np.asarray(ids, dtype=np.float64):
        for i, c in enumerate(cut):
            if v <= c:
                v = (v - c) % num_atoms_per_mol[i]
                if v == 0:
                    v = num_atoms_per_mol[i]
                v += sum(num_atoms_per_mol[:i])
                break
        out.append(v)
    return np.asarray(out, dtype=np.float64)


def extent(x, surf):
    """(lo, hi) of x[surf], NaN skipped; (NaN, NaN) without a value; a -0.0 wins the minimum, a +0.0 the maximum."""
    s = np.asarray(x, dtype=np.float64)[np.asarray(surf, dtype=bool)]
    s = s[~np.isnan(s)]
    if not len(s):
        return np.nan, np.nan
    lo, hi = s.min(), s.max()
    if lo == 0.0:
        lo = -0.0 if np.signbit(s[s == 0.0]).any() else 0.0
    if hi == 0.0:
        hi = 0.0 if (~np.signbit(s[s == 0.0])).any() else -0.0
    return lo, hi


def ref_bins(x, sel, lo, hi, w, d, nb):
    """(bin index after the wrap, has-a-bin mask) of the atoms `sel` selects by label, reference modes."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = x - lo
        if d > 0:
            b = s[sel & (s < d)] - (hi - lo)
        else:
            b = s[sel & (s > d)]
        q = b / w
        ok = (q < nb) & (q > -(nb + 1.0))
        k = np.trunc(q[ok]).astype(np.int64)
    return np.where(k < 0, k + nb, k), ok


def frame_counts(x, labels, surface_atom, atom_types, w, d):
    """(counts [len(atom_types), nb] int64, number of selected atoms without a bin) of one frame, reference modes."""
    nb = int(abs(d) / w)
    x = np.asarray(x, dtype=np.float64)
    lo, hi = extent(x, labels == surface_atom)
    cnt = np.zeros((len(atom_types), nb), dtype=np.int64)
    out = 0
    for i, t in enumerate(atom_types):
        k, ok = ref_bins(x, labels == t, lo, hi, w, d, nb)
        np.add.at(cnt[i], k, 1)
        out += int((~ok).sum())
    return cnt, out


def labels_of(fr, num_mols=None, num_atoms_per_mol=None):
    if num_mols and num_atoms_per_mol:
        return altered_labels(fr["ids"], num_mols, num_atoms_per_mol)
    return np.asarray(fr["types"], dtype=np.float64)


def calc_number_density(frames, surface_atom, atom_types, bin_size, dist_from_interface, axis_norm_interface,
                        num_mols=None, num_atoms_per_mol=None):
    """(DataFrame, CSV text) of calc_number_density; IndexError / KeyError where the reference raises them."""
    if axis_norm_interface not in ("x", "y", "z"):
        raise KeyError(axis_norm_interface)
    ax = "xyz".index(axis_norm_interface)
    nb = int(abs(dist_from_interface) / bin_size)
    total = np.zeros((len(atom_types), nb))
    for fr in frames:
        cnt, out = frame_counts(fr["xyz"][ax], labels_of(fr, num_mols, num_atoms_per_mol), surface_atom, atom_types,
                                bin_size, dist_from_interface)
        if out:
            raise IndexError("%d atoms outside the bins" % out)
        b = np.asarray(fr["bounds"], dtype=np.float64)
        L = b[:, 1] - b[:, 0]
        rho = cnt.astype(np.float64)
        rho = rho / (np.prod([L[j] for j in range(3) if j != ax]) * bin_size)
        total += rho
    total = total / len(frames)
    radii = (np.arange(nb) + 0.5) * bin_size
    pairs = np.array([[int(surface_atom)] * len(atom_types), list(atom_types)]).T
    cols = [R_LABEL] + ["g_%s-%s" % (p[0], p[1]) for p in pairs]
    df = pd.DataFrame(np.vstack((radii, total)).transpose(), columns=cols)
    buf = io.StringIO()
    df.to_csv(buf, index=False)
    return df, buf.getvalue()


def axis_profile(x, codes, mode, bin_size, dist, n_bins, n_rows, origin="lo"):
    """backend.axis_profile restated: x [F,N], codes [N] or [F,N] (uint16) ->
    (counts uint32 [F,n_rows,n_bins], extent [F,2], outside uint32 [F])."""
    x = np.asarray(x, dtype=np.float64)
    F, N = x.shape
    codes = np.asarray(codes).astype(np.int64)
    counts = np.zeros((F, n_rows, n_bins), dtype=np.uint32)
    ext = np.zeros((F, 2))
    outside = np.zeros(F, dtype=np.uint32)
    for f in range(F):
        c = codes if codes.ndim == 1 else codes[f]
        row = c & NONE
        lo, hi = extent(x[f], (c & SURFACE) != 0)
        ext[f] = lo, hi
        has_row = row < n_rows
        if mode == PROFILE:
            o = lo if isinstance(origin, str) and origin == "lo" else hi if isinstance(origin, str) else \
                np.broadcast_to(np.asarray(origin, dtype=np.float64), (F,))[f]
            with np.errstate(invalid="ignore", over="ignore"):
                t = ((x[f] - o) - dist) / bin_size
                ok = has_row & (t >= 0.0) & (t < n_bins)
            np.add.at(counts[f], (row[ok], np.trunc(t[ok]).astype(np.int64)), 1)
            outside[f] = int((has_row & ~ok).sum())
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                s = x[f] - lo
                sel = has_row & ((s < dist) if mode == REF_POS else (s > dist))
                b = s[sel] - (hi - lo) if mode == REF_POS else s[sel]
                q = b / bin_size
                ok = (q < n_bins) & (q > -(n_bins + 1.0))
                k = np.trunc(q[ok]).astype(np.int64)
            np.add.at(counts[f], (row[sel][ok], np.where(k < 0, k + n_bins, k)), 1)
            outside[f] = int((~ok).sum())
    return counts, ext, outside


def density_profile(x, rows_of_atoms, surf, boxes, ax, bin_size, s_min, s_max, origin, n_rows):
    """calc_density_profile restated on arrays: x [F,N], rows_of_atoms / surf [N] or [F,N] -> (s, mean [R,nb], std [R,nb],
    counts [F,R,nb], extent [F,2], outside [F]); origin "top", "bottom", a number, or values per frame [F]."""
    nb = int((s_max - s_min) / bin_size)
    codes = np.where(np.asarray(rows_of_atoms) < 0, NONE, rows_of_atoms) | np.where(surf, SURFACE, 0)
    org = {"top": "hi", "bottom": "lo"}[origin] if isinstance(origin, str) else origin
    counts, ext, outside = axis_profile(x, codes, PROFILE, bin_size, s_min, nb, n_rows, origin=org)
    vol = np.array([np.prod([b[j] for j in range(3) if j != ax]) * bin_size for b in boxes])
    rho = counts.astype(np.float64) / vol[:, None, None]
    return s_min + (np.arange(nb) + 0.5) * bin_size, rho.mean(axis=0), rho.std(axis=0), counts, ext, outside


# ---- the fixtures of tests/golden/number_density.npz (tools/make_number_density_golden.py) ----

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "number_density.npz")
N_SURF, N_LIQ = 200, 2000
# keyword arguments of calc_number_density per case; "src": which stored frame set
CASES = {
    "pos_z": dict(src="a", surface_atom=3, atom_types=[1, 2], bin_size=0.5, dist_from_interface=12.0,
                  axis_norm_interface="z"),
    "pos_x": dict(src="ax", surface_atom=3, atom_types=[1, 2], bin_size=0.173, dist_from_interface=12.0,
                  axis_norm_interface="x"),
    "boxes": dict(src="b", surface_atom=3, atom_types=[1, 2], bin_size=0.25, dist_from_interface=12.0,
                  axis_norm_interface="z"),
    "wrap": dict(src="w", surface_atom=3, atom_types=[1, 2], bin_size=0.5, dist_from_interface=12.0,
                 axis_norm_interface="z"),
    "neg_ok": dict(src="s", surface_atom=3, atom_types=[2, 1], bin_size=0.25, dist_from_interface=-12.0,
                   axis_norm_interface="z"),
    "neg_raises": dict(src="a", surface_atom=3, atom_types=[1, 2], bin_size=0.5, dist_from_interface=-12.0,
                       axis_norm_interface="z"),
    "no_surface": dict(src="a", surface_atom=9, atom_types=[1, 2], bin_size=0.5, dist_from_interface=12.0,
                       axis_norm_interface="z"),
    "lower_bound": dict(src="l", surface_atom=3, atom_types=[1, 2], bin_size=0.5, dist_from_interface=12.0,
                        axis_norm_interface="z"),
    "num_mols": dict(src="a", surface_atom=1, atom_types=[2, 3], bin_size=0.5, dist_from_interface=12.0,
                     axis_norm_interface="z", num_mols=[200, 1000], num_atoms_per_mol=[1, 2]),
    "surface_counted": dict(src="b", surface_atom=3, atom_types=[3, 1, 2], bin_size=0.25, dist_from_interface=12.0,
                            axis_norm_interface="z"),
    "repeated": dict(src="b", surface_atom=3, atom_types=[1, 1, 2], bin_size=0.25, dist_from_interface=12.0,
                     axis_norm_interface="z"),
    "absent": dict(src="b", surface_atom=3, atom_types=[2, 7], bin_size=0.25, dist_from_interface=12.0,
                   axis_norm_interface="z"),
    "bad_axis": dict(src="a", surface_atom=3, atom_types=[1], bin_size=0.5, dist_from_interface=12.0,
                     axis_norm_interface="w"),
}
RAISES = {"neg_raises": "IndexError", "bad_axis": "KeyError"}


def make_frames(seed, nf=3, lo=0.0, zmax=None, L=(20.0, 18.0, 30.0), slab=4.0):
    """Seeded frames: a slab of N_SURF type-3 atoms in z = lo + 1 .. lo + 1 + slab, N_LIQ atoms of types 1 and 2
    above it, coordinates with 4 decimals."""
    rng = np.random.default_rng(seed)
    n = N_SURF + N_LIQ
    out = []
    for f in range(nf):
        xyz = np.empty((3, n))
        xyz[0] = rng.uniform(0, L[0], n)
        xyz[1] = rng.uniform(0, L[1], n)
        xyz[2, :N_SURF] = rng.uniform(lo + 1.0, lo + 1.0 + slab, N_SURF)
        xyz[2, N_SURF:] = rng.uniform(lo + 1.0 + slab, zmax or (lo + L[2]), N_LIQ)
        types = np.r_[np.full(N_SURF, 3), rng.integers(1, 3, N_LIQ)].astype(np.int64)
        out.append(dict(ids=np.arange(1, n + 1), types=types, xyz=np.round(xyz, 4), timestep=100 * f,
                        bounds=np.array([[0, L[0]], [0, L[1]], [lo, lo + L[2]]], dtype=np.float64)))
    return out


def frame_sets():
    """The frame sets of the golden, by key (see CASES)."""
    sets = {"a": make_frames(1), "s": make_frames(4, zmax=12.0), "l": make_frames(7, lo=-15.0)}
    ax = make_frames(2, nf=4)
    for fr in ax:  # the slab normal to x
        fr["xyz"] = fr["xyz"][[2, 0, 1]]
        fr["bounds"] = fr["bounds"][[2, 0, 1]]
    sets["ax"] = ax
    b = make_frames(8, nf=4)
    for i, fr in enumerate(b):  # box lengths that differ from frame to frame
        fr["bounds"] = fr["bounds"] + np.array([[0, 0.37 * i], [0, 0.11 * i], [0, 0.5 * i]])
        fr["xyz"][2, 300:310] = 3.0
    sets["b"] = b
    w = make_frames(3)
    for fr in w:
        fr["xyz"][2, 300:320] = 2.01  # inside the slab: negative bins, wrapped into the top ones
        fr["xyz"][2, 320] = np.round(fr["xyz"][2, :N_SURF].max() - 0.3, 4)  # b in (-bin_size, 0): bin 0
    sets["w"] = w
    return sets


def load():
    return dict(np.load(GOLDEN, allow_pickle=False))


def frames_of(z, src):
    n = z[src + "_xyz"].shape[2]
    return [dict(ids=np.arange(1, n + 1), types=z[src + "_type"][f].astype(np.int64), xyz=z[src + "_xyz"][f],
                 bounds=z[src + "_bounds"][f], timestep=int(z[src + "_timestep"][f]))
            for f in range(len(z[src + "_xyz"]))]


def case_args(z, key):
    kw = dict(CASES[key])
    return frames_of(z, kw.pop("src")), kw


def write_dumps(frames, directory):
    """The frames as LAMMPS dumps (repr round trip: the same doubles parse back); returns the file pattern."""
    from mdproptools_amd.io import write_dump

    for fr in frames:
        tab = np.column_stack([fr["ids"], fr["types"], np.asarray(fr["xyz"]).T])
        write_dump(os.path.join(directory, "dump.%d.dump" % fr["timestep"]), fr["timestep"], fr["bounds"],
                   ["id", "type", "x", "y", "z"], tab)
    return "dump.*.dump"
