"""
Plain-numpy restatement of the bond-angle histograms (angular distribution): the test oracle of
backend.angle_hist and structural/angular_distribution.py. Every step in the specified arithmetic, unfused doubles:

- rsq(c, j): per axis a = |x_c - x_j|, min(a, |a - L|) (the |d| form of the single wrap), (ax*ax + ay*ay) + az*az;
  neighbour of c in role A: j != c, type[j] == type_a, rsq < r_ca**2 (strict), another molecule under exclusion;
- d_j = x_j - x_c, signed wrap d > L/2 ? d - L : (d < -L/2 ? d + L : d); n_j = sqrt((dx*dx + dy*dy) + dz*dz);
- cos = ((dxj*dxk + dyj*dyk) + dzj*dzk) / (n_j * n_k);
- bin = the number of m in [1, n_bins) with cos <= E[m], E[m] = cos(radians(m * bin_size)); NaN in no bin;
- a symmetric triplet (type_a == type_b, r_ca == r_cb) counts the unordered pairs of role-A neighbours, an asymmetric
  one the ordered pairs (j in role A, k in role B, j != k).

`angle_hist` is vectorised over the frames (one centre at a time); `brute_hist` is the same definition as nested
Python loops over one frame, for small cross-checks.
"""

import math
import os

import numpy as np


def cos_edges(bin_size):
    n_bins = int(np.ceil(180.0 / bin_size))
    return np.cos(np.radians(np.arange(n_bins) * bin_size))


def bin_of(cos, edges):
    """The number of m in [1, n_bins) with cos <= edges[m] (edges strictly decreasing); cos must not be NaN."""
    return np.searchsorted(-edges[1:], -np.asarray(cos), side="right")


def arccos_bin(cos, bin_size, n_bins):
    """The binning rule the table replaces: min(int(degrees(arccos(clip(cos))) / bin_size), n_bins - 1)."""
    theta = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
    return np.minimum((theta / bin_size).astype(np.int64), n_bins - 1)


def _wrap_abs(d, L):
    a = np.abs(d)
    return np.minimum(a, np.abs(a - L))


def _wrap(d, L):
    h = 0.5 * L
    return np.where(d > h, d - L, np.where(d < -h, d + L, d))


def is_symmetric(trip, rc2):
    return trip[0] == trip[2] and rc2[0] == rc2[1]


def angle_hist(xyz, box, types, triplets, r_cut_sq, edges, mol_of=None):
    """-> (hist int64 [T, n_bins], n_degenerate int64 [T], count int64 [F, C], centres [C]) as backend.angle_hist."""
    xyz = np.asarray(xyz, dtype=np.float64)
    F = len(xyz)
    L = np.asarray(box, dtype=np.float64).reshape(F, 3)
    types = np.asarray(types).astype(np.int64)
    trip = [tuple(int(v) for v in t) for t in triplets]
    rc2 = np.asarray(r_cut_sq, dtype=np.float64).reshape(len(trip), 2)
    n_bins = len(edges)
    centres = np.flatnonzero(np.isin(types, [t[1] for t in trip]))
    cand = np.flatnonzero(np.isin(types, [t[0] for t in trip] + [t[2] for t in trip]))
    hist = np.zeros((len(trip), n_bins), dtype=np.int64)
    degen = np.zeros(len(trip), dtype=np.int64)
    count = np.zeros((F, len(centres)), dtype=np.int64)
    for ci, c in enumerate(centres):
        mine = [t for t in range(len(trip)) if trip[t][1] == types[c]]
        rmax2 = max(rc2[t].max() for t in mine)
        ok = cand != c
        if mol_of is not None:
            ok &= np.asarray(mol_of)[cand] != np.asarray(mol_of)[c]
        xc = xyz[:, :, c]  # [F, 3]
        ax = [_wrap_abs(xc[:, k, None] - xyz[:, k, cand], L[:, k, None]) for k in range(3)]
        rsq = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]  # [F, n_cand]
        within = ok[None, :] & (rsq < rmax2)
        count[:, ci] = within.sum(axis=1)
        sel = np.flatnonzero(within.any(axis=0))
        if len(sel) < 2:
            continue
        at, rs, ins = cand[sel], rsq[:, sel], within[:, sel]
        d = [_wrap(xyz[:, k, at] - xc[:, k, None], L[:, k, None]) for k in range(3)]
        nrm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        with np.errstate(invalid="ignore", divide="ignore"):
            dot = (d[0][:, :, None] * d[0][:, None, :] + d[1][:, :, None] * d[1][:, None, :]) \
                + d[2][:, :, None] * d[2][:, None, :]
            cos = dot / (nrm[:, :, None] * nrm[:, None, :])  # [F, ns, ns]
        ns = len(sel)
        for t in mine:
            a, _, b = trip[t]
            in_a = ins & (types[at] == a)[None, :] & (rs < rc2[t, 0])
            if is_symmetric(trip[t], rc2[t]):
                pairs = in_a[:, :, None] & in_a[:, None, :] & np.triu(np.ones((ns, ns), dtype=bool), 1)[None]
            else:
                in_b = ins & (types[at] == b)[None, :] & (rs < rc2[t, 1])
                pairs = in_a[:, :, None] & in_b[:, None, :] & ~np.eye(ns, dtype=bool)[None]
            v = cos[pairs]
            nan = np.isnan(v)
            degen[t] += int(nan.sum())
            hist[t] += np.bincount(bin_of(v[~nan], edges), minlength=n_bins)
    return hist, degen, count, centres


def brute_hist(xyz, box, types, triplets, r_cut_sq, edges, mol_of=None):
    """(hist, n_degenerate) of ONE frame xyz [3, N], box [3], as nested loops over the definition."""
    n = xyz.shape[1]
    hist = np.zeros((len(triplets), len(edges)), dtype=np.int64)
    degen = np.zeros(len(triplets), dtype=np.int64)

    def geom(c, j):
        ax = [min(abs(xyz[k, c] - xyz[k, j]), abs(abs(xyz[k, c] - xyz[k, j]) - box[k])) for k in range(3)]
        d = []
        for k in range(3):
            v, Lk = xyz[k, j] - xyz[k, c], box[k]
            d.append(v - Lk if v > 0.5 * Lk else (v + Lk if v < -0.5 * Lk else v))
        return (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2], d

    def role(c, j, ty, r2):
        if j == c or types[j] != ty or (mol_of is not None and mol_of[j] == mol_of[c]):
            return None
        rsq, d = geom(c, j)
        return d if rsq < r2 else None

    for t, ((a, tc, b), (ra2, rb2)) in enumerate(zip(triplets, r_cut_sq)):
        sym = a == b and ra2 == rb2
        for c in range(n):
            if types[c] != tc:
                continue
            for j in range(n):
                dj = role(c, j, a, ra2)
                if dj is None:
                    continue
                for k in range(j + 1 if sym else 0, n):
                    dk = role(c, k, b, rb2)
                    if dk is None or k == j:
                        continue
                    nj = math.sqrt((dj[0] * dj[0] + dj[1] * dj[1]) + dj[2] * dj[2])
                    nk = math.sqrt((dk[0] * dk[0] + dk[1] * dk[1]) + dk[2] * dk[2])
                    den = nj * nk
                    if den == 0.0:
                        degen[t] += 1  # 0 / 0: NaN
                        continue
                    cos = ((dj[0] * dk[0] + dj[1] * dk[1]) + dj[2] * dk[2]) / den
                    hist[t, sum(1 for m in range(1, len(edges)) if cos <= edges[m])] += 1
    return hist, degen


# ---- lattices with closed-form counts ----

def simple_cubic(n, a):
    """(xyz [1, 3, n**3], box [1, 3]): every atom has 6 neighbours at a: 12 angles of 90 and 3 of 180 degrees."""
    g = np.arange(n) * float(a)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    return xyz[None], np.full((1, 3), n * float(a))


def fcc(n, a):
    """(xyz [1, 3, 4 n**3], box [1, 3]): 12 neighbours at a / sqrt(2): 24 angles of 60, 12 of 90, 24 of 120, 6 of 180."""
    g = np.arange(n) * float(a)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]) * float(a)
    xyz = (cells[:, :, None] + basis.T[:, None, :]).reshape(3, -1)
    return xyz[None], np.full((1, 3), n * float(a))


def write_dumps(xyz, box, types, directory, stem="ang"):
    """The frames as LAMMPS dumps, ids 1..N (repr round trip: the same doubles parse back); returns the pattern."""
    from mdproptools_amd.io import write_dump

    n = xyz.shape[2]
    for f in range(len(xyz)):
        tab = np.column_stack([np.arange(1, n + 1), np.asarray(types), xyz[f].T])
        bounds = np.column_stack([np.zeros(3), np.asarray(box[f], dtype=np.float64)])
        write_dump(os.path.join(directory, "%s.%d.dump" % (stem, f)), f, bounds, ["id", "type", "x", "y", "z"], tab)
    return os.path.join(directory, stem + ".*.dump")
