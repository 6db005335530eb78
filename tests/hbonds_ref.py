"""
Plain-numpy restatement of the hydrogen-bond analysis (hydrogen bonds): the test oracle of
backend.hbond_counts, backend.hbond_lifetime and structural/hydrogen_bonds.py. Every step in the specified arithmetic,
unfused doubles:

- rsq(p, q): per axis a = |x_p - x_q|, min(a, |a - L|) (the |d| form of the single wrap), (ax*ax + ay*ay) + az*az;
- hydrogen h of donor d is bonded to acceptor a when the atom of a is not the atom of d, mol_of differs under
  exclusion, rsq(d, a) < r_da_sq (strict), rsq(h, a) < r_ha_sq (when r_ha_sq > 0) and cos <= cos_cut, where
  u = x_d - x_h, v = x_a - x_h, each with the signed wrap d > L/2 ? d - L : (d < -L/2 ? d + L : d), and
  cos = ((ux*vx + uy*vy) + uz*vz) / (sqrt((ux*ux + uy*uy) + uz*uz) * sqrt((vx*vx + vy*vy) + vz*vz));
- a NaN cosine is no bond and counts in n_degenerate; a comparison with a non-finite value is false;
- the angle histogram takes every (h, a) that passes every test but the angle test: bin = the number of m in
  [1, n_bins) with cos <= E[m] (angular_ref.bin_of);
- with h(t) the indicator of a pair over the frames, c_int[k] = sum_t h(t) h(t + k) and c_cont[k] = the number of t
  with h(t) = ... = h(t + k) = 1, summed over the pairs.

`geometry` is vectorised over frames, hydrogens and acceptors; `brute_lifetime` is the lifetime definition as nested
Python loops over bit patterns, for small cross-checks.
"""

import os

import numpy as np

from angular_ref import bin_of, cos_edges  # noqa: F401  (the same table and rule)


def _wrap_abs(d, L):
    a = np.abs(d)
    return np.minimum(a, np.abs(a - L))


def _wrap(d, L):
    h = 0.5 * L
    return np.where(d > h, d - L, np.where(d < -h, d + L, d))


def rsq(p, q, L):
    """p, q [..., 3, ...] broadcastable with the axis of length 3 FIRST: p[k], q[k], L[k]."""
    ax, ay, az = (_wrap_abs(p[k] - q[k], L[k]) for k in range(3))
    return (ax * ax + ay * ay) + az * az


def cosine(xd, xh, xa, L):
    """The cosine of the angle at H between D and A (arrays with the axis of length 3 first)."""
    u = [_wrap(xd[k] - xh[k], L[k]) for k in range(3)]
    v = [_wrap(xa[k] - xh[k], L[k]) for k in range(3)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dot = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
        nu = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return dot / (nu * nv)


def donor_of(h_off):
    """[n_h]: the donor position of every hydrogen position."""
    h_off = np.asarray(h_off, dtype=np.int64)
    return np.repeat(np.arange(len(h_off) - 1), np.diff(h_off))


def geometry(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, r_ha_sq, mol_of=None):
    """-> (reach bool [F, n_h, n_acc]: every test but the angle test passed, cos float64 [F, n_h, n_acc])."""
    xyz = np.asarray(xyz, dtype=np.float64)
    F = len(xyz)
    L = np.asarray(box, dtype=np.float64).reshape(F, 3).T[:, :, None, None]  # [3, F, 1, 1]
    don, hat, acc = (np.asarray(v, dtype=np.int64) for v in (donors, h_atoms, acceptors))
    dh = don[donor_of(h_off)]  # the donor atom of every hydrogen
    xd = xyz[:, :, dh].transpose(1, 0, 2)[:, :, :, None]   # [3, F, n_h, 1]
    xh = xyz[:, :, hat].transpose(1, 0, 2)[:, :, :, None]
    xa = xyz[:, :, acc].transpose(1, 0, 2)[:, :, None, :]  # [3, F, 1, n_acc]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (dh[:, None] != acc[None, :])[None]
        if mol_of is not None:
            m = np.asarray(mol_of)
            ok = ok & (m[dh][:, None] != m[acc][None, :])[None]
        reach = ok & (rsq(xd, xa, L) < r_da_sq)
        if r_ha_sq > 0:
            reach = reach & (rsq(xh, xa, L) < r_ha_sq)
        cos = cosine(xd, xh, xa, L)
    return reach, cos


def bonded(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, r_ha_sq, cos_cut, mol_of=None):
    """bool [F, n_h, n_acc]."""
    reach, cos = geometry(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, r_ha_sq, mol_of)
    with np.errstate(invalid="ignore"):
        return reach & (cos <= cos_cut)


def hbond_counts(xyz, box, donors, don_class, h_off, h_atoms, acceptors, acc_class, r_da_sq, cos_cut, r_ha_sq=0.0,
                 edges=None, mol_of=None, n_dc=None, n_ac=None):
    """-> (n_bonds [F, n_dc, n_ac], n_donated [n_don], n_accepted [n_acc], angle_hist [n_dc, n_ac, n_bins],
    n_degenerate), int64, as backend.hbond_counts."""
    reach, cos = geometry(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, r_ha_sq, mol_of)
    F = len(reach)
    dcl, acl = np.asarray(don_class, dtype=np.int64), np.asarray(acc_class, dtype=np.int64)
    n_dc = int(n_dc) if n_dc is not None else int(dcl.max()) + 1
    n_ac = int(n_ac) if n_ac is not None else int(acl.max()) + 1
    dpos = donor_of(h_off)
    hcl = dcl[dpos]  # class of every hydrogen's donor
    nan = np.isnan(cos)
    with np.errstate(invalid="ignore"):
        bond = reach & (cos <= cos_cut)
    n_bonds = np.zeros((F, n_dc, n_ac), dtype=np.int64)
    n_bins = 0 if edges is None else len(edges)
    hist = np.zeros((n_dc, n_ac, n_bins), dtype=np.int64)
    for dc in range(n_dc):
        for ac in range(n_ac):
            sel = np.ix_(np.arange(F), np.flatnonzero(hcl == dc), np.flatnonzero(acl == ac))
            n_bonds[:, dc, ac] = bond[sel].sum(axis=(1, 2))
            if n_bins:
                v = cos[sel][reach[sel] & ~nan[sel]]
                hist[dc, ac] = np.bincount(bin_of(v, edges), minlength=n_bins)
    n_donated = np.zeros(len(dcl), dtype=np.int64)
    np.add.at(n_donated, dpos, bond.sum(axis=(0, 2)))
    n_accepted = bond.sum(axis=(0, 1)).astype(np.int64)
    return n_bonds, n_donated, n_accepted, hist, int((reach & nan).sum())


def lifetime_sums(h, max_lag):
    """h bool [P, F] -> (c_int, c_cont) int64 [max_lag + 1], vectorised over the pairs."""
    h = np.asarray(h, dtype=bool)
    F = h.shape[1]
    c_int = np.zeros(max_lag + 1, dtype=np.int64)
    c_cont = np.zeros(max_lag + 1, dtype=np.int64)
    alive = h.copy()  # alive[:, t]: h(t) = ... = h(t + k) = 1
    for k in range(max_lag + 1):
        c_int[k] = int((h[:, :F - k] & h[:, k:]).sum())
        c_cont[k] = int(alive.sum())
        if k + 1 < F:
            alive = alive[:, :-1] & h[:, k + 1:]
    return c_int, c_cont


def brute_lifetime(patterns, max_lag):
    """The same sums as nested loops over lists of 0 / 1."""
    c_int, c_cont = [0] * (max_lag + 1), [0] * (max_lag + 1)
    for bits in patterns:
        n = len(bits)
        for k in range(max_lag + 1):
            for t in range(n - k):
                if bits[t] and bits[t + k]:
                    c_int[k] += 1
                if all(bits[t:t + k + 1]):
                    c_cont[k] += 1
    return np.array(c_int, dtype=np.int64), np.array(c_cont, dtype=np.int64)


def hbond_lifetime(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, cos_cut, r_ha_sq=0.0, mol_of=None,
                   max_lag=None):
    """-> (c_int, c_cont, n_pairs, n_records) as backend.hbond_lifetime."""
    b = bonded(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, r_ha_sq, cos_cut, mol_of)
    F = len(b)
    h = b.reshape(F, -1).T  # [pairs, F]
    max_lag = F - 1 if max_lag is None else max_lag
    c_int, c_cont = lifetime_sums(h, max_lag)
    return c_int, c_cont, int(h.any(axis=1).sum()), int(h.sum())


def trapezoid(y, dx):
    y = np.asarray(y, dtype=np.float64)
    return float(((y[1:] + y[:-1]) * 0.5 * dx).sum())


def write_dumps(xyz, box, directory, stem="hb", step=1, steps=None):
    """The frames as LAMMPS dumps, ids 1..N, type 1 (repr round trip: the same doubles parse back); timestep f * step
    (or steps[f]); returns the pattern."""
    from mdproptools_amd.io import write_dump

    n = xyz.shape[2]
    for f in range(len(xyz)):
        tab = np.column_stack([np.arange(1, n + 1), np.ones(n), xyz[f].T])
        bounds = np.column_stack([np.zeros(3), np.asarray(box[f], dtype=np.float64)])
        ts = int(steps[f]) if steps is not None else f * step
        write_dump(os.path.join(directory, "%s.%d.dump" % (stem, ts)), ts, bounds, ["id", "type", "x", "y", "z"], tab)
    return os.path.join(directory, stem + ".*.dump")
