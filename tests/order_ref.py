"""
Plain-numpy restatement of the per-centre order parameters (order parameters): the test oracle of
backend.bond_order and structural/order_parameters.py. Y_lm comes from scipy.special.sph_harm_y; every other step is in
the specified arithmetic, unfused doubles:

- rsq(c, j): per axis a = |x_c - x_j|, min(a, |a - L|) (the |d| form of the single wrap), (ax*ax + ay*ay) + az*az;
  neighbour of c: a candidate (type in neighbour_types), j != c, rsq < r_cut**2 (strict), another molecule under
  exclusion; with n_nearest = k the k smallest by (rsq, atom index), else all; fewer than k (without k: none): short;
- d_j = x_j - x_c, signed wrap d > L/2 ? d - L : (d < -L/2 ? d + L : d); n_j = sqrt((dx*dx + dy*dy) + dz*dz);
  u_j = d_j / n_j; a selected neighbour with n_j == 0 or not finite: the row is degenerate;
- q_lm = (1/N) sum_j Y_lm(u_j) in ascending atom index, q_l = sqrt(4 pi / (2l + 1) sum_m |q_lm|**2);
- qbar_lm(c) = (q_lm(c) + sum_{j in N(c)} q_lm(j)) / (N + 1); NaN of any member (the row itself or a neighbour)
  propagates, and the row counts as short;
- the 4 nearest by (rsq, atom index), in ascending atom index: q_tet = 1 - 3/8 sum_{j<k} (cos_jk + 1/3)**2 with
  cos_jk = ((dxj*dxk + dyj*dyk) + dzj*dzk) / (n_j * n_k), s_k = 1 - 1/3 sum_k (n_k - rbar)**2 / (4 rbar**2); fewer than
  4: short; one of them with n == 0: degenerate.

`q_of_units` and `tetra` take leading batch dimensions; `bond_order` loops over frames and centres.
"""

import numpy as np
from scipy.special import eval_legendre, sph_harm_y

from angular_ref import _wrap, _wrap_abs, fcc, simple_cubic, write_dumps  # noqa: F401  (re-exported to the tests)

Q_SHORT, Q_DEGENERATE, TET_SHORT, TET_DEGENERATE, QBAR_SHORT = 1, 2, 4, 8, 16


def qlm_of_units(u, l):
    """q_lm [..., 2l + 1] (complex, m = -l .. l) of the unit vectors u [..., N, 3]: the mean of Y_lm over the N."""
    u = np.asarray(u, dtype=np.float64)
    theta = np.arctan2(np.hypot(u[..., 0], u[..., 1]), u[..., 2])  # (no arccos: it loses the digits near the poles)
    phi = np.arctan2(u[..., 1], u[..., 0])
    m = np.arange(-l, l + 1)
    y = sph_harm_y(l, m, theta[..., None], phi[..., None])  # [..., N, 2l + 1]
    tot = np.zeros(y.shape[:-2] + (2 * l + 1,), dtype=np.complex128)
    for j in range(y.shape[-2]):  # (ascending atom index)
        tot = tot + y[..., j, :]
    return tot / y.shape[-2]


def q_of_qlm(qlm, l):
    return np.sqrt(4.0 * np.pi / (2 * l + 1) * (np.abs(qlm) ** 2).sum(axis=-1))


def q_of_units(u, l):
    return q_of_qlm(qlm_of_units(u, l), l)


def q_of_shell(d, l):
    """q_l of the shell vectors d [..., N, 3] (not normalised)."""
    d = np.asarray(d, dtype=np.float64)
    return q_of_units(d / np.linalg.norm(d, axis=-1, keepdims=True), l)


def q_sq_addition_theorem(u, l):
    """q_l**2 = (1 / N**2) sum_jk P_l(u_j . u_k): the pair form (the kernel does not use it: near q_l = 0 it loses
    half the digits of q_l)."""
    u = np.asarray(u, dtype=np.float64)
    return eval_legendre(l, np.clip(u @ u.T, -1.0, 1.0)).sum() / len(u) ** 2


def tetra(d):
    """(q_tet, s_k) of four neighbour vectors d [..., 4, 3], already in ascending atom index."""
    d = np.asarray(d, dtype=np.float64)
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])  # [..., 4]
    s = 0.0
    for a in range(3):
        for b in range(a + 1, 4):
            dot = (d[..., a, 0] * d[..., b, 0] + d[..., a, 1] * d[..., b, 1]) + d[..., a, 2] * d[..., b, 2]
            cs = dot / (n[..., a] * n[..., b]) + 1.0 / 3.0
            s = s + cs * cs
    q_tet = 1.0 - 0.375 * s
    rbar = (((n[..., 0] + n[..., 1]) + n[..., 2]) + n[..., 3]) / 4.0
    den = 4.0 * (rbar * rbar)
    v = 0.0
    for a in range(4):
        v = v + ((n[..., a] - rbar) * (n[..., a] - rbar)) / den
    return q_tet, 1.0 - v / 3.0


def bond_order(xyz, box, types, centre_type, neighbour_types, r_cut_sq, degrees=(4, 6), n_nearest=None, averaged=False,
               tetrahedral=False, mol_of=None, cap=None, ctx=None):
    """The dict of backend.bond_order: q [F, C, D], qbar (or None), tet [F, C, 2] (or None), flags, count, centres."""
    xyz = np.asarray(xyz, dtype=np.float64)
    F = len(xyz)
    L = np.asarray(box, dtype=np.float64).reshape(F, 3)
    types = np.asarray(types).astype(np.int64)
    degrees = [int(l) for l in degrees]
    D = len(degrees)
    k_sel = int(n_nearest or 0)
    centres = np.flatnonzero(types == int(centre_type))
    cand = np.flatnonzero(np.isin(types, [int(t) for t in neighbour_types]))
    C = len(centres)
    q = np.full((F, C, D), np.nan)
    qlm = [np.full((F, C, 2 * l + 1), np.nan, dtype=np.complex128) for l in degrees]
    members = [[None] * C for _ in range(F)]
    tet = np.full((F, C, 2), np.nan) if tetrahedral else None
    flags = np.zeros((F, C), dtype=np.int32)
    count = np.zeros((F, C), dtype=np.int32)
    for ci, c in enumerate(centres):
        ok = cand != c
        if mol_of is not None:
            ok &= np.asarray(mol_of)[cand] != np.asarray(mol_of)[c]
        xc = xyz[:, :, c]
        with np.errstate(invalid="ignore"):
            ax = [_wrap_abs(xc[:, k, None] - xyz[:, k, cand], L[:, k, None]) for k in range(3)]
            rsq_all = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]
            within = ok[None, :] & (rsq_all < r_cut_sq)
        count[:, ci] = within.sum(axis=1)
        for f in range(F):
            nb = cand[within[f]]  # ascending atom index
            rsq = rsq_all[f][within[f]]
            d = np.stack([_wrap(xyz[f, k, nb] - xc[f, k], L[f, k]) for k in range(3)], axis=1)  # [n, 3]
            n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            order = np.lexsort((nb, rsq))  # by (rsq, atom index)
            if D:
                if len(nb) == 0 or len(nb) < k_sel:
                    flags[f, ci] |= Q_SHORT
                else:
                    sel = np.sort(order[:k_sel]) if k_sel else np.arange(len(nb))
                    if not np.all((n[sel] > 0) & np.isfinite(n[sel])):
                        flags[f, ci] |= Q_DEGENERATE
                    else:
                        u = d[sel] / n[sel, None]
                        for di, l in enumerate(degrees):
                            qlm[di][f, ci] = qlm_of_units(u, l)
                            q[f, ci, di] = q_of_qlm(qlm[di][f, ci], l)
                        members[f][ci] = nb[sel]
            if tetrahedral:
                if len(nb) < 4:
                    flags[f, ci] |= TET_SHORT
                else:
                    four = np.sort(order[:4])
                    if not np.all((n[four] > 0) & np.isfinite(n[four])):
                        flags[f, ci] |= TET_DEGENERATE
                    else:
                        tet[f, ci] = tetra(d[four])
    qbar = None
    if averaged:
        if not np.array_equal(cand, centres):
            raise ValueError("averaged needs neighbour_types == [centre_type]")
        centre_of = {int(a): i for i, a in enumerate(centres)}
        qbar = np.full((F, C, D), np.nan)
        for f in range(F):
            for ci in range(C):
                mem = members[f][ci]
                if mem is not None:
                    for di, l in enumerate(degrees):
                        tot = qlm[di][f, ci].copy()
                        for j in mem:  # (ascending atom index)
                            tot = tot + qlm[di][f, centre_of[int(j)]]
                        qbar[f, ci, di] = q_of_qlm(tot / (len(mem) + 1), l)
                if np.isnan(qbar[f, ci]).any():
                    flags[f, ci] |= QBAR_SHORT
    return {"q": q, "qbar": qbar, "tet": tet, "flags": flags, "count": count, "centres": centres.astype(np.int32)}


# ---- shells and lattices with closed-form values ----

def bcc(n, a):
    """(xyz [1, 3, 2 n**3], box [1, 3]): 8 neighbours at a sqrt(3) / 2, 6 more at a."""
    g = np.arange(n) * float(a)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0.5]]) * float(a)
    xyz = (cells[:, :, None] + basis.T[:, None, :]).reshape(3, -1)
    return xyz[None], np.full((1, 3), n * float(a))


def diamond(n, a):
    """(xyz [1, 3, 8 n**3], box [1, 3]): 4 neighbours at a sqrt(3) / 4, 12 more at a / sqrt(2)."""
    g = np.arange(n) * float(a)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    f = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    basis = np.concatenate([f, f + 0.25]) * float(a)
    xyz = (cells[:, :, None] + basis.T[:, None, :]).reshape(3, -1)
    return xyz[None], np.full((1, 3), n * float(a))


def shell_sc():
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def shell_fcc():
    s = [(a, b, 0) for a in (1, -1) for b in (1, -1)]
    return np.array(s + [(a, 0, b) for a, b, _ in s] + [(0, a, b) for a, b, _ in s], dtype=np.float64)


def shell_bcc8():
    return np.array([(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)], dtype=np.float64)


def shell_bcc14():
    return np.concatenate([shell_bcc8(), 2.0 * shell_sc()])


def shell_hcp():
    """The 12 nearest neighbours of an ideal hcp site: 6 in the plane, 3 above, 3 below (the same triangle)."""
    ang = np.arange(6) * np.pi / 3
    plane = np.stack([np.cos(ang), np.sin(ang), np.zeros(6)], axis=1)
    h = np.sqrt(2.0 / 3.0)
    tri = np.array([[0.5, np.sqrt(3) / 6, 0], [-0.5, np.sqrt(3) / 6, 0], [0, -np.sqrt(3) / 3, 0]])
    return np.concatenate([plane, tri + [0, 0, h], tri - [0, 0, h]])


def shell_icosahedron():
    g = (1 + np.sqrt(5)) / 2
    s = [(0, a, b * g) for a in (1, -1) for b in (1, -1)]
    return np.array(s + [(a, b, 0) for _, a, b in s] + [(b, 0, a) for _, a, b in s], dtype=np.float64)


def shell_diamond():
    return np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
