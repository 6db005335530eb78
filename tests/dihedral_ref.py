"""
numpy restatement of mdhip_dihedral_angles (include/mdhip.h) and of the tables structural/dihedral_distribution.py makes
of it; no GPU and no torch.

dihedral_angles repeats the stated operations in the stated order — explicit two-product cross terms, never np.cross
or np.einsum, which may reorder; numpy never fuses a product into a sum — so the library's histograms and U can be
compared with `==`. The bin is decided on the cosine against the host's cos(m * D) and on the sign of s; `atan2_bins`
is the independent route floor((degrees(atan2) + 180) / D) the CPU tests hold it against.
"""
import numpy as np

TM, TF = 64, 64  # molecules x frames per tile of the kernel (csrc/dihedrals.hip)


def cos_edges(n_bins):
    return np.cos(np.radians(np.arange(n_bins // 2) * (360.0 / n_bins)))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def torsion_terms(b1, b2, b3):
    """(c, s, sn, den, lb) of bond vectors given as triples of arrays (x, y, z), in the header's operations."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        l1, l2, lb = np.sqrt(_dot(n1, n1)), np.sqrt(_dot(n2, n2)), np.sqrt(_dot(b2, b2))
        den = l1 * l2
        c = _dot(n1, n2) / den
        s = _dot(b1, n2)
        sn = (s * lb) / den
    return c, s, sn, den, lb


def bins_of(c, s, n_bins, edges=None):
    """The bin of every (c, s): m = #{q in [1, n_bins/2): c <= edges[q]}, mirrored by the sign of s (+-0: positive)."""
    edges = cos_edges(n_bins) if edges is None else edges
    nb2 = n_bins // 2
    m = np.searchsorted(-edges[1:], -c, side="right")      # edges descend: -edges ascend; counts -edges[q] <= -c
    return np.where(s >= 0, nb2 + m, nb2 - 1 - m)


def dihedral_angles(x, box, job_atom0, job_mols, job_len, quads, job_row=None, n_bins=None, want_series=True):
    """-> (hist uint64 [n_rows, n_bins] or None, U [S,3,F] or None, degenerate uint64 [n_jobs]); x [F,3,A], box [F,3] or
    None, quads[j] = (i, j, k, l) 0-based inside the molecule."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    J = len(quads)
    rows = np.arange(J) if job_row is None else np.asarray(job_row)
    hist = None
    if n_bins is not None:
        hist = np.zeros((int(rows.max()) + 1, n_bins), dtype=np.uint64)
        edges = cos_edges(n_bins)
    out, degenerate = [], np.zeros(J, dtype=np.uint64)
    for j, (a0, mols, length, quad) in enumerate(zip(job_atom0, job_mols, job_len, quads)):
        assert len(set(quad)) == 4 and all(0 <= q < length for q in quad)
        a = int(a0) + np.arange(int(mols), dtype=np.int64) * int(length)
        p = [x[:, :, a + int(q)] for q in quad]                       # [F,3,M] each; only named atoms are read
        bonds = []
        for lo, hi in ((0, 1), (1, 2), (2, 3)):
            with np.errstate(invalid="ignore", over="ignore"):
                d = p[hi] - p[lo]
                if box is not None:
                    L = np.asarray(box, dtype=np.float64)[:, :, None]
                    half = L / 2
                    d = np.where(d > half, d - L, np.where(d < -half, d + L, d))
            bonds.append((d[:, 0], d[:, 1], d[:, 2]))
        c, s, sn, den, _ = torsion_terms(*bonds)                      # [F,M]
        zero = den == 0.0
        nan = ~zero & (np.isnan(c) | np.isnan(s))
        ok = ~zero & ~nan
        degenerate[j] = int(zero.sum())
        if hist is not None:
            b = bins_of(c[ok], s[ok], n_bins, edges)
            hist[rows[j]] += np.bincount(b, minlength=n_bins).astype(np.uint64)
        if want_series:
            u = np.zeros((F, 3, int(mols)))
            u[:, 0], u[:, 1] = np.where(zero, 0.0, c), np.where(zero, 0.0, sn)
            u[:, 0][nan] = np.nan
            u[:, 1][nan] = np.nan
            out.append(np.ascontiguousarray(u.transpose(2, 1, 0)))
    U = (np.concatenate(out) if out else np.zeros((0, 3, F))) if want_series else None
    return hist, U, degenerate


def atan2_bins(b1, b2, b3, n_bins):
    """The independent route: floor((degrees(atan2(lb * s, dot(n1, n2))) + 180) / D), bond vectors as in torsion_terms."""
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    lb = np.sqrt(_dot(b2, b2))
    phi = np.degrees(np.arctan2(lb * _dot(b1, n2), _dot(n1, n2)))
    return np.floor((phi + 180.0) / (360.0 / n_bins)).astype(np.int64)


def chain(phi_deg, theta_deg=111.0, bond=1.53):
    """Four atoms [4,3] of a butane-like chain with bond angles theta and the torsion phi (IUPAC sign)."""
    th, ph = np.radians(theta_deg), np.radians(phi_deg)
    p1 = np.array([0.0, 0.0, 0.0])
    p2 = p1 + np.array([bond, 0.0, 0.0])                               # b2 = p2 - p1 along +x
    p0 = p1 + bond * np.array([np.cos(th), np.sin(th), 0.0])           # b1 = p1 - p0
    # p3: the image of p0 through the midpoint geometry at torsion 0 (cis, same side), turned by phi about j -> k
    y, z = np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph)
    p3 = p2 + bond * np.array([-np.cos(th), y, z])
    return np.stack([p0, p1, p2, p3])


# ---- a small synthetic trajectory for the end-to-end tests ------------------------------------------------------------

NUM_MOLS, ATOMS_PER_MOL = [70, 9], [4, 6]
GRID = 1024.0  # every coordinate is a multiple of 1 / GRID: differences and wraps are exact, the text round-trips


def synthetic_trajectory(n_frames=40, box0=12.0, seed=11):
    """70 four-site chains and 9 six-site chains whose atoms jitter about a zigzag that drifts through a periodic box
    with edges that change per frame and axis. -> dict: steps [F] (equally spaced), lo / hi / L [F,3], ids, types [A],
    xu [F,3,A] unwrapped, x wrapped atom by atom into the box, img the image counts (xu = x + img * L exactly)."""
    rng = np.random.default_rng(seed)
    L = box0 + np.arange(n_frames)[:, None] / 64.0 + np.array([0.0, 0.5, 1.0])[None, :]
    lo = np.tile(np.array([0.0, -1.0, 0.25]), (n_frames, 1))
    xu, types = [], []
    for t, (mols, per) in enumerate(zip(NUM_MOLS, ATOMS_PER_MOL)):
        for _ in range(mols):
            centre = rng.random(3) * box0 + np.cumsum(rng.normal(0.0, 0.3, size=(n_frames, 3)), axis=0)    # [F,3]
            body = np.stack([1.3 * np.arange(per), 0.6 * (np.arange(per) % 2), np.zeros(per)], axis=1)     # zigzag
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            jitter = np.cumsum(rng.normal(0.0, 0.12, size=(n_frames, per, 3)), axis=0) + rng.normal(0, 0.3, (1, per, 3))
            pos = centre[:, None, :] + (body[None] + jitter) @ Q.T                                           # [F,per,3]
            xu.append(pos.transpose(0, 2, 1))
            types += [t + 1] * per
    xu = np.rint(np.concatenate(xu, axis=2) * GRID) / GRID
    img = np.floor((xu - lo[:, :, None]) / L[:, :, None])
    x = xu - img * L[:, :, None]
    assert np.array_equal(x + img * L[:, :, None], xu) and np.all(x >= lo[:, :, None]) and np.all(x < (lo + L)[:, :, None])
    A = xu.shape[2]
    return {"steps": 250 * np.arange(n_frames), "lo": lo, "hi": lo + L, "L": L, "ids": np.arange(1, A + 1),
            "types": np.array(types), "xu": xu, "x": x, "img": img}


def write_dumps(directory, traj, file_order=None, shuffle_seed=5):
    """One LAMMPS dump file per frame with the columns id type x y z ix iy iz xu yu zu, the atoms in a shuffled order.
    The files are named `traj.<n>.dump` with n the frame's place in `file_order` (default: time order), so a shuffled
    file_order gives a trajectory whose timestep column is out of order. -> the '*' pattern that matches them."""
    import os

    rng = np.random.default_rng(shuffle_seed)
    A = len(traj["ids"])
    order = range(len(traj["steps"])) if file_order is None else file_order
    for n, f in enumerate(order):
        rows = rng.permutation(A)
        with open(os.path.join(str(directory), "traj.%d.dump" % n), "w") as fh:
            fh.write("ITEM: TIMESTEP\n%d\nITEM: NUMBER OF ATOMS\n%d\nITEM: BOX BOUNDS pp pp pp\n" % (traj["steps"][f], A))
            for k in range(3):
                fh.write("%.10f %.10f\n" % (traj["lo"][f, k], traj["hi"][f, k]))
            fh.write("ITEM: ATOMS id type x y z ix iy iz xu yu zu\n")
            for i in rows:
                fh.write("%d %d %.10f %.10f %.10f %d %d %d %.10f %.10f %.10f\n" % (
                    (traj["ids"][i], traj["types"][i]) + tuple(traj["x"][f, :, i])
                    + tuple(int(v) for v in traj["img"][f, :, i]) + tuple(traj["xu"][f, :, i])))
    return os.path.join(str(directory), "traj.*.dump")


def entry_jobs(entries):
    """(job_atom0, job_mols, job_len, quads 0-based, job_row, group_off) of entries [(mol_type, [(i,j,k,l) 1-based])]
    over the synthetic layout: one job per quadruple, the jobs of an entry pooled into its row / group."""
    first = np.concatenate(([0], np.cumsum(np.multiply(NUM_MOLS, ATOMS_PER_MOL))))
    a0, mols, length, quads, rows, sizes = [], [], [], [], [], []
    for e, (mol_type, qs) in enumerate(entries):
        t = mol_type - 1
        for q in qs:
            a0.append(first[t]), mols.append(NUM_MOLS[t]), length.append(ATOMS_PER_MOL[t])
            quads.append([v - 1 for v in q]), rows.append(e)
        sizes.append(NUM_MOLS[t] * len(qs))
    return (np.array(a0, dtype=np.int64), np.array(mols, dtype=np.int64), np.array(length, dtype=np.int32),
            np.array(quads, dtype=np.int32), np.array(rows, dtype=np.int32),
            np.concatenate(([0], np.cumsum(sizes))).astype(np.int64))


# ---- the tables of structural/dihedral_distribution.py ------------------------------------------------------------------


def density(hist_row, n_bins):
    """counts / (total * D); all NaN without counts."""
    total = int(hist_row.sum())
    D = 360.0 / n_bins
    return hist_row.astype(np.int64) / (total * D) if total else np.full(n_bins, np.nan)


def population(hist_row, lo, hi, n_bins):
    """The share of the counts in [lo, hi) degrees (whole bins; lo > hi wraps through +-180)."""
    D = 360.0 / n_bins
    b0, b1 = int(round((lo + 180.0) / D)), int(round((hi + 180.0) / D))
    cnt = hist_row.astype(np.int64)
    inside = int(cnt[b0:b1].sum()) if lo <= hi else int(cnt[b0:].sum() + cnt[:b1].sum())
    total = int(cnt.sum())
    return inside / total if total else float("nan")
