"""
numpy restatement of mdhip_mol_shape (include/mdhip.h), operation by operation as the header states them, and of the
tables structural/molecular_shape.py makes of it; no GPU and no torch.

Vectorised over molecules and frames, with explicit loops over the atoms k, the sweeps and the rotations; no np.cross,
np.einsum or np.linalg, which may reorder, and numpy never fuses a product into a sum: the library's counts can be
compared with `==` and its values bit for bit (reorientation_ref.same_bits). The totals go through the tree of
dipole_ref. Shared by tests/test_shape_cpu.py and tests/test_gpu_shape.py.
"""
import numpy as np

from dipole_ref import bin_edges, tree_sum
from reorientation_ref import same_bits  # noqa: F401

N_SWEEPS = 5            # csrc/mol_shape.hip: SH_SWEEPS
CAP, RUN_MOLS = 1024, 256  # atoms per LDS stage, molecules per run (csrc/shape_plan.h)
TOTALS = ("Rg2", "Rg", "Ree2", "l1", "l2", "l3", "k2", "I2", "Rg4")
VALUES = ("Rg2", "Ree2", "k2", "l1", "l2", "l3")


def _wrap(d, L):
    if L is None:
        return d
    half = L / 2
    return np.where(d > half, d - L, np.where(d < -half, d + L, d))


def positions(x, box, a, length, unwrap):
    """p_k [F,3,M] for k = 0 .. length-1, one after the other (a generator: the tensor pass forms them again)."""
    L = None if box is None else np.asarray(box, dtype=np.float64)[:, :, None]
    first = x[:, :, a]
    p = np.zeros(first.shape)
    yield p
    for k in range(1, length):
        if unwrap:
            p = p + _wrap(x[:, :, a + k] - x[:, :, a + k - 1], L)
        else:
            p = _wrap(x[:, :, a + k] - first, L)
        yield p


def rotate(g, p, q, r):
    """One Jacobi rotation of the pair (p, q), r the third axis, on the dict g of arrays keyed by frozenset pairs / axes."""
    pq, rp, rq = frozenset((p, q)), frozenset((r, p)), frozenset((r, q))
    gpq = g[pq]
    live = gpq != 0.0
    with np.errstate(all="ignore"):
        theta = (g[q] - g[p]) / (2.0 * gpq)
        root = np.sqrt(theta * theta + 1.0)
        t = np.where(theta >= 0.0, 1.0 / (theta + root), -1.0 / (-theta + root))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        u = t * gpq
        a, b = g[rp], g[rq]
        new = {p: g[p] - u, q: g[q] + u, pq: np.zeros_like(gpq), rp: c * a - s * b, rq: s * a + c * b}
    for key, val in new.items():
        g[key] = np.where(live, val, g[key])


def principal_moments(gxx, gyy, gzz, gxy, gyz, gzx, sweeps=N_SWEEPS):
    """(l1, l2, l3) of the tensors by `sweeps` sweeps of cyclic Jacobi over (x,y), (x,z), (y,z), then the three
    compare-exchanges of the header."""
    g = {0: np.array(gxx, dtype=np.float64), 1: np.array(gyy, dtype=np.float64), 2: np.array(gzz, dtype=np.float64),
         frozenset((0, 1)): np.array(gxy, dtype=np.float64), frozenset((1, 2)): np.array(gyz, dtype=np.float64),
         frozenset((2, 0)): np.array(gzx, dtype=np.float64)}
    for _ in range(sweeps):
        rotate(g, 0, 1, 2)
        rotate(g, 0, 2, 1)
        rotate(g, 1, 2, 0)
    a, b, d = g[0], g[1], g[2]
    sw = a < b
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    sw = b < d
    b, d = np.where(sw, d, b), np.where(sw, b, d)
    sw = a < b
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    return a, b, d


def tensors(x, box, a, length, w, ends, unwrap):
    """(Gxx, Gyy, Gzz, Gxy, Gyz, Gzx, Ree2) [F,M] each, of the molecules whose first atoms are `a`."""
    w = np.asarray(w, dtype=np.float64)
    M = np.float64(0.0)
    for k in range(length):
        M = M + w[k]
    with np.errstate(all="ignore"):
        s = np.zeros(x[:, :, a].shape)
        pe = {}
        for k, p in enumerate(positions(x, box, a, length, unwrap)):
            s = s + w[k] * p
            if k == ends[0]:
                pe[0] = p
            if k == ends[1]:
                pe[1] = p
        c = s / M
        G = [np.zeros(s[:, 0].shape) for _ in range(6)]
        for k, p in enumerate(positions(x, box, a, length, unwrap)):
            q = p - c
            t = w[k] * q
            G[0] = G[0] + t[:, 0] * q[:, 0]
            G[1] = G[1] + t[:, 1] * q[:, 1]
            G[2] = G[2] + t[:, 2] * q[:, 2]
            G[3] = G[3] + t[:, 0] * q[:, 1]
            G[4] = G[4] + t[:, 1] * q[:, 2]
            G[5] = G[5] + t[:, 2] * q[:, 0]
        G = [g / M for g in G]
        r = pe[1] - pe[0]
        ree2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    return G + [ree2]


def invariants(gxx, gyy, gzz, gxy, gyz, gzx):
    """(Rg2, I2, k2) of the tensors; k2 = 0 where Rg2 == 0."""
    with np.errstate(all="ignore"):
        rg2 = (gxx + gyy) + gzz
        i2 = ((gxx * gyy + gyy * gzz) + gzz * gxx) - ((gxy * gxy + gyz * gyz) + gzx * gzx)
        k2 = np.where(rg2 == 0.0, 0.0, 1.0 - (3.0 * i2) / (rg2 * rg2))
    return rg2, i2, k2


def radial_bins(v, edges, n_bins):
    """(bins of the v with 0 <= v < edges[n_bins], the number of all others)."""
    v = np.asarray(v).ravel()
    with np.errstate(invalid="ignore"):
        inside = (v >= 0.0) & (v < edges[n_bins])
    k = np.searchsorted(edges, v[inside], side="right") - 1
    return np.bincount(k, minlength=n_bins).astype(np.uint64), int((~inside).sum())


def mol_shape(x, box, job_atom0, job_mols, job_len, weights, ends=None, unwrap=1, bin_size=0.05, n_bins=200, n_kbins=50,
              edges=None, sweeps=N_SWEEPS):
    """-> dict as backend.mol_shape returns it (per_mol [F,6,S] and totals [J,9,F] always), plus "uncounted" uint64 [J]:
    the (molecule, frame) pairs with a non-finite k2 and Rg2 != 0."""
    x = np.asarray(x, dtype=np.float64)
    F, J = x.shape[0], len(weights)
    edges = bin_edges(bin_size, n_bins) if edges is None else edges
    out = {"hist_rg": np.zeros((J, n_bins), dtype=np.uint64), "hist_ee": np.zeros((J, n_bins), dtype=np.uint64),
           "hist_k": np.zeros((J, n_kbins), dtype=np.uint64), "beyond": np.zeros((J, 2), dtype=np.uint64),
           "degenerate": np.zeros(J, dtype=np.uint64), "uncounted": np.zeros(J, dtype=np.uint64)}
    values, totals = [], []
    for j, (a0, mols, length) in enumerate(zip(job_atom0, job_mols, job_len)):
        length = int(length)
        a = int(a0) + np.arange(int(mols), dtype=np.int64) * length
        e = (0, length - 1) if ends is None else tuple(int(v) for v in ends[j])
        gxx, gyy, gzz, gxy, gyz, gzx, ree2 = tensors(x, box, a, length, weights[j], e, unwrap)
        rg2, i2, k2 = invariants(gxx, gyy, gzz, gxy, gyz, gzx)
        l1, l2, l3 = principal_moments(gxx, gyy, gzz, gxy, gyz, gzx, sweeps)
        out["hist_rg"][j], out["beyond"][j, 0] = radial_bins(rg2, edges, n_bins)
        out["hist_ee"][j], out["beyond"][j, 1] = radial_bins(ree2, edges, n_bins)
        zero = rg2 == 0.0
        ok = ~zero & np.isfinite(k2)
        out["degenerate"][j] = int(zero.sum())
        out["uncounted"][j] = int((~zero & ~ok).sum())
        with np.errstate(all="ignore"):
            kb = k2[ok] * np.float64(n_kbins)
            b = np.where(kb >= n_kbins, n_kbins - 1, np.where(kb < 0.0, 0, np.trunc(np.clip(kb, -1, n_kbins)))).astype(np.int64)
            out["hist_k"][j] = np.bincount(b, minlength=n_kbins).astype(np.uint64)
            values.append(np.stack([rg2, ree2, k2, l1, l2, l3], axis=1))                      # [F,6,M]
            totals.append(np.stack([tree_sum(v) for v in (rg2, np.sqrt(rg2), ree2, l1, l2, l3, k2, i2, rg2 * rg2)]))
    out["per_mol"] = np.ascontiguousarray(np.concatenate(values, axis=2))
    out["totals"] = np.stack(totals)
    return out


# ---- the tables of structural/molecular_shape.py ---------------------------------------------------------------------------


def density(hist_row, width):
    """counts / (total * width); all NaN without counts."""
    total = int(hist_row.sum())
    return hist_row.astype(np.int64) / (total * width) if total else np.full(len(hist_row), np.nan)


def summary_row(totals, n_mols, n_frames):
    """The summary columns of one molecule type from its totals [9,F] in time order: plain means over molecules and
    frames (np.sum over the frames, one division), then the formulas of calc_molecular_shape's docstring."""
    n = float(n_mols * n_frames)
    if not n:
        return None
    mean = {name: float(np.sum(totals[k])) / n for k, name in enumerate(TOTALS)}
    return {"<Rg>": mean["Rg"], "<Rg2>^1/2": np.sqrt(mean["Rg2"]), "<Ree2>^1/2": np.sqrt(mean["Ree2"]),
            "<Ree2>/<Rg2>": mean["Ree2"] / mean["Rg2"] if mean["Rg2"] else np.nan,
            "<l1>": mean["l1"], "<l2>": mean["l2"], "<l3>": mean["l3"],
            "asphericity": mean["l1"] - (mean["l2"] + mean["l3"]) / 2, "acylindricity": mean["l2"] - mean["l3"],
            "<k2>": mean["k2"], "k2 (ratio of averages)": 1.0 - 3.0 * mean["I2"] / mean["Rg4"] if mean["Rg4"] else np.nan}
