"""
numpy restatement of mdhip_mol_moments and mdhip_vector_pair_hist (include/mdhip.h), operation by operation as the
header states them, and of the host formulas of structural/orientational_correlation.py and structural/dielectric.py.
numpy does not fuse and np.rint rounds half to even; the fixed-point sums are Python integers. Shared by
tests/test_dipole_cpu.py and tests/test_gpu_dipole.py.
"""

import math

import numpy as np

from reorientation_ref import same_bits, write_dumps  # noqa: F401  (the dump writer and the bit comparison of the siblings)

EPS = 2.0 ** -53
ONE = 1 << 32
W_TOTAL = 256  # partial sums of a total (csrc/moments.hip)


# ---- mdhip_mol_moments ---------------------------------------------------------------------------------------------------


def _term_sum(x, box, a, terms, length):
    """sum_k w_k * w(x[a+k] - x[a]) [F,3,M] in ascending k, starting from w_1 * d_1; None without terms."""
    v = None
    for k, w in terms:
        assert 1 <= k < length
        d = x[:, :, a + k] - x[:, :, a]
        if box is not None:
            L = np.asarray(box, dtype=np.float64)[:, :, None]
            half = L / 2
            d = np.where(d > half, d - L, np.where(d < -half, d + L, d))
        p = np.float64(w) * d
        v = p if v is None else v + p
    return v


def tree_sum(v):
    """The fixed order of the totals over the last axis: partial i adds the entries i, i + 256, ... in order, then
    red[i] += red[i + w], w = 128 .. 1."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    red = np.zeros(v.shape[:-1] + (W_TOTAL,))
    for m0 in range(0, n, W_TOTAL):
        chunk = v[..., m0:m0 + W_TOTAL]
        red[..., : chunk.shape[-1]] = red[..., : chunk.shape[-1]] + chunk
    w = W_TOTAL // 2
    while w:
        red[..., :w] = red[..., :w] + red[..., w:2 * w]
        w //= 2
    return red[..., 0]


def mol_moments(x, box, job_atom0, job_mols, job_len, site_terms, vec_terms, job_unit):
    """-> dict: site, vec [F,3,S], total [J,3,F], sq_total [J,F], degenerate uint64 [J]."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    sites, vecs, totals, squares = [], [], [], []
    degenerate = np.zeros(len(job_unit), dtype=np.uint64)
    for j, (a0, mols, length) in enumerate(zip(job_atom0, job_mols, job_len)):
        a = int(a0) + np.arange(int(mols), dtype=np.int64) * int(length)
        o = _term_sum(x, box, a, site_terms[j], length)
        site = x[:, :, a] if o is None else x[:, :, a] + o
        v = _term_sum(x, box, a, vec_terms[j], length)
        if v is None:
            v = np.zeros((F, 3, len(a)))
        elif job_unit[j]:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                n2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
                v = v / np.sqrt(n2)[:, None, :]
            zero = n2 == 0.0
            v[np.broadcast_to(zero[:, None, :], v.shape)] = 0.0
            v[np.broadcast_to(~np.isfinite(n2)[:, None, :], v.shape)] = np.nan
            degenerate[j] = int(zero.sum())
        with np.errstate(invalid="ignore", over="ignore"):
            totals.append(tree_sum(v).T)                                                       # [3,F]
            squares.append(tree_sum((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))  # [F]
        sites.append(site), vecs.append(v)
    return {"site": np.ascontiguousarray(np.concatenate(sites, axis=2)), "vec": np.ascontiguousarray(np.concatenate(vecs, axis=2)),
            "total": np.stack(totals), "sq_total": np.stack(squares), "degenerate": degenerate}


# ---- mdhip_vector_pair_hist ----------------------------------------------------------------------------------------------


def bin_edges(bin_size, nbins):
    """edges[k] = the smallest double whose bin (int)(sqrt(rsq) / bin_size) is k, as mdhip_bin_edges defines them: found
    by bisection on the doubles."""
    edges = np.zeros(nbins + 1)
    for k in range(1, nbins + 1):
        lo, hi = 0.0, (k * bin_size) ** 2 * 1.01 + 1e-300
        assert int(math.sqrt(hi) / bin_size) >= k
        while True:
            mid = lo + (hi - lo) / 2
            if mid == lo or mid == hi:
                break
            if int(np.sqrt(np.float64(mid)) / np.float64(bin_size)) >= k:
                hi = mid
            else:
                lo = mid
        edges[k] = hi
    return edges


def vector_pair_hist(site, vec, box, group_off, jobs, bin_size, nbins, edges=None):
    """-> (hist uint64 [J,nbins], sums object [J,3,nbins] of Python int, beyond, unsummed, pairs uint64 [J])."""
    site, vec, box = (np.asarray(v, dtype=np.float64) for v in (site, vec, box))
    if edges is None:
        edges = bin_edges(bin_size, nbins)
    F = site.shape[0]
    J = len(jobs)
    hist = np.zeros((J, nbins), dtype=np.uint64)
    sums = np.zeros((J, 3, nbins), dtype=object)
    beyond, unsummed, pairs = (np.zeros(J, dtype=np.uint64) for _ in range(3))
    for jn, (ga, gb) in enumerate(jobs):
        ia = np.arange(group_off[ga], group_off[ga + 1])
        ib = np.arange(group_off[gb], group_off[gb + 1])
        pairs[jn] = F * (len(ia) * len(ib) - (len(ia) if ga == gb else 0))
        if not len(ia) or not len(ib):
            continue
        valid = ia[:, None] != ib[None, :]
        for f in range(F):
            with np.errstate(all="ignore"):
                d = []
                for ax in range(3):
                    L = box[f, ax]
                    inv = np.float64(1.0) / L
                    dd = site[f, ax, ib][None, :] - site[f, ax, ia][:, None]
                    d.append(dd - L * np.rint(dd * inv))
                rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                inside = (rsq < edges[nbins]) & valid
                beyond[jn] += int((valid & ~inside).sum())
                ii, jj = np.nonzero(inside)
                if not len(ii):
                    continue
                r2 = rsq[ii, jj]
                k = np.searchsorted(edges, r2, side="right") - 1
                vi, vj = vec[f][:, ia[ii]], vec[f][:, ib[jj]]
                c = (vi[0] * vj[0] + vi[1] * vj[1]) + vi[2] * vj[2]
                c2 = c * c
                e = ((d[0][ii, jj] * vj[0] + d[1][ii, jj] * vj[1]) + d[2][ii, jj] * vj[2]) / np.sqrt(r2)
                ok = (np.abs(c) < 2.0) & (np.abs(c2) < 2.0) & (np.abs(e) < 2.0)  # (False for a NaN)
            np.add.at(hist[jn], k, np.uint64(1))
            unsummed[jn] += int((~ok).sum())
            for s, val in enumerate((c, c2, e)):
                fixed = np.rint(val[ok] * 4294967296.0)
                for kk, add in zip(k[ok].tolist(), fixed.tolist()):
                    sums[jn, s, kk] += int(add)
    return hist, sums, beyond, unsummed, pairs


def split_words(value):
    """(low, high) uint64 words of the 128-bit two's complement of a Python int."""
    v = value % (1 << 128)
    return v & ((1 << 64) - 1), v >> 64


# ---- the host formulas ---------------------------------------------------------------------------------------------------


def pair_columns(hist, sums, n_frames, n_a, n_b, same, mean_volume, bin_size):
    """The columns of calc_orientational_correlation from one pair's integers, formula by formula as its docstring
    states them; every mean one correctly rounded division of two integers."""
    n_bins = len(hist)
    k_bin = np.arange(n_bins, dtype=np.float64)
    shell = 4.0 / 3.0 * math.pi * bin_size ** 3 * ((k_bin + 1.0) ** 3 - k_bin ** 3)
    count = np.array([float(int(h)) for h in hist])
    rho_b = n_b / mean_volume
    with np.errstate(invalid="ignore", divide="ignore"):
        g = count / ((n_frames * n_a) * rho_b * shell)
    mean = lambda s: np.array([int(v) / (ONE * int(h)) if int(h) else float("nan") for v, h in zip(s, hist)])  # noqa: E731
    cum = np.cumsum(np.array([int(v) for v in sums[0]], dtype=object))
    g_k = np.array([(1.0 if same else 0.0) + int(v) / (ONE * n_frames * n_a) for v in cum])
    return {"r": (k_bin + 0.5) * bin_size, "g(r)": g, "<cos>": mean(sums[0]), "<P2>": 1.5 * mean(sums[1]) - 0.5,
            "<cos_r>": mean(sums[2]), "G_K": g_k}


def dielectric(total, sq_total, volume, n_mols, temperature, dipole_unit, distance_unit):
    """eps_r, its running value, <mu^2> and g_K per type from the series in time order (see
    structural/dielectric.py: dielectric_from_series), with the unit factors given: dipole_unit C m, distance_unit m."""
    k_b, eps0 = 1.380649 * 10 ** -23, 8.8541878128 * 10 ** -12
    total, sq_total, volume = (np.asarray(v, dtype=np.float64) for v in (total, sq_total, volume))
    n_types, _, F = total.shape
    M = np.zeros((3, F))
    for t in range(n_types):
        M = M + total[t]
    factor = dipole_unit ** 2 / (3.0 * eps0 * distance_unit ** 3 * k_b * float(temperature))

    def fluctuation(m, upto):
        sq = (m[0, :upto] * m[0, :upto] + m[1, :upto] * m[1, :upto]) + m[2, :upto] * m[2, :upto]
        mean = [np.mean(m[x, :upto]) for x in range(3)]
        return np.mean(sq) - ((mean[0] * mean[0] + mean[1] * mean[1]) + mean[2] * mean[2])

    running = np.array([1.0 + factor * fluctuation(M, n) / np.mean(volume[:n]) for n in range(1, F + 1)])
    mu2 = np.array([np.mean(sq_total[t]) / n_mols[t] if n_mols[t] else np.nan for t in range(n_types)])
    with np.errstate(invalid="ignore", divide="ignore"):
        g_k = np.array([fluctuation(total[t], F) / (n_mols[t] * mu2[t]) if n_mols[t] else np.nan for t in range(n_types)])
    return {"M": M, "eps_r": float(running[-1]), "running": running, "mu2": mu2, "g_K": g_k}


def acf(M, max_lag):
    """Phi(k) = sum_axis c_axis(k) / sum_axis c_axis(0), c(k) = sum_t m[t+k] m[t] / (n - k), m = M - <M> per axis."""
    m = M - np.mean(M, axis=1)[:, None]
    n = M.shape[1]
    c = np.array([[math.fsum(m[x, k:] * m[x, : n - k]) / (n - k) for k in range(max_lag + 1)] for x in range(3)])
    s = (c[0] + c[1]) + c[2]
    return s / s[0]


# ---- a small water-like liquid with ions ---------------------------------------------------------------------------------

NUM_MOLS, ATOMS_PER_MOL = [40, 6], [3, 1]
CHARGES = [np.array([-0.8, 0.4, 0.4]), np.array([1.0])]
GRID = 1024.0  # every coordinate is a multiple of 1 / GRID: the text of the dumps round-trips


def water_like(n_frames=6, box0=12.0, seed=11, integer=False):
    """40 three-site molecules (O, H, H about 1 apart, tumbling) and 6 monatomic ions in a periodic box whose edges change
    from frame to frame; the dict of reorientation_ref.synthetic_trajectory. `integer`: every coordinate a whole number
    (dipoles times 5 and their sums are then small integers: the totals are exact whatever the order)."""
    rng = np.random.default_rng(seed)
    L = box0 + np.arange(n_frames)[:, None] / 32.0 + np.array([0.0, 0.25, 0.5])[None, :]
    lo = np.tile(np.array([0.0, -1.0, 0.5]), (n_frames, 1))
    A = int(np.dot(NUM_MOLS, ATOMS_PER_MOL))
    xu = np.empty((n_frames, 3, A))
    for f in range(n_frames):
        centre = rng.random((3, sum(NUM_MOLS))) * L[f][:, None] + lo[f][:, None]
        for m in range(NUM_MOLS[0]):
            arms = rng.normal(size=(3, 2))
            arms /= np.linalg.norm(arms, axis=0)
            xu[f, :, 3 * m] = centre[:, m]
            xu[f, :, 3 * m + 1:3 * m + 3] = centre[:, m][:, None] + (3.0 * arms if integer else arms)
        xu[f, :, 3 * NUM_MOLS[0]:] = centre[:, NUM_MOLS[0]:]
    xu = np.rint(xu) if integer else np.rint(xu * GRID) / GRID
    if integer:
        L, lo = np.rint(L), np.rint(lo)
    img = np.floor((xu - lo[:, :, None]) / L[:, :, None])
    x = xu - img * L[:, :, None]
    assert np.array_equal(x + img * L[:, :, None], xu)
    types = np.array([1, 2, 2] * NUM_MOLS[0] + [3] * NUM_MOLS[1])
    water = np.array([-2.0, 1.0, 1.0]) if integer else CHARGES[0]
    q = np.concatenate([np.tile(water, NUM_MOLS[0]), np.tile(CHARGES[1], NUM_MOLS[1])])
    return {"steps": 200 * np.arange(n_frames), "lo": lo, "hi": lo + L, "L": L, "ids": np.arange(1, A + 1), "types": types,
            "q": q, "xu": xu, "x": x, "img": img}
