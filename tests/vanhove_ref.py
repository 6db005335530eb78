"""
numpy restatement of mdhip_van_hove_distinct (include/mdhip.h), the same from plain Python loops, and the tables
Displacement.calc_van_hove_distinct builds from it. The reference has no van Hove code, so there is no golden: this
restatement is the yardstick, as tests/displacement_ref.py is for the self part, and tests/test_vanhove_cpu.py checks
it against the loops and against a direct all-pairs count. The system builders and the dump writer are those of
displacement_ref.
"""
import math

import numpy as np

from displacement_ref import fractional_walk, grid_walk, read_dumps, three_groups, write_dumps  # noqa: F401

LDS_WORDS = 16128  # largest row the kernel keeps in LDS (csrc/vanhove.hip: VH_LDS_WORDS)


def _origins(n_frames, lag, stride):
    return np.arange(0, n_frames - lag, stride)


def pair_rsq(ri, rj, L):
    """ri [O,3,Na] at the origins t0, rj [O,3,Nb] at t0 + k, L [O,3] = box[t0] -> rsq [O,Na,Nb]: d = rj - ri per axis,
    one shift by L iff |d| > L/2 (strict), rsq = (dx dx + dy dy) + dz dz."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = rj[:, :, None, :] - ri[:, :, :, None]
        Lc = np.asarray(L, dtype=np.float64)[:, :, None, None]
        d = np.where(np.abs(d) > Lc / 2, d - np.sign(d) * Lc, d)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def van_hove_distinct(r, box, group_off, jobs, bin_size, n_bins, ctx=None):
    """The signature and results of backend.van_hove_distinct."""
    r = np.asarray(r, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    F = r.shape[0]
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 4)
    J = len(jobs)
    hist = np.zeros((J, n_bins), dtype=np.uint64)
    beyond = np.zeros(J, dtype=np.uint64)
    pairs = np.zeros(J, dtype=np.uint64)
    for j, (a, b, k, s) in enumerate(jobs):
        a0, a1 = int(group_off[a]), int(group_off[a + 1])
        b0, b1 = int(group_off[b]), int(group_off[b + 1])
        keep = np.ones((a1 - a0, b1 - b0), dtype=bool)
        if a == b:
            np.fill_diagonal(keep, False)
        h = np.zeros(n_bins, dtype=np.int64)
        n_beyond = n_pairs = 0
        origins = _origins(F, k, s)
        step = max(1, (1 << 21) // max(1, keep.size))  # origins per slice: bounded memory
        for c in range(0, len(origins), step):
            t0 = origins[c:c + step]
            rsq = pair_rsq(r[t0][:, :, a0:a1], r[t0 + k][:, :, b0:b1], box[t0])[:, keep]
            with np.errstate(invalid="ignore", over="ignore"):
                q = np.sqrt(rsq) / bin_size
                inside = q < n_bins  # (false for NaN and +inf)
            h += np.bincount(q[inside].astype(np.int64), minlength=n_bins)
            n_beyond += rsq.size - int(np.count_nonzero(inside))
            n_pairs += rsq.size
        hist[j], beyond[j], pairs[j] = h.astype(np.uint64), n_beyond, n_pairs
    return hist, beyond, pairs


def van_hove_distinct_loops(r, box, group_off, jobs, bin_size, n_bins):
    """The same from plain Python loops, one number at a time (small systems only) -> [(hist, beyond, pairs)]."""
    r = np.asarray(r, dtype=np.float64)
    F = r.shape[0]
    out = []
    for a, b, k, s in jobs:
        h, n_beyond, n_pairs = [0] * n_bins, 0, 0
        t0 = 0
        while t0 + k <= F - 1:
            for i in range(int(group_off[a]), int(group_off[a + 1])):
                for j in range(int(group_off[b]), int(group_off[b + 1])):
                    if j == i:
                        continue
                    n_pairs += 1
                    rsq = 0.0
                    d = [0.0, 0.0, 0.0]
                    for x in range(3):
                        dx = float(r[t0 + k, x, j]) - float(r[t0, x, i])
                        L = float(box[t0][x])
                        if abs(dx) > L / 2:
                            dx = dx - L if dx > 0 else dx + L
                        d[x] = dx
                    rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    ok = rsq == rsq and rsq != math.inf
                    bin_ = int(math.sqrt(rsq) / bin_size) if ok else n_bins
                    if bin_ < n_bins:
                        h[bin_] += 1
                    else:
                        n_beyond += 1
            t0 += s
        out.append((h, n_beyond, n_pairs))
    return out


def expected_pairs(n_frames, group_off, jobs):
    """pairs[job] = origins * (N_a N_b - (a == b ? N_a : 0)) from the formula."""
    size = np.diff(np.asarray(group_off, dtype=np.int64))
    return np.array([len(_origins(n_frames, k, s)) * (int(size[a]) * int(size[b]) - (int(size[a]) if a == b else 0))
                     for a, b, k, s in jobs], dtype=np.uint64)


# ---- the tables of Displacement.calc_van_hove_distinct -------------------------------------------------------------

def lag_frames(t, delta):
    return int(math.floor(t / delta + 0.5))


def default_pairs(atom_types):
    types = list(atom_types)
    return [(a, b) for i, a in enumerate(types) for b in types[i:]]


def distinct_tables(r, box, group_off, atom_types, pairs, lags, stride, delta, bin_size, n_bins,
                    run=van_hove_distinct):
    """({(a, b): columns}, summary columns) of Displacement.calc_van_hove_distinct for lags in frames:
    G_d[bin] = hist / ((origins N_a) rho_b shell[bin]), rho_b = N_b / mean volume of the origin frames."""
    types = list(atom_types)
    box = np.asarray(box, dtype=np.float64)
    F = r.shape[0]
    jobs = [(types.index(a), types.index(b), k, stride) for a, b in pairs for k in lags]
    hist, beyond, n_pairs = run(r, box, group_off, jobs, bin_size, n_bins)
    size = np.diff(np.asarray(group_off, dtype=np.int64))
    k_bin = np.arange(n_bins, dtype=np.float64)
    shell = 4.0 / 3.0 * math.pi * bin_size ** 3 * ((k_bin + 1.0) ** 3 - k_bin ** 3)
    volume = box[:, 0] * box[:, 1] * box[:, 2]
    gd, summary = {}, {"pair": [], "Time (ps)": [], "origins": [], "pairs": [], "beyond r_max": []}
    for p, (a, b) in enumerate(pairs):
        n_a, n_b = float(size[types.index(a)]), float(size[types.index(b)])
        cols = {"r": (k_bin + 0.5) * bin_size}
        for i, k in enumerate(lags):
            j = p * len(lags) + i
            t0 = _origins(F, k, stride)
            rho_b = n_b / np.mean(volume[t0])
            with np.errstate(invalid="ignore", divide="ignore"):
                cols[k * delta] = hist[j] / ((len(t0) * n_a) * rho_b * shell)
            summary["pair"].append("%s-%s" % (a, b))
            summary["Time (ps)"].append(k * delta)
            summary["origins"].append(len(t0))
            summary["pairs"].append(int(n_pairs[j]))
            summary["beyond r_max"].append(int(beyond[j]))
        gd[(a, b)] = cols
    return gd, summary
