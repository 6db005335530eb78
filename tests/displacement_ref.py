"""
numpy restatement of mdhip_displacement_hist (include/mdhip.h) and of the tables Displacement builds from it, the
system builders of the displacement tests and a writer of small text dumps. The reference's Displacement.calc_dist
returns nothing (dynamical/residence_time.py:211-254), so there is no golden: this restatement is the yardstick, and
tests/test_displacement_cpu.py checks it against a plain Python loop and against a true unwrapped walk.
"""
import math
import os

import numpy as np

CHUNK = 64       # frames per chunk of the kernel's image-count passes (csrc/displacement.hip: DP_CHUNK)
LDS_WORDS = 16128  # largest row the kernel keeps in LDS (DP_LDS_WORDS)


def image_counts(x, box):
    """x [F,3,E] wrapped, box [F,3] -> (n int64 [F,3,E], crossings)."""
    x = np.asarray(x, dtype=np.float64)
    L = np.asarray(box, dtype=np.float64)[1:, :, None]
    with np.errstate(invalid="ignore"):
        d = x[1:] - x[:-1]
        shift = np.where(d > L / 2, -1, 0) + np.where(d < -L / 2, 1, 0)
    n = np.zeros(x.shape, dtype=np.int64)
    n[1:] = np.cumsum(shift, axis=0)
    return n, int(np.count_nonzero(shift))


def unwrap(x, box):
    """-> (xu [F,3,E], crossings); box None: x itself."""
    x = np.asarray(x, dtype=np.float64)
    if box is None:
        return x, 0
    n, crossings = image_counts(x, box)
    prod = n.astype(np.float64) * np.asarray(box, dtype=np.float64)[:, :, None]
    return x + prod, crossings


def displacement_hist(r, box, group_off, jobs, bin_size, n_bins, ctx=None):
    """The signature and results of backend.displacement_hist."""
    xu, crossings = unwrap(r, box)
    F = xu.shape[0]
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 3)
    J = len(jobs)
    hist = np.zeros((J, n_bins), dtype=np.uint64)
    overflow = np.zeros(J, dtype=np.uint64)
    windows = np.zeros(J, dtype=np.uint64)
    moments = np.zeros((J, 3), dtype=np.float64)
    for j, (g, k, s) in enumerate(jobs):
        e0, e1 = int(group_off[g]), int(group_off[g + 1])
        t0 = np.arange(0, F - k, s)
        d = xu[t0 + k][:, :, e0:e1] - xu[t0][:, :, e0:e1]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        rsq = ((dx * dx + dy * dy) + dz * dz).ravel()
        with np.errstate(invalid="ignore", over="ignore"):
            dist = np.sqrt(rsq)
            q = dist / bin_size
            inside = q < n_bins  # (false for NaN)
            bins = q[inside].astype(np.int64)
            hist[j] = np.bincount(bins, minlength=n_bins).astype(np.uint64)
            overflow[j] = rsq.size - bins.size
            windows[j] = rsq.size
            moments[j] = np.sum(dist), np.sum(rsq), np.sum(rsq * rsq)
    return hist, overflow, windows, moments, crossings


def displacement_hist_loops(r, box, group_off, jobs, bin_size, n_bins):
    """The same from plain Python loops, one number at a time (small systems only)."""
    r = np.asarray(r, dtype=np.float64)
    F, _, E = r.shape
    xu = [[[float(r[f, a, e]) for e in range(E)] for a in range(3)] for f in range(F)]
    crossings = 0
    if box is not None:
        for a in range(3):
            for e in range(E):
                n = 0
                for f in range(1, F):
                    d = float(r[f, a, e]) - float(r[f - 1, a, e])
                    L = float(box[f][a])
                    if d > L / 2:
                        n -= 1
                        crossings += 1
                    elif d < -L / 2:
                        n += 1
                        crossings += 1
                    xu[f][a][e] = float(r[f, a, e]) + float(n) * L
    out = []
    for g, k, s in jobs:
        h, ovf, win, m = [0] * n_bins, 0, 0, [0.0, 0.0, 0.0]
        t0 = 0
        while t0 + k <= F - 1:
            for e in range(int(group_off[g]), int(group_off[g + 1])):
                dx, dy, dz = (xu[t0 + k][a][e] - xu[t0][a][e] for a in range(3))
                rsq = (dx * dx + dy * dy) + dz * dz
                win += 1
                m[0] += math.sqrt(rsq) if rsq == rsq else rsq
                m[1] += rsq
                m[2] += rsq * rsq
                b = int(math.sqrt(rsq) / bin_size) if rsq == rsq and rsq != math.inf else n_bins
                if b < n_bins:
                    h[b] += 1
                else:
                    ovf += 1
            t0 += s
        out.append((h, ovf, win, m))
    return out, crossings


# ---- systems ----------------------------------------------------------------------------------------------------

def grid_walk(seed, n_frames, n_ent, max_step=0.45, vary_box=True):
    """Wrapped coordinates on a 2^-10 grid: a walk with steps up to `max_step` box edges per frame, so that atoms
    cross the faces several times in both directions; the box changes every frame (by multiples of 2^-10).
    -> (x [F,3,E], box [F,3])"""
    rng = np.random.default_rng(seed)
    base = np.array([8.0, 9.5, 11.25])
    box = np.tile(base, (n_frames, 1))
    if vary_box:
        box = box + rng.integers(-64, 65, size=(n_frames, 3)) / 1024.0
    lim = (max_step * base * 1024).astype(np.int64)
    steps = np.stack([rng.integers(-lim[a], lim[a] + 1, size=(n_frames, n_ent)) for a in range(3)], axis=1)
    steps[0] = np.stack([rng.integers(0, int(base[a] * 1024), size=n_ent) for a in range(3)])
    u = np.cumsum(steps, axis=0) / 1024.0
    return np.ascontiguousarray(np.mod(u, box[:, :, None])), box


def three_groups(n_ent):
    """Three contiguous groups of which the middle one is empty."""
    a = n_ent // 3
    return np.array([0, a, a, n_ent], dtype=np.int64)


def fractional_walk(seed, n_frames, n_ent, max_step=0.2):
    """A true unwrapped walk in fractional coordinates s (steps below `max_step` box edges), in a box that changes by
    up to 1 % per frame. -> (x wrapped [F,3,E], box [F,3], xu true [F,3,E]); s(0) is in [0, 1)."""
    rng = np.random.default_rng(seed)
    s = np.cumsum(rng.uniform(-max_step, max_step, size=(n_frames, 3, n_ent)), axis=0)
    s = s - s[0] + rng.uniform(0.0, 1.0, size=(3, n_ent))
    box = np.array([20.0, 25.0, 30.0]) * (1.0 + 0.01 * np.sin(0.3 * np.arange(n_frames)))[:, None]
    x = (s - np.floor(s)) * box[:, :, None]
    return x, box, s * box[:, :, None]


# ---- dumps ------------------------------------------------------------------------------------------------------

def write_dumps(path, x, xu, box, types, step=100):
    """One text dump per frame, dump.<timestep>.lammpstrj, columns id type x y z xu yu zu; atoms in shuffled order.
    -> the pattern."""
    from mdproptools_amd import io as mio

    rng = np.random.default_rng(5)
    n = x.shape[2]
    for f in range(x.shape[0]):
        order = rng.permutation(n)
        table = np.column_stack([np.arange(1, n + 1), types, x[f].T, xu[f].T])[order]
        bounds = [(0.0, float(box[f, a])) for a in range(3)]
        mio.write_dump(os.path.join(path, "dump.%d.lammpstrj" % (f * step)), f * step, bounds,
                       ["id", "type", "x", "y", "z", "xu", "yu", "zu"], table)
    return os.path.join(path, "dump.*.lammpstrj")


def read_dumps(pattern, atom_types, cols):
    """What Displacement hands the library: (r [F,3,E] grouped by type, box [F,3], group_off, timesteps)."""
    from mdproptools_amd import io as mio

    planes, boxes, steps = [], [], []
    for ts, bounds, _, _, pl in mio.iter_native_frames(pattern, ["id", "type"] + list(cols), sort_by="id"):
        groups = [np.flatnonzero(pl[1] == t) for t in atom_types]
        planes.append(pl[2:5][:, np.concatenate(groups)])
        b = np.asarray(bounds, dtype=np.float64)
        boxes.append(b[:, 1] - b[:, 0])
        steps.append(int(ts))
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return np.ascontiguousarray(np.stack(planes)), np.stack(boxes), off, steps


# ---- the tables of Displacement ---------------------------------------------------------------------------------

def lag_frames(tau, delta):
    return max(1, int(math.floor(tau / delta + 0.5)))


def alpha2(moments, windows):
    w = windows.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 3.0 * (moments[:, 2] / w) / (5.0 * (moments[:, 1] / w) ** 2) - 1.0


def dist_tables(r, box, group_off, atom_types, residence_time, delta, bin_size, n_bins, overlap):
    """(dist_df, hist_df) of Displacement.calc_dist as dicts of columns."""
    lags = [lag_frames(residence_time[t], delta) for t in atom_types]
    jobs = [(g, k, 1 if overlap else k) for g, k in enumerate(lags)]
    hist, overflow, windows, moments, _ = displacement_hist(r, box, group_off, jobs, bin_size, n_bins)
    w = windows.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = {"type": list(atom_types), "residence time (ps)": [residence_time[t] for t in atom_types],
                "lag (frames)": lags, "windows": windows.astype(np.int64), "mean distance": moments[:, 0] / w,
                "rms distance": np.sqrt(moments[:, 1] / w), "alpha2": alpha2(moments, windows),
                "beyond r_max": overflow.astype(np.int64)}
        cols = {"r": (np.arange(n_bins) + 0.5) * bin_size}
        for g, t in enumerate(atom_types):
            cols[t] = hist[g] / (w[g] * bin_size)
    return dist, cols


def van_hove_tables(r, box, group_off, atom_types, lags, delta, bin_size, n_bins):
    """(gs {type: columns}, alpha2 columns) of Displacement.calc_van_hove for lags in frames."""
    jobs = [(g, k, 1) for g in range(len(atom_types)) for k in lags]
    hist, _, windows, moments, _ = displacement_hist(r, box, group_off, jobs, bin_size, n_bins)
    w = windows.astype(np.float64)
    a2 = alpha2(moments, windows)
    n = len(lags)
    gs, al = {}, {"Time (ps)": [k * delta for k in lags]}
    for g, t in enumerate(atom_types):
        cols = {"r": (np.arange(n_bins) + 0.5) * bin_size}
        for i, k in enumerate(lags):
            cols[k * delta] = hist[g * n + i] / (w[g * n + i] * bin_size)
        gs[t] = cols
        al[t] = a2[g * n:(g + 1) * n]
    return gs, al


def moments_close(got, want, windows):
    """|got - want| <= windows * 2^-52 * |want| per entry (the terms are identical non-negative doubles, so two
    summation orders differ by at most 2 (n - 1) 2^-53 relative); NaN must match NaN."""
    got, want = np.asarray(got), np.asarray(want)
    tol = windows.astype(np.float64)[:, None] * 2.0 ** -52 * np.abs(want)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= tol[~nan]))
