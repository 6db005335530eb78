"""
numpy restatement of mdhip_self_relaxation (include/mdhip.h): the same unfused operation order in float64 and sums in
Python integers, plus a plain triple loop, the truth that the kernel's fixed-point sinc sums are held against
(math.fsum of float64 sinc terms, with the bound derived from the header's 2^-34), and the constants of the kernel's
tiles (csrc/relaxation_plan.h) that the GPU tests choose their shapes from. The reference has nothing like it, so this
restatement is the yardstick; tests/test_relaxation_cpu.py checks it against the loops.
"""
import math

import numpy as np

import displacement_ref as D

TO, TK, EB, CELLS = 32, 64, 16, 8  # origins and lags of a tile, entities of a stage, cells of a lane (rx:: constants)
UNIT = 1 << 32
GUARD = 1 << 30


def n_origins(F, k, s):
    return (F - 1 - k) // s + 1 if k <= F - 1 else 0


def sinc(x):
    """sin(x) / x in float64, 1 at 0, 0 at +inf."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))
    return np.where(np.isinf(x), 0.0, v)


def _rsq(xu, t0, k, e0, e1):
    with np.errstate(invalid="ignore", over="ignore"):
        d = xu[t0 + k][:, :, e0:e1] - xu[t0][:, :, e0:e1]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        return (dx * dx + dy * dy) + dz * dz  # [origins, entities]


def self_relaxation(r, box, group_off, max_lag, origin_stride=1, a=None, q=None, ctx=None, want_truth=False):
    """The signature and results of backend.self_relaxation. With want_truth also (truth [L,G,n_q] = math.fsum of the
    float64 sinc terms, x_max [L,G] = the largest q |dr| of a lag and group)."""
    xu, _ = D.unwrap(r, box)
    F = xu.shape[0]
    off = np.asarray(group_off, dtype=np.int64)
    G = len(off) - 1
    L = int(max_lag) + 1
    s = int(origin_stride)
    a_sq = None
    if a is not None:
        av = np.broadcast_to(np.asarray(a, dtype=np.float64), (G,))
        a_sq = av * av
    qv = np.zeros((G, 0))
    if q is not None:
        qv = np.asarray(q, dtype=np.float64)
        if qv.ndim <= 1:
            qv = np.broadcast_to(qv.reshape(-1), (G, qv.size))
    n_q = qv.shape[1]
    origins = np.array([n_origins(F, k, s) for k in range(L)], dtype=np.uint64)
    count1 = np.zeros((L, G), dtype=np.uint64)
    count2 = np.zeros((L, G), dtype=np.uint64)
    fs = np.zeros((L, G, n_q), dtype=np.int64)
    nonfinite = np.zeros((L, G), dtype=np.uint64)
    truth = np.zeros((L, G, n_q))
    x_max = np.zeros((L, G))
    for k in range(L):
        t0 = np.arange(0, F - k, s)
        for g in range(G):
            rsq = _rsq(xu, t0, k, int(off[g]), int(off[g + 1]))
            ok = np.isfinite(rsq)
            nonfinite[k, g] = int(np.count_nonzero(~ok))
            if a_sq is not None:
                with np.errstate(invalid="ignore"):
                    n = np.count_nonzero(ok & (rsq < a_sq[g]), axis=1)
                count1[k, g] = int(np.sum(n.astype(object))) if n.size else 0
                count2[k, g] = int(np.sum(n.astype(object) ** 2)) if n.size else 0
            if n_q:
                dist = np.sqrt(rsq[ok])
                for j in range(n_q):
                    x = qv[g, j] * dist
                    v = sinc(x)
                    add = np.rint(v * float(UNIT)).astype(np.int64).astype(object)
                    fs[k, g, j] = int(np.sum(add)) if add.size else 0
                    truth[k, g, j] = math.fsum(v)
                    x_max[k, g] = max(x_max[k, g], float(x.max()) if x.size else 0.0)
    out = (origins, count1, count2, fs, nonfinite)
    return out + (truth, x_max) if want_truth else out


def self_relaxation_loops(r, box, group_off, max_lag, origin_stride=1, a=None, q=None):
    """The same from plain Python loops, one number at a time (small systems only): lists [k][g] of
    (origins, count1, count2, [fs_j], nonfinite)."""
    r = np.asarray(r, dtype=np.float64)
    F, _, E = r.shape
    xu = [[[float(r[f, c, e]) for e in range(E)] for c in range(3)] for f in range(F)]
    if box is not None:
        for c in range(3):
            for e in range(E):
                n = 0
                for f in range(1, F):
                    d = float(r[f, c, e]) - float(r[f - 1, c, e])
                    edge = float(box[f][c])
                    if d > edge / 2:
                        n -= 1
                    elif d < -edge / 2:
                        n += 1
                    xu[f][c][e] = float(r[f, c, e]) + float(n) * edge
    G = len(group_off) - 1
    av = None if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (G,))
    qq = np.zeros((G, 0))
    if q is not None:
        qq = np.asarray(q, dtype=np.float64)
        if qq.ndim <= 1:
            qq = np.broadcast_to(qq.reshape(-1), (G, qq.size))
    out = []
    for k in range(max_lag + 1):
        row = []
        for g in range(G):
            ag = None if av is None else float(av[g])
            qg = [float(v) for v in qq[g]]
            n_orig = c1 = c2 = bad = 0
            fsum = [0] * len(qg)
            t0 = 0
            while t0 + k <= F - 1:
                n_orig += 1
                n = 0
                for e in range(int(group_off[g]), int(group_off[g + 1])):
                    dx, dy, dz = (xu[t0 + k][c][e] - xu[t0][c][e] for c in range(3))
                    rsq = (dx * dx + dy * dy) + dz * dz
                    if rsq != rsq or rsq == math.inf:
                        bad += 1
                        continue
                    if ag is not None and rsq < ag * ag:
                        n += 1
                    for j, qj in enumerate(qg):
                        x = qj * math.sqrt(rsq)
                        v = 1.0 if x == 0.0 else (0.0 if x == math.inf else math.sin(x) / x)
                        fsum[j] += int(np.rint(v * float(UNIT)))
                c1 += n
                c2 += n * n
                t0 += origin_stride
            row.append((n_orig, c1, c2, fsum, bad))
        out.append(row)
    return out


def fs_bound(origins, sizes, x_max):
    """|fs / 2^32 - truth| <= W (2^-33 + 2^-34) + W x_max 2^-52 per (lag, group): the fixed-point rounding of every
    addend (half a unit), the 2^-34 the header allows the kernel's sinc, and the rounding of x = q * sqrt(rsq) (two
    roundings, 2^-52 relative, through |sinc'| <= 1/2 — and as much again for the float64 sine of the truth)."""
    w = origins.astype(np.float64)[:, None] * np.asarray(sizes, dtype=np.float64)[None, :]
    return w * (2.0 ** -33 + 2.0 ** -34) + w * x_max * 2.0 ** -52


def tables(r, box, group_off, atom_types, delta, max_lag, origin_stride, a, q):
    """The columns of StructuralRelaxation.calc_relaxation from the restatement: a {type: number} or None, q
    {type: [numbers]} or None."""
    G = len(atom_types)
    av = None if a is None else [a[t] for t in atom_types]
    qv = None if q is None else [q[t] for t in atom_types]
    origins, c1, c2, fs, _ = self_relaxation(r, box, group_off, max_lag, origin_stride, av, qv)
    cols = {"Time (ps)": np.arange(max_lag + 1) * delta, "origins": origins.astype(np.int64)}
    o = origins.astype(np.float64)
    for g in range(G):
        t = atom_types[g]
        n = int(group_off[g + 1] - group_off[g])
        w = o * float(n)
        if qv is not None:
            for j, qj in enumerate(qv[g]):
                cols["Fs_%s_q%g" % (t, qj)] = fs[:, g, j].astype(np.float64) / float(UNIT) / w
        if av is not None:
            cols["Q_%s" % t] = c1[:, g].astype(np.float64) / w
            chi = []
            for k in range(max_lag + 1):
                O, a1, a2 = int(origins[k]), int(c1[k, g]), int(c2[k, g])
                chi.append((O * a2 - a1 * a1) / (O * O * n) if O > 1 and n else 0.0)
            cols["chi4_%s" % t] = np.array(chi)
    return cols
