"""
numpy restatement of mdhip_free_volume (include/mdhip.h), operation by operation as the header states them; no GPU and
no torch. Brute force: every grid point against every atom, no cells — the cell grid of the library is an organisation
of the work, not part of the specification, so agreeing with this is agreeing that the cells lose nothing.

numpy never fuses a product into a sum and its sqrt and division are correctly rounded, so the library's counts can be
compared with `==` and its field bit for bit. Shared by tests/test_free_volume_cpu.py and tests/test_gpu_free_volume.py.
"""
import numpy as np

MAX_NC, MARGIN, BRICK, CHUNK = 64, 2.0 ** -20, 1024, 1024  # csrc/cell_plan.h, csrc/free_volume.hip
LDS_CELLS = 6144


def wrapped(x, L):
    """xw of a coordinate: s = x / L; f = s - floor(s); f = f < 1 ? f : 0; xw = f * L."""
    s = x / L
    f = s - np.floor(s)
    f = np.where(f < 1.0, f, 0.0)
    return f * L


def points(g, L):
    """p [G,3] of the grid g = (gx, gy, gz) in a frame of edges L [3]; point (i, j, k) at (i * gy + j) * gz + k."""
    axes = [((np.arange(g[a], dtype=np.float64) + 0.5) / float(g[a])) * float(L[a]) for a in range(3)]
    p = np.empty((g[0], g[1], g[2], 3))
    p[..., 0], p[..., 1], p[..., 2] = axes[0][:, None, None], axes[1][None, :, None], axes[2][None, None, :]
    return p.reshape(-1, 3)


def field(xyz, box, atom_class, radius, grid, r_search, chunk_cells=1_000_000):
    """(s [F,G] float64, nearest [F,G] int32) of the header."""
    xyz, box = np.asarray(xyz, dtype=np.float64), np.asarray(box, dtype=np.float64)
    cls, radius = np.asarray(atom_class, dtype=np.int64), np.asarray(radius, dtype=np.float64)
    F, _, N = xyz.shape
    g = [int(v) for v in grid]
    G = g[0] * g[1] * g[2]
    rs2 = float(r_search) * float(r_search)
    s_all, near_all = np.full((F, G), np.inf), np.full((F, G), -1, dtype=np.int32)
    step = max(1, chunk_cells // max(G, 1))
    for f in range(F):
        L = box[f]
        seen = (cls >= 0) & np.isfinite(xyz[f]).all(axis=0)
        who = np.nonzero(seen)[0]                       # ascending atom index
        if not len(who):
            continue
        with np.errstate(all="ignore"):
            xw = np.stack([wrapped(xyz[f, a, who], L[a]) for a in range(3)])
        R = radius[cls[who]]
        p = points(g, L)
        best, near = s_all[f], near_all[f]
        for a0 in range(0, len(who), step):
            sl = slice(a0, a0 + step)
            rsq = None
            d2 = []
            for a in range(3):
                d = np.abs(p[:, a, None] - xw[a, None, sl])
                d = np.minimum(d, np.abs(d - L[a]))
                d2.append(d * d)
            rsq = (d2[0] + d2[1]) + d2[2]
            sj = np.where(rsq < rs2, np.sqrt(rsq) - R[None, sl], np.inf)
            k = np.argmin(sj, axis=1)                    # the first (lowest index) of the chunk's minima
            m = sj[np.arange(G), k]
            better = m < best                            # strict: an earlier chunk's (lower) index stays at a tie
            best[better] = m[better]
            near[better] = who[sl][k[better]]
    return s_all, near_all


def counts(s, nearest, atom_class, n_classes, edges, probe, grid):
    """The header's counts from the field: dict of hist uint64 [C,nbins], occupied uint64 [C], beyond int, n_free int64
    [F,P], free_map uint32 [gx,gy,gz]."""
    cls, edges, probe = np.asarray(atom_class, dtype=np.int64), np.asarray(edges, dtype=np.float64), np.asarray(probe, dtype=np.float64)
    nb = len(edges) - 1
    hist, occupied = np.zeros((n_classes, nb), dtype=np.uint64), np.zeros(n_classes, dtype=np.uint64)
    none = nearest < 0
    lining = np.where(none, 0, cls[np.maximum(nearest, 0)])
    occ = ~none & (s < 0)
    binned = ~none & (s >= 0) & (s < edges[nb])
    b = np.searchsorted(edges, s[binned], side="right") - 1   # edges[b] <= s < edges[b+1], by comparison
    np.add.at(hist, (lining[binned], b), 1)
    np.add.at(occupied, lining[occ], 1)
    free = none[:, :, None] | (s[:, :, None] >= probe[None, None, :])
    return {"hist": hist, "occupied": occupied, "beyond": int(s.size - int(occ.sum()) - int(binned.sum())),
            "n_free": free.sum(axis=1).astype(np.int64),
            "free_map": free[:, :, 0].sum(axis=0).astype(np.uint32).reshape(tuple(int(v) for v in grid))}


def free_volume(xyz, box, atom_class, radius, grid, r_search, edges, probe=(0.0,)):
    """Everything backend.free_volume returns, with "s" [F,gx,gy,gz] and "nearest"."""
    s, near = field(xyz, box, atom_class, radius, grid, r_search)
    out = counts(s, near, atom_class, len(np.atleast_1d(radius)), edges, probe, grid)
    shape = (s.shape[0],) + tuple(int(v) for v in grid)
    out["s"], out["nearest"] = s.reshape(shape), near.reshape(shape)
    return out


def cells(L, r_search):
    """nc of csrc/cell_plan.h (cp_cells) for one edge."""
    need = float(r_search) * (1.0 + MARGIN)
    q = L / need
    nc = MAX_NC if q >= MAX_NC else (int(q) if q >= 1.0 else 1)
    while nc > 1 and not L / nc >= need:
        nc -= 1
    while nc < MAX_NC and L / (nc + 1) >= need:
        nc += 1
    return nc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
