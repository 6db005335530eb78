"""
Designed residence trajectories whose shell-residence counts are known in closed form.

Each pair GROUP g sits at its own lattice site, 20 A from the next: a_g central atoms in a tight cluster (a 0.4 A
cube) at the site and b_g shell atoms in another such cluster that sits 3 A from the site in the frames where the
group's 0/1 presence pattern p_g(t) is 1 and 9 A away where it is 0. Every (central, shell) pair of the group is then
in the shell (LO, HI] = (2, 4] exactly when p_g(t) = 1; every other distance (inside a cluster, to another site) lies
well outside the shell. A per-frame jitter moves every atom without changing any hit, and the central atoms jump by
whole box lengths from frame to frame (unwrapped coordinates: their differences stay within the single wrap).

    counts[k] = sum_g a_g b_g acorr(p_g)[k],   acorr(p)[k] = sum_t p(t) p(t + k)

(twice that when both clusters form ONE atom set, the relation of a type with itself: (i, j) and (j, i) both count).
This scales to 65 535 frames and millions of pairs where oracle.cpu_ref.residence_counts (O(F^2 pairs)) cannot;
tests/test_residence_design_cpu.py checks it against that oracle at small sizes.
"""

import numpy as np

LO, HI = 2.0, 4.0  # the shell: lo < r <= hi
SPACING = 20.0  # between group sites (along x)
_CLUSTER = 0.2  # half edge of a cluster's cube
_JITTER = 0.03  # per-frame move of every atom, per axis
_IN, _OUT = np.array([3.0, 0.0, 0.0]), np.array([0.0, 0.0, 9.0])  # shell cluster's offset from the site


def acorr(p):
    """Exact integer autocorrelation sum_t p(t) p(t + k), k = 0 .. F-1, of a 0/1 series (int64). Direct below 2048
    frames; above, an FFT rounded to integers, with a check that the rounding is exact."""
    p = np.asarray(p, dtype=np.int64)
    F = len(p)
    if F <= 2048:
        return np.correlate(p, p, "full")[F - 1:].astype(np.int64)
    n = 1 << int(2 * F - 1).bit_length()
    fp = np.fft.rfft(p.astype(np.float64), n)
    c = np.fft.irfft(fp * np.conj(fp), n)[:F]
    r = np.rint(c)
    assert np.max(np.abs(c - r)) < 0.25, "FFT autocorrelation not exactly integral"
    out = r.astype(np.int64)
    assert out[0] == int(p.sum()) and out.min() >= 0
    return out


def patterns(F, seed=0):
    """The presence patterns the tests use, by name: bool [F] each."""
    rng = np.random.default_rng(seed)
    t = np.arange(F)
    run0 = F // 3
    return {
        "always": np.ones(F, bool),
        "run": (t >= run0) & (t < run0 + max(1, F // 4)),  # one run
        "periodic": (t % 7) < 3,  # on 3, off 4: a period that does not divide 64
        "random": rng.random(F) < 0.5,
        "ends": (t == 0) | (t == F - 1),  # the full span; the first and the last bit of the mask
        "never": np.zeros(F, bool),
    }


class Design:
    """xi [F,3,ni], xj [F,3,nj] (the same array when same=True), box [F,3], counts int64 [F], n_records."""

    def __init__(self, xi, xj, box, counts, n_records):
        self.xi, self.xj, self.box, self.counts, self.n_records = xi, xj, box, counts, n_records


def designed(groups, seed=0, same=False, box=None):
    """
    groups: [(pattern bool [F], a, b)], one lattice site each. same=False: the central atoms of every group form xi,
    the shell atoms xj. same=True: both clusters of every group form one set x (use with exclude_diagonal).
    box: (Lx, Ly, Lz) for every frame, at least (20 * groups, 20, 20) (the default).
    """
    F = len(groups[0][0])
    G = len(groups)
    L = np.array(box if box is not None else (SPACING * G, SPACING, SPACING), dtype=np.float64)
    assert L[0] >= SPACING * G and L[1] >= SPACING and L[2] >= SPACING
    rng = np.random.default_rng(1000 + seed)
    ca, sh = [], []
    counts = np.zeros(F, dtype=np.int64)
    n_rec = 0
    for g, (p, a, b) in enumerate(groups):
        p = np.asarray(p, dtype=bool)
        assert len(p) == F
        site = np.array([SPACING * g + 10.0, 10.0, 10.0])
        ua = site[None, :, None] + rng.uniform(-_CLUSTER, _CLUSTER, (1, 3, a))
        off = np.where(p[:, None], _IN[None, :], _OUT[None, :])  # [F,3]
        ub = site[None, :, None] + off[:, :, None] + rng.uniform(-_CLUSTER, _CLUSTER, (1, 3, b))
        ca.append(np.broadcast_to(ua, (F, 3, a)))
        sh.append(ub)
        w = (2 if same else 1) * a * b
        counts += w * acorr(p)
        n_rec += w * int(p.sum())
    xi = np.concatenate(ca, axis=2)
    xj = np.concatenate(sh, axis=2)
    xi = xi + rng.uniform(-_JITTER, _JITTER, xi.shape)
    xj = xj + rng.uniform(-_JITTER, _JITTER, xj.shape)
    # unwrapped central atoms: whole box lengths per frame and axis (-1, 0 or +1: |d| stays below 1.5 L)
    xi = xi + rng.integers(-1, 2, (F, 3, xi.shape[2])) * L[None, :, None]
    boxes = np.tile(L, (F, 1))
    if same:
        x = np.ascontiguousarray(np.concatenate([xi, xj], axis=2))
        return Design(x, x, boxes, counts, n_rec)
    return Design(np.ascontiguousarray(xi), np.ascontiguousarray(xj), boxes, counts, n_rec)


def oracle_counts(d, same=False):
    """The brute-force oracle on a design's coordinates: (counts int64 [F], n_records)."""
    from oracle import cpu_ref as O

    F = d.xi.shape[0]
    h = np.array([O.shell_indicator(d.xi[f].T, d.xj[f].T, d.box[f], LO * LO, HI * HI, same) for f in range(F)])
    return O.residence_counts(h), int(h.sum())
