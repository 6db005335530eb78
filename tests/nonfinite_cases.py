"""
Non-finite input ("NaN stays home"): the poison patterns and placements shared by tests/test_nonfinite_cpu.py and
tests/test_gpu_nonfinite.py. Data builders only — no kernel, no oracle.

A dump of a run that blew up holds `nan`, `-nan` and `inf`; the reader passes them on and nothing refuses them. The
reference's answer is defined all the same (include/mdhip.h, "Non-finite input"):
  * pair counts: a pair with a non-finite difference on any axis is in no cutoff, every other pair counts as before —
    the integers of the frame are those of the frame with the poisoned atoms DELETED;
  * sums: the value enters exactly the sums it enters in plain numpy, and no others.
"""
import numpy as np

NAN, INF, HUGE = float("nan"), float("inf"), 1.0e300

# name -> the values written over (x, y, z) of every poisoned atom (None: the coordinate stays)
PATTERNS = {
    "nan_one_axis": (None, NAN, None),
    "nan_all_axes": (NAN, NAN, NAN),
    "plus_inf": (INF, None, None),
    "minus_inf": (None, None, -INF),
    "two_plus_inf": (None, INF, None),  # on two atoms of the frame: their difference on y is inf - inf = NaN
    "huge_finite": (HUGE, None, None),  # finite, but every difference with it overflows rsq to +inf
}
PATTERN_NAMES = tuple(PATTERNS)


def places(n):
    """Atom indices to poison: the first and last atom, both sides of a 64-atom wave and of a 256-atom tile."""
    return tuple(sorted({p for p in (0, 63, 64, 255, 256, n - 1) if 0 <= p < n}))


def atoms_of(pattern, place, n):
    """The atoms pattern `pattern` poisons when placed at `place`: that atom, and for "two_plus_inf" a second one half
    the frame further on."""
    if pattern == "two_plus_inf":
        return (place, (place + n // 2) % n)
    return (place,)


def poison(x, pattern, atoms):
    """x [3, n] is not touched; returns a copy with `pattern` written over `atoms`."""
    y = np.array(x, dtype=np.float64, copy=True)
    for ax, v in enumerate(PATTERNS[pattern]):
        if v is not None:
            y[ax, list(atoms)] = v
    return y


def delete(x, types, atoms):
    """The frame without `atoms`: (x [3, n - k], types [n - k])."""
    keep = np.ones(x.shape[1], dtype=bool)
    keep[list(atoms)] = False
    return np.ascontiguousarray(x[:, keep]), np.ascontiguousarray(np.asarray(types)[keep])


def schedule(n, n_frames, every_combination=False):
    """Which (pattern, atoms) each frame of a trajectory gets; frame 0 stays clean. every_combination: all patterns x all
    placements (n_frames is ignored); otherwise frame f takes pattern (f - 1) mod 6 and the placements in turn, so that
    1 + 6 k frames give every pattern k placements."""
    pl = places(n)
    out = [None]
    if every_combination:
        for p in PATTERN_NAMES:
            for q in pl:
                out.append((p, atoms_of(p, q, n)))
        return out
    for f in range(1, n_frames):
        p = PATTERN_NAMES[(f - 1) % len(PATTERN_NAMES)]
        q = pl[((f - 1) // len(PATTERN_NAMES) + (f - 1)) % len(pl)]
        out.append((p, atoms_of(p, q, n)))
    return out


def trajectory(clean, plan):
    """clean [F, 3, n], plan = one (pattern, atoms) or None per frame (schedule(); any tuple of atoms will do, places(n)
    for a frame poisoned at every placement) -> the poisoned copy [F, 3, n]."""
    out = np.array(clean, dtype=np.float64, copy=True)
    for f, entry in enumerate(plan):
        if entry is not None:
            out[f] = poison(clean[f], entry[0], entry[1])
    return out


def uniform_frames(seed, n_frames, n, box):
    """n atoms uniform in the cell [0, L) of every frame: [F, 3, n]."""
    rng = np.random.default_rng(seed)
    L = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
    return rng.uniform(0.0, 1.0, (n_frames, 3, n)) * L[None, :, None]


def k1024(rng, shape, k=40):
    """Exact data: k / 1024 with |k| <= `k` — sums of such values and of their products are exact in float64, so that
    "bit-identical" does not depend on the order of a summation."""
    return rng.integers(-k, k + 1, shape).astype(np.float64) / 1024.0


def group_sums_direct(v, go):
    """v [..., E] -> [..., G]: every group summed on its own (np.sum over its slice; an empty group gives 0). Prefix
    differences would carry a NaN into every later group."""
    go = np.asarray(go)
    return np.stack([v[..., go[g]:go[g + 1]].sum(axis=-1) for g in range(len(go) - 1)], axis=-1)


def same_bits(a, b):
    """Equal element by element with NaN == NaN (payload and sign of a NaN are not compared) and -0.0 == 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# The tokens a blown-up run writes, as the C library prints them, and what they must parse to
DUMP_TOKENS = (("nan", NAN), ("-nan", NAN), ("inf", INF), ("-inf", -INF), ("NaN", NAN), ("Inf", INF))
