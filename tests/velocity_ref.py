"""
numpy restatement of mdhip_velocity_spectrum (include/mdhip.h) and of the tables `VelocityCorrelation` makes of it
(mdproptools_amd/dynamical/velocity_correlation.py): the series coef * v, exact lag sums (int64 for integer input, long
double otherwise), a long-double direct DFT for `power`, a0 and the two documented error bounds; a synthetic trajectory
whose velocities are multiples of 1 / 1024 (the dump text round-trips exactly) and its dump writer.
"""
import os

import numpy as np

EPS52 = 2.0 ** -52
LD = np.longdouble


def default_length(n_frames):
    """The smallest power of two >= 2 * n_frames, at least 4."""
    L = 4
    while L < 2 * n_frames:
        L *= 2
    return L


def interleaved_groups(n_ent, skip=7):
    """(0, 1, 1, 0, 1, 1, ...) with every `skip`-th entity (from the fourth on) in no group."""
    g = np.where(np.arange(n_ent) % 3 == 0, 0, 1).astype(np.int32)
    g[3::skip] = -1
    return g


def series(v, coef=None):
    """s [3, E, F] = coef[e] * v[t, a, e] (one rounded multiplication), time-major. Integer arrays (v, and coef when
    given) stay int64: the products and every sum of them are then exact."""
    v = np.asarray(v)
    if np.issubdtype(v.dtype, np.integer) and (coef is None or np.issubdtype(np.asarray(coef).dtype, np.integer)):
        s = v.astype(np.int64)
        if coef is not None:
            s = s * np.asarray(coef).astype(np.int64)[None, None, :]
    else:
        s = v.astype(np.float64)
        if coef is not None:
            s = s * np.asarray(coef, dtype=np.float64)[None, None, :]
    return np.ascontiguousarray(np.transpose(s, (1, 2, 0)))


def n_groups_of(ent_group):
    g = np.asarray(ent_group)
    return max(int(g.max()) + 1, 1) if g.size else 1


def a0_truth(s, ent_group, G=None):
    """a0 [G, 4]: the sum of the squares per (group, axis) and the total; int64 for integer series, else long double."""
    G = n_groups_of(ent_group) if G is None else G
    wide = s if s.dtype == np.int64 else s.astype(LD)
    per = (wide * wide).sum(axis=2)                                        # [3, E]
    out = np.zeros((G, 4), dtype=wide.dtype)
    for g in range(G):
        out[g, :3] = per[:, np.asarray(ent_group) == g].sum(axis=1)
        out[g, 3] = out[g, :3].sum()
    return out


def lag_truth(s, ent_group, max_lag, G=None):
    """sums [max_lag+1, G, 4] by direct summation: int64 for integer series (exact), else long double."""
    G = n_groups_of(ent_group) if G is None else G
    F = s.shape[2]
    wide = s if s.dtype == np.int64 else s.astype(LD)
    members = [np.flatnonzero(np.asarray(ent_group) == g) for g in range(G)]
    out = np.zeros((max_lag + 1, G, 4), dtype=wide.dtype)
    for k in range(max_lag + 1):
        per = (wide[:, :, : F - k] * wide[:, :, k:]).sum(axis=2)           # [3, E]
        for g in range(G):
            out[k, g, :3] = per[:, members[g]].sum(axis=1)
    out[:, :, 3] = out[:, :, :3].sum(axis=2)
    return out


def power_truth(s, ent_group, L, G=None):
    """power [G, 4, L/2+1] by a long-double direct DFT (the phase index reduced mod L exactly before the cosine)."""
    G = n_groups_of(ent_group) if G is None else G
    F, K = s.shape[2], L // 2 + 1
    idx = (np.arange(K)[:, None] * np.arange(F)[None, :]) % L
    ang = (2 * np.pi * LD(1)) * idx.astype(LD) / LD(L)
    cos, sin = np.cos(ang), np.sin(ang)                                    # [K, F]
    out = np.zeros((G, 4, K), dtype=LD)
    for e, g in enumerate(np.asarray(ent_group)):
        if g < 0:
            continue
        for a in range(3):
            x = s[a, e].astype(LD)
            re, im = cos @ x, sin @ x
            out[g, a] += re * re + im * im
    out[:, 3] = out[:, :3].sum(axis=1)
    return out


def sums_bound(a0, L):
    """[G, 4]: |sums[k][g][a] - exact| <= 4 * 2^-52 * log2(L) * a0[g][a] (the header's bound), the totals column as the
    three axes: a0[g][3] is the scale of column 3."""
    # (Column 3 is (x + y) + z of the finished values: three axis errors and two roundings of at most 2^-53 * a0[g][3]
    # each could in principle add up to (1 + 1 / (4 log2 L)) of this bound; the stated bound is what is asserted.)
    return 4.0 * EPS52 * np.log2(L) * np.asarray(a0, dtype=np.float64)


def power_bound(a0, L, n_frames):
    """[G, 4]: |power - exact| <= 4 * 2^-52 * log2(L) * sqrt(n_frames) * a0, for series without a dominant line; the
    totals column as the three axes."""
    return sums_bound(a0, L) * np.sqrt(float(n_frames))


def velocity_spectrum(v, ent_group, max_lag, L=None, coef=None, want_power=False, out=None, ctx=None):
    """backend.velocity_spectrum from the exact sums, rounded to double: what the host tests put in its place."""
    v = np.asarray(v, dtype=np.float64)
    s = series(v, coef)
    G = n_groups_of(ent_group)
    L = default_length(v.shape[0]) if L is None else L
    sums = lag_truth(s, ent_group, max_lag, G).astype(np.float64)
    power = power_truth(s, ent_group, L, G).astype(np.float64) if want_power else None
    return sums, power, a0_truth(s, ent_group, G).astype(np.float64)


# ---- a small synthetic trajectory for the end-to-end tests -------------------------------------------------------------

NUM_MOLS, ATOMS_PER_MOL = [25, 15], [3, 5]
ATOM_TYPES = [[1, 2, 2], [3, 4, 3, 4, 5]]          # atom types inside a molecule of each kind: interleaved groups
MASSES = [15.9994, 1.008, 12.011, 14.0067, 32.06]   # per atom type
GRID = 1024.0  # every velocity is a multiple of 1 / GRID: the text round-trips


def synthetic_trajectory(n_frames=60, seed=11):
    """150 atoms (25 x 3 + 15 x 5) whose velocities are AR(1) series plus a molecular drift, on the grid. -> dict: steps
    [F], ids, types, mass, q [A], x [F,3,A] positions (not used by the class), v [F,3,A]."""
    rng = np.random.default_rng(seed)
    types, mol = [], []
    m = 0
    for t, (mols, per) in enumerate(zip(NUM_MOLS, ATOMS_PER_MOL)):
        for _ in range(mols):
            types += ATOM_TYPES[t]
            mol += [m] * per
            m += 1
    types, mol = np.array(types), np.array(mol)
    A = len(types)
    v = np.empty((n_frames, 3, A))
    drift = np.empty((n_frames, 3, m))
    cur, cur_m = rng.normal(size=(3, A)), rng.normal(size=(3, m))
    for f in range(n_frames):
        cur = 0.8 * cur + 0.6 * rng.normal(size=(3, A))
        cur_m = 0.95 * cur_m + 0.3 * rng.normal(size=(3, m))
        v[f], drift[f] = cur, cur_m
    v = np.rint((v + drift[:, :, mol]) * 0.01 * GRID) / GRID
    x = np.rint(rng.random((n_frames, 3, A)) * 20.0 * GRID) / GRID
    return {"steps": 500 * np.arange(n_frames), "ids": np.arange(1, A + 1), "types": types,
            "mass": np.array(MASSES)[types - 1], "q": np.where(types % 2 == 0, 0.5, -0.5), "x": x, "v": v, "mol": mol}


def write_dumps(directory, traj, frames=None, shuffle_seed=5, columns="id type mass q x y z vx vy vz", steps=None):
    """One LAMMPS dump file per frame, `vel.<timestep>.dump`, the atoms in a shuffled order; `columns`: a subset of
    id type mass q x y z vx vy vz, in that order. -> the '*' pattern that matches them."""
    rng = np.random.default_rng(shuffle_seed)
    A = len(traj["ids"])
    steps = traj["steps"] if steps is None else steps
    names = columns.split()
    for f in (range(len(traj["steps"])) if frames is None else frames):
        rows = rng.permutation(A)
        with open(os.path.join(str(directory), "vel.%d.dump" % steps[f]), "w") as fh:
            fh.write("ITEM: TIMESTEP\n%d\nITEM: NUMBER OF ATOMS\n%d\nITEM: BOX BOUNDS pp pp pp\n" % (steps[f], A))
            fh.write("0.0 20.0\n0.0 20.0\n0.0 20.0\n")
            fh.write("ITEM: ATOMS " + " ".join(names) + "\n")
            for i in rows:
                cell = {"id": "%d" % traj["ids"][i], "type": "%d" % traj["types"][i], "mass": "%.4f" % traj["mass"][i],
                        "q": "%.4f" % traj["q"][i]}
                for k, c in enumerate("xyz"):
                    cell[c] = "%.10f" % traj["x"][f, k, i]
                    cell["v" + c] = "%.10f" % traj["v"][f, k, i]
                fh.write(" ".join(cell[c] for c in names) + "\n")
    return os.path.join(str(directory), "vel.*.dump")


def com_velocities(traj):
    """(v_com [F,3,M], mol_type [M] 1-based, mol_mass [M]) in plain numpy (long double sums, rounded once)."""
    mol, mass = traj["mol"], traj["mass"].astype(LD)
    M = int(mol.max()) + 1
    out = np.empty((traj["v"].shape[0], 3, M))
    mm = np.empty(M)
    for m in range(M):
        sel = mol == m
        mm[m] = float(mass[sel].sum())
        out[:, :, m] = ((traj["v"][:, :, sel].astype(LD) * mass[sel]).sum(axis=2) / mass[sel].sum()).astype(np.float64)
    return out, np.repeat(np.arange(1, len(NUM_MOLS) + 1), NUM_MOLS), mm
