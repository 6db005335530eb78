"""
Plain-numpy restatement of the contact components (aggregates): the test oracle of
backend.contact_components and structural/aggregates.py.

- rsq(i, j): per axis a = |x_i - x_j|, min(a, |a - L|) (the |d| form of the single wrap), (ax*ax + ay*ay) + az*az,
  unfused doubles (the rsq of tests/angular_ref.py);
- position p of list A and position q of list B are in contact when node_of[A[p]] != node_of[B[q]] and
  rsq < rsq_cut[class_a[p], class_b[q]] (strict; an entry <= 0 never links);
- every contact unites the two nodes in a serial union-find; label = the smallest member of the component.

`contact_components` walks A x B (one A atom at a time, vectorised over the frames and B) and then the contacts one by
one. `census` restates the host tables of calc_aggregates with dictionaries. Below them: the builders of the test
systems.
"""

from collections import Counter

import numpy as np

from angular_ref import _wrap_abs, simple_cubic, write_dumps  # noqa: F401  (write_dumps: for the tests)


def contact_components(xyz, box, atoms_a, class_a, atoms_b, class_b, rsq_cut, node_of, n_nodes):
    """-> (label int64 [F, n_nodes], n_components int64 [F], n_contacts int64 [F]) as backend.contact_components."""
    xyz = np.asarray(xyz, dtype=np.float64)
    F = len(xyz)
    L = np.asarray(box, dtype=np.float64).reshape(F, 3)
    atoms_a, atoms_b = np.asarray(atoms_a, dtype=np.int64), np.asarray(atoms_b, dtype=np.int64)
    class_a, class_b = np.asarray(class_a, dtype=np.int64), np.asarray(class_b, dtype=np.int64)
    cut = np.asarray(rsq_cut, dtype=np.float64)
    node_of = np.asarray(node_of, dtype=np.int64)
    parent = np.tile(np.arange(n_nodes), (F, 1))
    n_contacts = np.zeros(F, dtype=np.int64)

    def find(row, x):
        while row[x] != x:
            row[x] = row[row[x]]
            x = row[x]
        return x

    nb = node_of[atoms_b]
    for p, i in enumerate(atoms_a):
        if not len(atoms_b):
            break
        ax = [_wrap_abs(xyz[:, k, i, None] - xyz[:, k, atoms_b], L[:, k, None]) for k in range(3)]
        rsq = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]  # [F, n_b]
        hit = (rsq < cut[class_a[p]][class_b][None, :]) & (nb != node_of[i])[None, :]
        for f, q in zip(*np.nonzero(hit)):
            n_contacts[f] += 1
            row = parent[f]
            ra, rb = find(row, node_of[i]), find(row, nb[q])
            if ra != rb:
                row[max(ra, rb)] = min(ra, rb)
    label = np.empty((F, n_nodes), dtype=np.int64)
    for f in range(F):
        row = parent[f]
        if np.array_equal(row, np.arange(n_nodes)):
            label[f] = row
            continue
        for m in range(n_nodes):  # (roots only ever hang under smaller ones: the root is the smallest member)
            label[f, m] = find(row, m)
    return label, (label == np.arange(n_nodes)[None, :]).sum(axis=1), n_contacts


def census(labels, node_type, steps=None, n_contacts=None):
    """(rows, sizes, per_frame) of calc_aggregates from labels [F, n]: rows = [(composition tuple over the sorted node
    types, n_aggregates)] in the census order, sizes = {size: n_aggregates}, per_frame = [(step, n_aggregates,
    largest, n_contacts)]."""
    labels = np.asarray(labels)
    tids = sorted(set(int(t) for t in node_type))
    comps, sizes, per = Counter(), Counter(), []
    for f, row in enumerate(labels):
        members = {}
        for m, lab in enumerate(row):
            members.setdefault(int(lab), []).append(int(node_type[m]))
        for mem in members.values():
            comps[tuple(mem.count(t) for t in tids)] += 1
            sizes[len(mem)] += 1
        per.append((int(steps[f]) if steps is not None else f, len(members), max(len(m) for m in members.values()),
                    int(n_contacts[f]) if n_contacts is not None else 0))
    rows = sorted(comps.items(), key=lambda kv: (-kv[1], kv[0]))
    return rows, dict(sizes), per


def all_atoms(n):
    """(atoms_a, class_a, atoms_b, class_b, node_of, n_nodes): every atom a node of its own, listed on both sides."""
    idx = np.arange(n)
    return idx, np.zeros(n, dtype=np.int64), idx, np.zeros(n, dtype=np.int64), idx, n


def lists(types, contacts):
    """(atoms_a, class_a, atoms_b, class_b, rsq_cut) of contacts [(type_a, type_b, r_cut), ...]: list A holds the atoms
    of every type_a, list B those of every type_b, the classes are the ranks of the types, a pair that no contact names
    has the table entry 0."""
    types = np.asarray(types)
    ta, tb = sorted({c[0] for c in contacts}), sorted({c[1] for c in contacts})
    cut = np.zeros((len(ta), len(tb)))
    for a, b, r in contacts:
        cut[ta.index(a), tb.index(b)] = float(r) ** 2
    aa, ab = np.flatnonzero(np.isin(types, ta)), np.flatnonzero(np.isin(types, tb))
    return aa, np.searchsorted(ta, types[aa]), ab, np.searchsorted(tb, types[ab]), cut


# ---- systems with closed-form components ----

def line(M=12, spacing=2.0, seed=0, cut=()):
    """(xyz [1, 3, M - len(cut)], box [1, 3]): atoms on a line along x, `spacing` apart, the box M * spacing long (a
    ring through the boundary), atom indices a seeded shuffle of the positions; the positions in `cut` are left out."""
    pos = np.array([k for k in range(M) if k not in cut])
    order = np.random.default_rng(seed).permutation(len(pos))
    xyz = np.ones((1, 3, len(pos)))
    xyz[0, 0, order] = pos * float(spacing)
    return xyz, np.full((1, 3), M * float(spacing))


def path(n, spacing=1.0, seed=0, split=False):
    """A path of n nodes along x whose indices are a seeded permutation of their positions, in a box too long to close
    it: (xyz [1, 3, n], box [1, 3], parity [n] of every atom's position). split: the odd positions sit on a second
    line half a spacing above the even ones, and consecutive positions of one parity are `spacing` apart — with the
    classes = parity and cutoffs only on the diagonal, two chains within reach of each other that never link."""
    perm = np.random.default_rng(seed).permutation(n)
    k = np.arange(n)
    xyz = np.ones((1, 3, n))
    if split:
        xyz[0, 0, perm] = (k // 2) * float(spacing)
        xyz[0, 1, perm] = 1.0 + 0.5 * spacing * (k % 2)
    else:
        xyz[0, 0, perm] = k * float(spacing)
    parity = np.empty(n, dtype=np.int64)
    parity[perm] = k % 2
    return xyz, np.array([[(n + 10) * float(spacing), 50.0, 50.0]]), parity


def ball(rng, centre, k, r):
    """k points within r of `centre`, 3 decimals."""
    p = rng.normal(size=(3, k))
    p = p / np.linalg.norm(p, axis=0) * (r * rng.uniform(0.2, 0.95, k))
    return np.round(np.asarray(centre)[:, None] + p, 3)


def contention(n_a=64, n_b=512, seed=0):
    """n_a A atoms and n_b B atoms inside one ball of radius 1 (every pair closer than 2.5 wraps nothing in the box of
    40) and one far B atom: (xyz [1, 3, n_a + n_b + 1], box, atoms_a, atoms_b)."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([ball(rng, [20.0] * 3, n_a + n_b, 1.0), np.full((3, 1), 35.0)], axis=1)[None]
    return xyz, np.full((1, 3), 40.0), np.arange(n_a), np.arange(n_a, n_a + n_b + 1)


def bridge_system():
    """(xyz [1, 3, 14], box [1, 3]) for the layout num_mols [2, 3, 2], num_atoms_per_mol [1, 2, 3]: 2 cations (altered
    atom type 1), 3 anions (types 2, 3), 2 solvent molecules (types 4, 5, 6). Anion 0 bridges the two cations through
    its two atoms (each 1.0 from one cation); the two atoms of anion 1 are 0.5 from each other and far from the rest;
    anion 2 and the solvent are far from everything."""
    pos = [[10.0, 10.0, 10.0], [14.0, 10.0, 10.0],                      # cations 0, 1
           [11.0, 10.0, 10.0], [13.0, 10.0, 10.0],                      # anion 0
           [20.0, 20.0, 20.0], [20.5, 20.0, 20.0],                      # anion 1
           [25.0, 5.0, 5.0], [25.0, 9.0, 5.0],                          # anion 2
           [30.0, 30.0, 30.0], [35.0, 30.0, 30.0], [40.0, 30.0, 30.0],  # the solvent
           [30.0, 35.0, 30.0], [35.0, 35.0, 30.0], [40.0, 35.0, 30.0]]
    return np.array(pos).T[None], np.full((1, 3), 50.0)


def edge_system(seed, n, n_frames=2):
    """Types 1, 2, 3 in turn (atoms 3 i, 3 i + 1, 3 i + 2); frame 0 carries the edges of the arithmetic for the
    contact (1, 2, 3.5) in the box 12 x 9 x 6; the box differs per frame."""
    rng = np.random.default_rng(seed)
    box = np.array([[12.0, 9.0, 6.0], [12.5, 9.25, 6.5], [11.75, 9.5, 6.25]])[:n_frames]
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * np.array([11.5, 8.9, 5.9])[None, :, None], 3)
    types = np.arange(n) % 3 + 1
    c = lambda i: 3 * i        # noqa: E731  (the i-th atom of type 1)
    a = lambda i: 3 * i + 1    # noqa: E731  (the i-th atom of type 2)
    f = xyz[0]
    f[:, c(0)], f[:, a(0)] = [5.0, 5.0, 2.0], [8.5, 5.0, 2.0]          # exactly r_cut: no link
    f[:, c(1)], f[:, a(1)] = [4.0, 4.0, 1.0], [4.0, 4.5, 4.0]          # d_z == +L/2
    f[:, c(2)], f[:, a(2)] = [9.0, 4.0, 5.0], [9.5, 4.0, 2.0]          # d_z == -L/2
    f[:, c(3)] = [0.2, 0.3, 0.1]                                       # links across each of the three boundaries
    f[:, a(3)], f[:, a(4)], f[:, a(5)] = [11.5, 0.3, 0.1], [0.2, 8.6, 0.1], [0.2, 0.3, 5.4]
    return xyz, box, types
