"""
What the five consumers of csrc/shell_gather.h share, on the GPU, on ONE small system: angle_hist (angles.hip),
bond_order (bond_order.hip), sdf_hist (sdf.hip), contact_components (aggregates.hip) and hbond_counts (hbonds.hip) each
count the candidates within the cutoff of every centre, and every count equals (==) the numpy referee: the single-wrap
rsq of tests/angular_ref.py, strictly below the cutoff, the centre's own atom excluded and, with mol_of, the atoms of
its molecule too.

The system: 2 frames, 4302 atoms in a cubic box as 1434 molecules of 3 consecutive atoms that lie close together
(mol_of = arange(N) // 3), 33 centres (two tiles of 16 and one centre), 4097 candidates (one chunk and one candidate),
from a seeded default_rng. 5 of the centres are candidates themselves; the third atom of most centres' molecules is a
candidate, and — the molecules being compact — within the cutoff: the self test and the molecule test both decide hits.
The atom after a centre in its molecule, its hydrogen in hbond_counts, is no candidate: an acceptor on the hydrogen would
be a degenerate angle. Rows hold a handful of neighbours.

Three cases: no mol_of (the kernels look the candidate's atom up because a centre is a candidate), mol_of, and centres
that share no atom with the candidates without mol_of — the path where shell::shares_an_atom lets the kernels skip the
lookup.

angle_hist and bond_order choose their centres and candidates by atom type, which cannot say "5 of 33 centres are
candidates too"; the two overlapping cases therefore hand the lists to mdhip_angle_hist and mdhip_bond_order directly,
marshalled as backend.py does, and the disjoint case goes through backend.angle_hist and backend.bond_order.
"""
import ctypes as C

import numpy as np
import pytest

from angular_ref import _wrap_abs

pytestmark = pytest.mark.gpu

F, N_MOL, N_CEN, N_CAND, N_BOTH = 2, 1434, 33, 4097, 5
N = 3 * N_MOL
BOX = 30.0
R_CUT = 2.1  # 4097 candidates in 27 000: 5.9 within the sphere on average
RC2 = R_CUT * R_CUT
SEED = 20240611


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _hydrogen_of(atoms):
    """The atom after each atom in its molecule of three (the first after the last)."""
    return (3 * (atoms // 3) + (atoms % 3 + 1) % 3).astype(np.int32)


def _referee(xyz, box, centres, cand, mol_of):
    """count [F, C] of candidates j with rsq(centre, j) < RC2, j != centre, and another molecule under exclusion."""
    L = box[:, :, None]  # [F, 3, 1]
    count = np.zeros((len(xyz), len(centres)), dtype=np.int64)
    for k, c in enumerate(centres):
        a = _wrap_abs(xyz[:, :, c, None] - xyz[:, :, cand], L)  # [F, 3, n_cand]
        rsq = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        ok = cand != c
        if mol_of is not None:
            ok = ok & (mol_of[cand] != mol_of[c])
        count[:, k] = (ok[None, :] & (rsq < RC2)).sum(axis=1)
    return count


def _build_system():
    rng = np.random.default_rng(SEED)
    mol_of = (np.arange(N) // 3).astype(np.int32)
    home = rng.uniform(0.0, BOX, size=(F, 3, N_MOL))
    xyz = np.ascontiguousarray(np.repeat(home, 3, axis=2) + rng.normal(0.0, 0.45, size=(F, 3, N)))
    box = np.full((F, 3), BOX)
    # centres: one atom each of 33 + 5 molecules; the atom after it in the molecule is its hydrogen, never a candidate
    mols = rng.choice(N_MOL, size=N_CEN + N_BOTH, replace=False)
    listed = (3 * mols + rng.integers(0, 3, size=len(mols))).astype(np.int32)
    centres, spare = np.sort(listed[:N_CEN]), listed[N_CEN:]
    both = rng.choice(centres, size=N_BOTH, replace=False)
    free = np.setdiff1d(np.arange(N), np.concatenate([listed, _hydrogen_of(listed)]))
    cand = np.sort(np.concatenate([both, rng.choice(free, size=N_CAND - N_BOTH, replace=False)])).astype(np.int32)
    # the disjoint case: the centres that are candidates give way to the five spare ones
    apart = np.sort(np.concatenate([np.setdiff1d(centres, both), spare])).astype(np.int32)
    assert len(cand) == N_CAND and len(np.intersect1d(centres, cand)) == N_BOTH
    assert len(apart) == N_CEN and len(np.intersect1d(apart, cand)) == 0
    assert len(np.intersect1d(_hydrogen_of(listed), cand)) == 0
    s = {"xyz": xyz, "box": box, "mol_of": mol_of, "cand": cand,
         "cases": {"overlap": (centres, None, _referee(xyz, box, centres, cand, None)),
                   "overlap-mol": (centres, mol_of, _referee(xyz, box, centres, cand, mol_of)),
                   "apart": (apart, None, _referee(xyz, box, apart, cand, None))}}
    plain, excl = s["cases"]["overlap"][2], s["cases"]["overlap-mol"][2]
    assert 2.0 < plain.mean() < 12.0 and plain.max() <= 64  # a handful per row, below the first-try cap
    assert (plain - excl).sum() >= 20  # candidates of the centres' own molecules are within the cutoff
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def system():
    """The system and the referee's counts of the three cases, computed once."""
    return _build_system()


CASES =["overlap", "overlap-mol", "apart"]


def _case(system, case):
    centres, mol, want = system["cases"][case]
    return system["xyz"], system["box"], centres, system["cand"], mol, want


def _types(centres, cand):
    """Atom types that make backend.angle_hist and backend.bond_order choose these (disjoint) lists."""
    typ = np.full(N, 3, dtype=np.int32)
    typ[centres], typ[cand] = 1, 2
    return typ


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.mark.parametrize("case", CASES)
def test_angle_hist_count(B, system, case):
    xyz, box, centres, cand, mol, want = _case(system, case)
    edges = B.angle_cos_edges(10.0)
    if case == "apart":
        _, _, count, cen = B.angle_hist(xyz, box, _types(centres, cand), [(2, 1, 2)], [[RC2, RC2]], edges, mol_of=mol)
        assert np.array_equal(cen, centres)
    else:
        ctx = B.default_context()
        T, n_bins, cap = 1, len(edges), 64
        zc, za = np.zeros(len(centres), dtype=np.int32), np.zeros(len(cand), dtype=np.int32)
        trip, rc2 = np.zeros((1, 3), dtype=np.int32), np.full((1, 2), RC2)
        hist, degen = np.zeros((T, n_bins), dtype=np.uint64), np.zeros(T, dtype=np.uint64)
        count = np.zeros((F, len(centres)), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_angle_hist(
            ctx.h, F, N, B.ptr(xyz), 0, B.ptr(box), len(centres), _ip(centres), _ip(zc), len(cand), _ip(cand), _ip(za),
            _ip(mol), T, _ip(trip), B.ptr(rc2), n_bins, B.ptr(edges), cap, B.ptr(hist, C.c_uint64),
            B.ptr(degen, C.c_uint64), _ip(count)))
        # every unordered pair of a row's neighbours is one angle of the symmetric triplet
        assert int(hist.sum() + degen.sum()) == int((want * (want - 1) // 2).sum())
    print(case, "angle_hist count sum", int(count.sum()), "referee", int(want.sum()))
    assert np.array_equal(count, want)


@pytest.mark.parametrize("case", CASES)
def test_bond_order_count(B, system, case):
    xyz, box, centres, cand, mol, want = _case(system, case)
    if case == "apart":
        out = B.bond_order(xyz, box, _types(centres, cand), 1, [2], RC2, degrees=(4,), mol_of=mol)
        assert np.array_equal(out["centres"], centres)
        count = out["count"]
    else:
        ctx = B.default_context()
        deg, cap, C_ = np.array([4], dtype=np.int32), 64, len(centres)
        q, flags = np.full((F, C_, 1), np.nan), np.zeros((F, C_), dtype=np.int32)
        count = np.zeros((F, C_), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_bond_order(
            ctx.h, F, N, B.ptr(xyz), 0, B.ptr(box), C_, _ip(centres), len(cand), _ip(cand), _ip(mol), RC2, 1, _ip(deg),
            0, 0, 0, cap, B.ptr(q), None, None, _ip(flags), _ip(count)))
        assert np.array_equal(np.isnan(q[:, :, 0]), want == 0)  # (q_4 of every row with a neighbour)
    print(case, "bond_order count sum", int(count.sum()), "referee", int(want.sum()))
    assert np.array_equal(count, want)


@pytest.mark.parametrize("case", CASES)
def test_sdf_hist_n_hits(B, system, case):
    xyz, box, centres, cand, mol, want = _case(system, case)
    x_atom = _hydrogen_of(centres)  # the two other atoms of the molecule
    xy_atom = _hydrogen_of(x_atom)
    hist, degen, n_hits, bad_rows = B.sdf_hist(xyz, box, centres, x_atom, xy_atom, cand, np.zeros(len(cand), np.int32),
                                               1, R_CUT, R_CUT, mol_of=mol)
    print(case, "sdf_hist n_hits sum", int(n_hits.sum()), "referee", int(want.sum()))
    assert np.array_equal(n_hits, want)
    assert bad_rows == 0 and int(np.asarray(hist).sum() + degen.sum()) == int(want.sum())


@pytest.mark.parametrize("case", CASES)
def test_contact_components_n_contacts(B, system, case):
    xyz, box, centres, cand, mol, want = _case(system, case)
    node_of, n_nodes = (np.arange(N, dtype=np.int32), N) if mol is None else (mol, N_MOL)
    _, _, n_contacts = B.contact_components(xyz, box, centres, np.zeros(len(centres), np.int32), cand,
                                            np.zeros(len(cand), np.int32), [[RC2]], node_of, n_nodes)
    print(case, "contact_components n_contacts", n_contacts, "referee", want.sum(axis=1))
    assert np.array_equal(n_contacts.astype(np.int64), want.sum(axis=1))


@pytest.mark.parametrize("case", CASES)
def test_hbond_counts_n_bonds(B, system, case):
    xyz, box, centres, cand, mol, want = _case(system, case)
    n_bonds, n_donated, n_accepted, _, n_degenerate = B.hbond_counts(
        xyz, box, centres, np.zeros(len(centres), np.int32), np.arange(len(centres) + 1, dtype=np.int32),
        _hydrogen_of(centres), cand, np.zeros(len(cand), np.int32), RC2, 1.0, r_ha_sq=0.0, cos_edges=None, mol_of=mol)
    print(case, "hbond_counts n_bonds", n_bonds.sum(axis=(1, 2)), "referee", want.sum(axis=1), "degenerate", n_degenerate)
    assert n_degenerate == 0
    assert np.array_equal(n_bonds.sum(axis=(1, 2)).astype(np.int64), want.sum(axis=1))
    assert np.array_equal(n_donated.astype(np.int64), want.sum(axis=0))
