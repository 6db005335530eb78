"""
CPU-only checks of the hydrogen-bond analysis: the numpy restatement (tests/hbonds_ref.py) on closed forms, the
lifetime integers against a brute-force loop over bit patterns, the host code of structural/hydrogen_bonds.py
(topology from the altered types, normalisation, tau, argument errors) and the two new symbols at the ABI.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hbonds_ref as R
from conftest import REPO
from mdproptools_amd import _lib, backend
from mdproptools_amd.common.com_mols import calc_atom_type
from mdproptools_amd.structural import hydrogen_bonds as HB

L = np.array([20.0, 20.0, 20.0])
COS150 = float(np.cos(np.radians(150.0)))


def _dimer(d, h, a):
    """One frame of three atoms: donor 0, hydrogen 1, acceptor 2."""
    return np.array([d, h, a], dtype=np.float64).T[None], L[None]


def _one(xyz, box, r_da=3.5, cos_cut=COS150, r_ha_sq=0.0):
    reach, cos = R.geometry(xyz, box, [0], [0, 1], [1], [2], r_da ** 2, r_ha_sq)
    b = R.bonded(xyz, box, [0], [0, 1], [1], [2], r_da ** 2, r_ha_sq, cos_cut)
    return bool(reach[0, 0, 0]), float(cos[0, 0, 0]), bool(b[0, 0, 0])


# ---- the restatement on closed forms ----

def test_collinear_dimer():
    reach, cos, bond = _one(*_dimer([5, 5, 5], [5.96, 5, 5], [7.8, 5, 5]))
    assert reach and cos == -1.0 and bond
    assert _one(*_dimer([5, 5, 5], [5.96, 5, 5], [7.8, 5, 5]), cos_cut=-1.0)[2]  # cos == cos_cut is in
    # across the boundary: the same dimer shifted so that H and A are wrapped differently
    reach, cos, bond = _one(*_dimer([19.5, 5, 5], [0.46, 5, 5], [2.3, 5, 5]))
    assert reach and bond and cos == pytest.approx(-1.0, abs=1e-15)


def test_perpendicular_dimer():
    xyz, box = _dimer([6, 6, 3], [6, 7, 3], [8, 7, 3])
    reach, cos, bond = _one(xyz, box, cos_cut=0.0)
    assert reach and cos == 0.0 and bond
    assert not _one(xyz, box)[2]  # 90 degrees is no bond at 150


def test_acceptor_at_exactly_r_da_is_out():
    xyz, box = _dimer([5, 5, 2], [6, 5, 2], [8.5, 5, 2])
    assert float(R.rsq(xyz[0][:, 0], xyz[0][:, 2], L)) == 3.5 ** 2
    assert _one(xyz, box) == (False, -1.0, False)
    xyz[0, 0, 2] = 8.499
    assert _one(xyz, box) == (True, -1.0, True)
    assert not _one(xyz, box, r_ha_sq=2.4 ** 2)[0] and _one(xyz, box, r_ha_sq=2.6 ** 2)[0]  # H...A is 2.499
    xyz[0, 0, 1], xyz[0, 0, 2] = 6.0, 8.0
    assert not _one(xyz, box, r_ha_sq=4.0)[0] and _one(xyz, box, r_ha_sq=4.0 + 1e-12)[0]  # H...A exactly 2: strict


def test_degenerate_and_nonfinite():
    xyz, box = _dimer([5, 5, 5], [5, 5, 5], [7, 5, 5])  # H on D
    reach, cos, bond = _one(xyz, box)
    assert reach and np.isnan(cos) and not bond
    top = ([0], [0], [0, 1], [1], [2], [0])
    assert R.hbond_counts(xyz, box, *top, 3.5 ** 2, COS150, edges=R.cos_edges(1.0))[4] == 1
    for bad in (np.nan, np.inf, -np.inf):
        for atom in range(3):
            xyz, box = _dimer([5, 5, 5], [5.96, 5, 5], [7.8, 5, 5])
            xyz[0, 1, atom] = bad
            assert not _one(xyz, box)[2]
            if atom != 1:
                assert not _one(xyz, box)[0]


def test_counts_of_a_small_system_against_loops():
    """hbond_counts against the definition written as loops over (frame, donor, hydrogen, acceptor)."""
    rng = np.random.default_rng(0)
    box = np.array([[7.0, 6.5, 6.0], [7.5, 6.0, 6.5]])
    xyz = np.round(rng.uniform(0, 6, (2, 3, 24)), 3)
    don, dcl = [0, 3, 6, 9], [0, 1, 0, 1]
    h_off, h_atoms = [0, 2, 3, 3, 6], [1, 2, 4, 10, 11, 12]
    acc, acl = [0, 3, 13, 14, 15, 16, 17, 18, 19, 20], [0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    for d, lo, hi in ((0, 0, 2), (3, 2, 3), (9, 3, 6)):
        for h in h_atoms[lo:hi]:
            xyz[:, :, h] = np.round(xyz[:, :, d] + rng.normal(size=(2, 3)) * 0.55, 3)
    mol_of = np.arange(24) // 3
    edges = R.cos_edges(10.0)
    cut = float(np.cos(np.radians(100.0)))
    nb, nd, na, hist, degen = R.hbond_counts(xyz, box, don, dcl, h_off, h_atoms, acc, acl, 3.5 ** 2, cut,
                                             r_ha_sq=2.8 ** 2, edges=edges, mol_of=mol_of)
    wb, wd, wa, wh = np.zeros_like(nb), np.zeros_like(nd), np.zeros_like(na), np.zeros_like(hist)
    for f in range(2):
        for di, d in enumerate(don):
            for k in range(h_off[di], h_off[di + 1]):
                for ai, a in enumerate(acc):
                    if a == d or mol_of[a] == mol_of[d]:
                        continue
                    if not float(R.rsq(xyz[f][:, d], xyz[f][:, a], box[f])) < 3.5 ** 2:
                        continue
                    if not float(R.rsq(xyz[f][:, h_atoms[k]], xyz[f][:, a], box[f])) < 2.8 ** 2:
                        continue
                    c = float(R.cosine(xyz[f][:, d], xyz[f][:, h_atoms[k]], xyz[f][:, a], box[f]))
                    wh[dcl[di], acl[ai], sum(1 for m in range(1, len(edges)) if c <= edges[m])] += 1
                    if c <= cut:
                        wb[f, dcl[di], acl[ai]] += 1
                        wd[di] += 1
                        wa[ai] += 1
    assert wb.sum() > 0 and degen == 0
    assert np.array_equal(nb, wb) and np.array_equal(nd, wd) and np.array_equal(na, wa) and np.array_equal(hist, wh)


# ---- the lifetime integers ----

def test_lifetime_sums_against_brute_force():
    rng = np.random.default_rng(1)
    pats = [(rng.random(23) < p).astype(int) for p in (0.2, 0.5, 0.8, 0.95)]
    pats += [np.ones(23, dtype=int), np.zeros(23, dtype=int), (np.arange(23) % 4 < 2).astype(int)]
    for max_lag in (0, 5, 22):
        c_int, c_cont = R.lifetime_sums(np.array(pats), max_lag)
        b_int, b_cont = R.brute_lifetime([list(p) for p in pats], max_lag)
        assert np.array_equal(c_int, b_int) and np.array_equal(c_cont, b_cont)
        assert c_int[0] == c_cont[0] == sum(int(p.sum()) for p in pats)
        assert np.all(c_cont <= c_int)


def test_lifetime_closed_forms():
    F = 40
    k = np.arange(F)
    c_int, c_cont = R.lifetime_sums(np.ones((1, F), dtype=bool), F - 1)
    assert np.array_equal(c_int, F - k) and np.array_equal(c_cont, F - k)
    c_int, c_cont = R.lifetime_sums((np.arange(F) % 4 < 2)[None], F - 1)  # 1100 1100 ...
    assert c_cont[0] == 20 and c_cont[1] == 10 and not c_cont[2:].any()
    assert c_int[4] == 18 and c_int[2] == 0
    # every run of L ones adds max(0, L - k)
    runs = np.zeros((1, 30), dtype=bool)
    runs[0, 2:9] = runs[0, 12:15] = runs[0, 29:] = True  # L = 7, 3, 1
    _, c_cont = R.lifetime_sums(runs, 29)
    assert np.array_equal(c_cont, [max(0, 7 - j) + max(0, 3 - j) + max(0, 1 - j) for j in range(30)])


# ---- host code ----

def _types(num_mols, num_atoms_per_mol):
    n = int(np.dot(num_mols, num_atoms_per_mol))
    return calc_atom_type(np.arange(1, n + 1), num_mols, num_atoms_per_mol).astype(np.int32)


def test_topology_water_like():
    n, mol_of = HB._layout([4], [3])
    assert n == 12 and np.array_equal(mol_of, np.arange(12) // 3)
    top = HB._topology(_types([4], [3]), mol_of, [(1, 2), (1, 3)], [1])
    assert np.array_equal(top["donors"], [0, 3, 6, 9]) and np.array_equal(top["don_class"], [0, 0, 0, 0])
    assert np.array_equal(top["h_off"], [0, 2, 4, 6, 8])
    assert np.array_equal(top["h_atoms"], [1, 2, 4, 5, 7, 8, 10, 11])
    assert np.array_equal(top["acceptors"], [0, 3, 6, 9]) and np.array_equal(top["acc_class"], [0, 0, 0, 0])
    assert top["d_types"] == [1] and top["a_types"] == [1]


def test_topology_two_species():
    """Two ions of one atom, three waters O H H, two methanols C O H H3 (the hydroxyl H is atom 3 of the molecule):
    altered types 1 | 2 3 4 | 5 6 7 8."""
    num_mols, apm = [2, 3, 2], [1, 3, 4]
    types = _types(num_mols, apm)
    assert list(types) == [1, 1, 2, 3, 4, 2, 3, 4, 2, 3, 4, 5, 6, 7, 8, 5, 6, 7, 8]
    n, mol_of = HB._layout(num_mols, apm)
    top = HB._topology(types, mol_of, [(6, 7), (2, 3), (2, 4)], [2, 6, 1])
    assert top["d_types"] == [6, 2]                                     # classes in the order given
    assert np.array_equal(top["donors"], [2, 5, 8, 12, 16])
    assert np.array_equal(top["don_class"], [1, 1, 1, 0, 0])
    assert np.array_equal(top["h_off"], [0, 2, 4, 6, 7, 8])
    assert np.array_equal(top["h_atoms"], [3, 4, 6, 7, 9, 10, 13, 17])
    assert np.array_equal(top["acceptors"], [0, 1, 2, 5, 8, 12, 16])
    assert np.array_equal(top["acc_class"], [2, 2, 0, 0, 0, 1, 1])


def test_argument_errors(tmp_path):
    types, (n, mol_of) = _types([2, 3], [1, 3]), HB._layout([2, 3], [1, 3])
    with pytest.raises(ValueError, match="num_mols and num_atoms_per_mol"):
        HB._layout(None, None)
    with pytest.raises(ValueError, match="num_mols and num_atoms_per_mol"):
        HB.calc_hydrogen_bonds([(2, 3)], [2], "nowhere.*.dump", None, None)
    with pytest.raises(ValueError, match="num_mols and num_atoms_per_mol"):
        HB.calc_hbond_lifetime([(2, 3)], [2], "nowhere.*.dump", [], [])
    with pytest.raises(ValueError, match="hydrogen type 3 has no donor of type 1 in its molecule"):
        HB._topology(types, mol_of, [(1, 3)], [2])
    with pytest.raises(ValueError, match="names no atom"):
        HB._topology(types, mol_of, [(2, 9)], [2])
    with pytest.raises(ValueError, match="donors must be a non-empty list"):
        HB._topology(types, mol_of, [], [2])
    with pytest.raises(ValueError, match="acceptors must be a non-empty list"):
        HB._topology(types, mol_of, [(2, 3)], [])
    with pytest.raises(ValueError, match="non-empty"):
        HB.calc_hydrogen_bonds([], [2], "nowhere.*.dump", [2, 3], [1, 3])
    with pytest.raises(ValueError, match="r_da must be positive"):
        HB._geometry(0.0, 150.0, None)
    with pytest.raises(ValueError, match="angle_cut"):
        HB._geometry(3.5, 190.0, None)
    # a non-uniform time step is refused before anything reaches the GPU
    xyz = np.round(np.random.default_rng(0).uniform(0, 9, (3, 3, 6)), 3)
    pattern = R.write_dumps(xyz, np.full((3, 3), 9.0), str(tmp_path), steps=[0, 10, 30])
    with pytest.raises(ValueError, match="uniformly spaced"):
        HB.calc_hbond_lifetime([(1, 2), (1, 3)], [1], pattern, [2], [3])
    with pytest.raises(ValueError, match="does not match"):
        HB.calc_hbond_lifetime([(1, 2), (1, 3)], [1], pattern, [3], [3])


def test_normalisation_and_tau(monkeypatch):
    """C[k] = (c[k] / (F - k)) / (c[0] / F); tau of a pure exponential is the closed trapezoid value."""

    def cumtrapz(y, dx):  # (backend.cumtrapz runs on the GPU; its arithmetic is tested there)
        y = np.asarray(y)
        return np.cumsum((y[1:] + y[:-1]) * 0.5 * dx)

    monkeypatch.setattr(backend, "cumtrapz", cumtrapz)
    F, delta = 64, 0.25
    k = np.arange(F)
    c_int = np.array([1000 * (F - j) for j in k], dtype=np.uint64)   # an always-bonded population: C_int == 1
    c_cont = np.array([(F - j) * 2 ** (20 - j) if j <= 20 else 0 for j in k], dtype=np.uint64)  # C_cont == 2**-k
    table, tau_int, tau_cont = HB._lifetime_table(c_int, c_cont, F, delta)
    assert list(table.columns) == ["Time (ps)", "C_int", "C_cont"]
    assert np.array_equal(table["Time (ps)"].to_numpy(), k * delta)
    assert np.array_equal(table["C_int"].to_numpy(), np.ones(F))
    want = np.where(k <= 20, 0.5 ** np.minimum(k, 20), 0.0)
    assert np.array_equal(table["C_cont"].to_numpy(), want)
    assert tau_int == (F - 1) * delta
    # trapezoid of q**k, k = 0 .. 20, then the step down to 0: dx * (1/2 + q + ... + q**20)  (both ends halved, the
    # last one's other half belongs to the step to zero)
    closed = delta * (0.5 + sum(0.5 ** j for j in range(1, 21)))
    assert tau_cont == pytest.approx(closed, rel=1e-15)
    # a single frame, and a trajectory without bonds
    t1, a, b = HB._lifetime_table(np.array([5], dtype=np.uint64), np.array([5], dtype=np.uint64), 1, 0.0)
    assert t1["C_int"].iloc[0] == 1.0 and (a, b) == (0.0, 0.0)
    t0, a, b = HB._lifetime_table(np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), 3, 1.0)
    assert np.isnan(t0["C_int"]).all() and np.isnan(a) and np.isnan(b)


# ---- ABI ----

def test_abi_of_the_two_symbols():
    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    lib_path = os.path.join(REPO, "mdproptools_amd", "libmdhip.so")
    _lib.load()
    exported = ""
    if shutil.which("nm"):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True,
                                  check=True).stdout
    for name, n_args in (("mdhip_hbond_counts", 28), ("mdhip_hbond_lifetime", 23)):
        m = re.search(r"^int %s\((.*?)\);" % name, text, flags=re.M | re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is _lib.C.c_int and len(argtypes) == n_args
        for a, t in zip(args, argtypes):  # pointer against pointer, width against width
            if "*" in a:
                assert t is _lib.C.c_void_p or hasattr(t, "contents") or t is _lib.C.c_char_p, (name, a, t)
            else:
                want = {"int64_t": 8, "int32_t": 4, "int": 4, "double": 8}[a.split()[-2]]
                assert _lib.C.sizeof(t) == want and not hasattr(t, "contents"), (name, a, t)
                assert (t is _lib.C.c_double) == (a.split()[-2] == "double"), (name, a, t)
        if exported:
            assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    assert _lib.load().mdhip_version() == 610
