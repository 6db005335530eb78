"""
Host side of structural/molecular_shape.py and the numpy restatement of mdhip_mol_shape the GPU tests compare the library
with (tests/shape_ref.py); no GPU.

The restatement is held against an independent route — centre, second-moment matrix, trace, invariants and end-to-end
vector accumulated in np.longdouble from the unwrapped coordinates, the moments by np.linalg.eigvalsh — on 10^5 random
molecules that include tensors with two moments of 1e-12, planar and collinear ones. That measurement fixed the sweep
count of the kernel (shape_ref.N_SWEEPS = csrc/mol_shape.hip: SH_SWEEPS) and the bounds asserted here; DESIGN 4.13e has
the figures. Lattice shapes with known answers are compared with `==`.
"""
import os
import re

import numpy as np
import pytest

import shape_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
# Measured maxima of `deviations` over both unwrap modes and the seeds 2026, 1 and 2 at 8 sweeps — the figures at 4 and
# 5 sweeps are the same to every digit printed, at 3 sweeps the moments are off by 2e-10 —, in units of
# 2^-53: lambda 16.72, Rg2 12.29, Ree2 10.52, kappa2 11.96. The bounds are those maxima times a margin of 4, rounded
# up: between seeds the maxima move by tens of percent, not by a factor.
BOUNDS = {"lambda": 67 * EPS, "Rg2": 50 * EPS, "Ree2": 43 * EPS, "kappa2": 48 * EPS}


def _rotations(rng, n):
    Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return Q


def random_molecules(seed=2026):
    """x [1,3,A] and jobs [(atom0, mols, len, weights)]: 85 000 random molecules of 2, 3, 5, 16 and 40 atoms of any size and
    place, 5 000 with two moments of 1e-12, 5 000 planar and 5 000 collinear ones (half of each kind exactly so, along
    the axes; half turned by a random rotation)."""
    rng = np.random.default_rng(seed)
    parts, jobs, a0 = [], [], 0

    def add(pos, w):                                           # pos [M,len,3]
        nonlocal a0
        M, n, _ = pos.shape
        parts.append(pos.transpose(2, 0, 1).reshape(3, M * n))
        jobs.append((a0, M, n, w))
        a0 += M * n

    for n in (2, 3, 5, 16, 40):
        M = 17000
        scale = 10.0 ** rng.uniform(-1.0, 1.5, size=(M, 1, 1))
        pos = rng.normal(size=(M, 1, 3)) * 100.0 + np.cumsum(rng.normal(size=(M, n, 3)) * scale, axis=1)
        add(pos, rng.uniform(1.0, 32.0, size=n))
    M = 5000
    a, b = rng.uniform(0.5, 3.0, size=M), np.sqrt(3e-12)
    cross = np.zeros((M, 6, 3))
    cross[:, 0, 0], cross[:, 1, 0] = a, -a
    cross[:, 2, 1], cross[:, 3, 1], cross[:, 4, 2], cross[:, 5, 2] = b, -b, b, -b
    add(rng.normal(size=(M, 1, 3)) + cross @ _rotations(rng, M).transpose(0, 2, 1), np.ones(6))
    for n, dims in ((7, 2), (5, 1)):
        flat = np.zeros((M, n, 3))
        flat[:, :, :dims] = rng.normal(size=(M, n, dims)) * 3.0
        Q = _rotations(rng, M)
        Q[: M // 2] = np.eye(3)[rng.permutation(3)]
        offset = rng.normal(size=(M, 1, 3)) * (np.arange(M) >= M // 2)[:, None, None]     # (the exact half stays on the lattice axes)
        add(offset + flat @ Q.transpose(0, 2, 1), rng.uniform(1.0, 16.0, size=n))
    return np.ascontiguousarray(np.concatenate(parts, axis=1)[None]), jobs


def independent(x, job):
    """(moments [M,3] descending, |G|_F, Rg2, Ree2, kappa2, extent^2) of a job's molecules in extended precision."""
    a0, M, n, w = job
    X = x[0][:, a0:a0 + M * n].reshape(3, M, n).astype(np.longdouble)
    w = np.asarray(w, dtype=np.longdouble)
    com = (X * w).sum(axis=2) / w.sum()
    q = X - com[:, :, None]
    G = np.empty((M, 3, 3), dtype=np.longdouble)
    for i in range(3):
        for j in range(3):
            G[:, i, j] = (w * q[i] * q[j]).sum(axis=1) / w.sum()
    rg2 = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    i2 = (G[:, 0, 0] * G[:, 1, 1] + G[:, 1, 1] * G[:, 2, 2] + G[:, 2, 2] * G[:, 0, 0]
          - G[:, 0, 1] ** 2 - G[:, 1, 2] ** 2 - G[:, 2, 0] ** 2)
    r = X[:, :, n - 1] - X[:, :, 0]
    extent2 = ((X - X[:, :, :1]) ** 2).sum(axis=0).max(axis=1)
    lam = np.linalg.eigvalsh(G.astype(np.float64))[:, ::-1]
    return lam, np.sqrt((G ** 2).sum(axis=(1, 2))), rg2, (r ** 2).sum(axis=0), 1 - 3 * i2 / (rg2 * rg2), extent2


def deviations(x, jobs, sweeps, unwrap=1):
    """The largest deviation of the restatement from the independent route over all molecules: the moments relative to
    |G|_F, Rg2 relative to itself, Ree2 relative to the squared extent of the molecule about its first atom (the
    positions it is a difference of carry rounding errors of that size), kappa2 absolute."""
    worst = dict.fromkeys(BOUNDS, 0.0)
    for job in jobs:
        a0, M, n, w = job
        got = R.mol_shape(x, None, [a0], [M], [n], [w], unwrap=unwrap, sweeps=sweeps)["per_mol"][0]    # [6,M]
        lam, norm, rg2, ree2, k2, extent2 = independent(x, job)
        dev = {"lambda": np.abs(got[3:6].T - lam).max(axis=1) / norm, "Rg2": np.abs(got[0] - rg2) / rg2,
               "Ree2": np.abs(got[1] - ree2) / extent2, "kappa2": np.abs(got[2] - k2)}
        for key, v in dev.items():
            worst[key] = max(worst[key], float(np.max(v)))
    return worst


@pytest.fixture(scope="module")
def molecules():
    return random_molecules()


def test_restatement_against_extended_precision(molecules):
    x, jobs = molecules
    assert sum(j[1] for j in jobs) == 100000
    for unwrap in (1, 0):
        dev = deviations(x, jobs, R.N_SWEEPS, unwrap)
        print("unwrap", unwrap, {k: "%.2f eps" % (v / EPS) for k, v in dev.items()})
        for key, bound in BOUNDS.items():
            assert dev[key] <= bound, (key, dev[key] / EPS)


def test_the_sweep_count_is_the_smallest_that_meets_the_bound_plus_one(molecules):
    x, jobs = molecules
    special = jobs[5:] + jobs[:1]                          # the moments converge last where two of them nearly coincide
    enough = [s for s in range(1, R.N_SWEEPS + 1) if deviations(x, special + jobs[3:4], s)["lambda"] <= BOUNDS["lambda"]]
    assert enough and enough[0] == R.N_SWEEPS - 1, enough
    text = open(os.path.join(REPO, "mdproptools_amd", "csrc", "mol_shape.hip")).read()
    assert int(re.search(r"constexpr int SH_SWEEPS = (\d+);", text).group(1)) == R.N_SWEEPS


def _one(points, w=None, n_kbins=4, **kw):
    """The restatement's values of one molecule given as [len,3] points: dict of scalars and the histograms."""
    pts = np.asarray(points, dtype=np.float64)
    x = np.ascontiguousarray(pts.T[None])
    out = R.mol_shape(x, None, [0], [1], [len(pts)], [np.ones(len(pts)) if w is None else w], n_kbins=n_kbins, bin_size=0.25,
                      n_bins=16, **kw)
    out.update(dict(zip(R.VALUES, out["per_mol"][0, :, 0].tolist())))
    return out


def test_exact_shapes():
    rod = _one([(k, 0, 0) for k in range(4)])
    assert rod["Rg2"] == (4 * 4 - 1) / 12 == 1.25 and rod["k2"] == 1.0 and (rod["l1"], rod["l2"], rod["l3"]) == (1.25, 0.0, 0.0)
    assert rod["Ree2"] == 9.0 and rod["hist_k"][0].tolist() == [0, 0, 0, 1]
    assert np.flatnonzero(rod["hist_rg"][0]).tolist() == [int(np.sqrt(1.25) / 0.25)] and rod["hist_ee"][0, 12] == 1
    for axis in range(3):                                       # ... along every axis, and shifted
        pts = np.zeros((4, 3))
        pts[:, axis] = np.arange(4) - 7.0
        got = _one(pts)
        assert (got["Rg2"], got["k2"], got["l1"], got["l2"], got["l3"]) == (1.25, 1.0, 1.25, 0.0, 0.0)
    diag = _one([(k, k, 0) for k in range(4)])                  # the same rod along (1, 1, 0): one exact rotation
    assert diag["Rg2"] == 2.5 and diag["k2"] == 1.0 and (diag["l1"], diag["l2"], diag["l3"]) == (2.5, 0.0, 0.0)
    square = _one([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)])
    assert square["Rg2"] == 0.5 and square["k2"] == 0.25 and (square["l1"], square["l2"], square["l3"]) == (0.25, 0.25, 0.0)
    assert square["hist_k"][0].tolist() == [0, 1, 0, 0] and square["Ree2"] == 1.0
    cube = _one([(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    assert cube["Rg2"] == 0.75 and cube["k2"] == 0.0 and (cube["l1"], cube["l2"], cube["l3"]) == (0.25, 0.25, 0.25)
    assert cube["hist_k"][0].tolist() == [1, 0, 0, 0] and cube["Ree2"] == 3.0 and not cube["degenerate"].any()
    atom = _one([(3.0, 4.0, 5.0)])
    assert atom["degenerate"].tolist() == [1] and not atom["hist_k"].any() and atom["hist_rg"][0, 0] == 1
    assert (atom["Rg2"], atom["Ree2"], atom["k2"], atom["l1"]) == (0.0, 0.0, 0.0, 0.0)
    # weights: the centre moves to the heavy atom, a massless first atom does not count
    pair = _one([(0, 0, 0), (4, 0, 0)], w=[1.0, 3.0])
    assert pair["Rg2"] == (1 * 9.0 + 3 * 1.0) / 4 and pair["k2"] == 1.0
    ghost = _one([(9, 9, 9), (0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], w=[0.0, 1, 1, 1, 1], ends=[(1, 4)])
    assert (ghost["Rg2"], ghost["k2"], ghost["Ree2"]) == (1.25, 1.0, 9.0)


def test_chain_mode_follows_a_chain_through_the_box():
    """A straight 40-atom chain of spacing 1 in a box of edge 8, wrapped atom by atom: chain mode gives the rod exactly."""
    xu = np.zeros((1, 3, 40))
    xu[0, 0] = np.arange(40) + 0.5
    x = np.mod(xu, 8.0)
    L = np.full((1, 3), 8.0)
    got = R.mol_shape(x, L, [0], [1], [40], [np.ones(40)], unwrap=1, n_bins=1000)["per_mol"][0, :, 0]
    assert got[0] == (40 * 40 - 1) / 12 and got[1] == 39.0 ** 2 and got[2] == 1.0 and got[3] == (40 * 40 - 1) / 12
    first = R.mol_shape(x, L, [0], [1], [40], [np.ones(40)], unwrap=0, n_bins=1000)["per_mol"][0, :, 0]
    assert first[0] < 8.0 and first[0] != got[0]


# ---- the tables of the module ---------------------------------------------------------------------------------------------


def test_tables_from_synthetic_counts():
    from mdproptools_amd.structural import molecular_shape as M

    rng = np.random.default_rng(3)
    J, nb, nk, F = 3, 8, 4, 5
    hist_rg, hist_ee = rng.integers(0, 50, (J, nb)).astype(np.uint64), rng.integers(0, 50, (J, nb)).astype(np.uint64)
    hist_k = rng.integers(0, 50, (J, nk)).astype(np.uint64)
    hist_rg[1] = hist_ee[1] = 0
    hist_k[1] = 0                                                    # an empty type
    n_mols = np.array([7, 0, 2])
    totals = rng.random((J, 9, F)) * n_mols[:, None, None]
    beyond, degenerate = np.array([[1, 2], [0, 0], [3, 0]], dtype=np.uint64), np.array([0, 0, 4], dtype=np.uint64)
    steps = 100 * np.arange(F)
    out = M.tables(["a", "b", "c"], n_mols, steps, hist_rg, hist_ee, hist_k, beyond, degenerate, totals, 0.5)
    assert sorted(out) == sorted(M.TABLES) and list(out["summary"].columns) == M.SUMMARY
    assert np.array_equal(out["rg"]["r (A)"], 0.25 + 0.5 * np.arange(nb)) and np.array_equal(out["kappa2"]["kappa2"], [0.125, 0.375, 0.625, 0.875])
    for j, name in enumerate("abc"):
        for table, hist, width in (("rg", hist_rg, 0.5), ("ree", hist_ee, 0.5), ("kappa2", hist_k, 0.25)):
            col = out[table]["p_" + name].to_numpy()
            assert np.array_equal(col, R.density(hist[j], width), equal_nan=True)
            if j == 1:
                assert np.isnan(col).all()
            else:
                assert abs(col.sum() * width - 1.0) < 1e-14      # normalised
        row = out["summary"].iloc[j]
        want = R.summary_row(totals[j], n_mols[j], F)
        if want is None:
            assert all(np.isnan(row[k]) for k in M.SUMMARY[2:13])
        else:
            assert all(row[k] == want[k] for k in want), (row, want)
            assert row["asphericity"] == row["<l1>"] - (row["<l2>"] + row["<l3>"]) / 2
        assert (row["molecule"], row["n_mols"], row["beyond Rg"], row["beyond Ree"], row["degenerate"]) == (
            name, n_mols[j], beyond[j, 0], beyond[j, 1], degenerate[j])
    assert np.array_equal(out["frames"]["timestep"], steps)
    assert np.array_equal(out["frames"]["Rg_a"], totals[0, 1] / 7.0) and np.array_equal(out["frames"]["Ree2_c"], totals[2, 2] / 2.0)
    assert np.isnan(out["frames"]["Rg_b"]).all()


def test_argument_errors():
    from mdproptools_amd.structural import molecular_shape as M

    call = lambda **kw: M.calc_molecular_shape(**dict(dict(filename="none.*.dump", num_mols=[3, 2], num_atoms_per_mol=[4, 6],  # noqa: E731
                                                           mass=[1.0, 12.0]), **kw))
    for kw, text in ((dict(ends=[(1, 5), None]), "must be in"), (dict(ends=[(0, 2), None]), "must be in"),
                     (dict(ends=[(1, 2)]), "ends must hold"), (dict(ends=[3, None]), "not a pair"),
                     (dict(num_mols=[3]), "one entry per molecule type"), (dict(mol_types=[1], mol_names=["a", "b"]), "mol_names"),
                     (dict(mol_names=["a", "a"]), "mol_names"), (dict(mol_types=[3]), "mol_types"), (dict(mol_types=[1, 1]), "twice"),
                     (dict(mol_types=[]), "at least one"), (dict(unwrap="Chain"), "unwrap must be"), (dict(unwrap=1), "unwrap must be"),
                     (dict(coords="scaled"), "coords must be"), (dict(kappa_bins=0), "kappa_bins"), (dict(kappa_bins=1025), "kappa_bins"),
                     (dict(bin_size=0.0), "positive and finite"), (dict(r_max=300.0, bin_size=0.05), "larger bin_size"),
                     (dict(r_max=float("nan")), "positive and finite")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    assert M.default_r_max([4, 6]) == 5.0 and M.default_r_max([1]) == 2.0 and M._n_bins(5.0, 0.05) == 100
    with pytest.raises(ValueError, match="same atom types"):
        M.weight_rows(np.array([1, 2, 1, 1]), [1.0, 2.0], [0], [2], [2], ["a"])
    with pytest.raises(ValueError, match="outside the 2 entries of mass"):
        M.weight_rows(np.array([1, 3, 1, 3]), [1.0, 2.0], [0], [2], [2], ["a"])
    with pytest.raises(ValueError, match="mass must hold"):
        M.weight_rows(np.array([1, 2, 1, 2]), None, [0], [2], [2], ["a"])
    rows = M.weight_rows(np.array([1, 2, 1, 2, 2]), [1.0, 16.0], [0, 4], [2, 1], [2, 1], ["a", "b"])
    assert [r.tolist() for r in rows] == [[1.0, 16.0], [16.0]]


# ---- ABI and build --------------------------------------------------------------------------------------------------------


def test_the_entry_point_is_declared_bound_and_built():
    from mdproptools_amd import _lib, build

    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    m = re.search(r"\bint mdhip_mol_shape\s*\(([^;]*)\);", text)
    assert m, "include/mdhip.h does not declare mdhip_mol_shape"
    assert "mdhip_mol_shape" in _lib.PROTOTYPES and "mol_shape.hip" in build.SOURCES
    assert len(_lib.PROTOTYPES["mdhip_mol_shape"][1]) == len(m.group(1).split(",")) == 26
    assert os.path.join(build.CSRC, "shape_plan.h") in build.HEADERS          # (its changes rebuild the library)
    assert callable(_lib.load().mdhip_mol_shape)
