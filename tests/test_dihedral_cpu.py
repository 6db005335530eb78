"""
Host side of structural/dihedral_distribution.py and the numpy restatement of mdhip_dihedral_angles the GPU tests compare
against (tests/dihedral_ref.py); no GPU. Where a public function needs the library's kernel, `backend.dihedral_angles`
(and `backend.orient_corr`) are replaced by the restatement, so what is checked here is the host code around them —
arguments, labels, jobs, tables, files — and the restatement itself on geometry whose torsions are known.
"""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest

import dihedral_ref as R
import reorientation_ref as RR
from conftest import REPO
from mdproptools_amd import backend
from mdproptools_amd.structural import dihedral_distribution as M
from mdproptools_amd.structural.dihedral_distribution import calc_dihedral_correlation, calc_dihedral_distribution


def test_signatures():
    assert str(inspect.signature(calc_dihedral_distribution)) == (
        "(dihedrals, filename, num_mols, num_atoms_per_mol, bin_size=1.0, states=None, coords='wrapped', "
        "save_mode=True, working_dir=None)")
    assert str(inspect.signature(calc_dihedral_correlation)) == (
        "(dihedrals, filename, num_mols, num_atoms_per_mol, dt=1, max_lag=None, coords='wrapped', save_mode=True, "
        "working_dir=None)")
    assert str(inspect.signature(backend.dihedral_angles)) == (
        "(x, box, job_atom0, job_mols, job_len, quads, job_row=None, n_bins=None, want_series=False, out=None, ctx=None)")
    assert backend.DIHEDRAL_MAX_ROWS == 16 and backend.DIHEDRAL_MAX_BINS == 1440
    assert M.STREAM is True and M.BATCH_BYTES is None and M.MAX_DIHEDRALS == 16
    assert M.DEFAULT_STATES == {"g-": (-120, 0), "g+": (0, 120), "t": (120, -120)}


@pytest.mark.parametrize("dihedrals", [
    [],                                                   # empty
    [(1, 1, 2, 3)], [(1, 1, 2, 3, 4, 5)], [(1,)],         # wrong arity
    [(1, [(1, 2, 3)])], [(1, [(1, 2, 3, 4)], "a", "b")], [(1, [(1, 2, 3, 4)], 7)], [(1, [])],
    [(0, 1, 2, 3, 4)], [(3, 1, 2, 3, 4)],                 # molecule type out of range
    [(1, 0, 2, 3, 4)], [(1, 1, 2, 3, 5)], [(2, [(1, 2, 3, 4), (3, 4, 5, 7)])],   # an atom outside the molecule
    [(1, 1, 2, 2, 3)], [(2, [(1, 2, 3, 4), (6, 5, 4, 6)])],                      # a repeated atom
    [(1, 1, 2, 3, 4)] * 2,                                # the same default label twice
    [(2, [(1, 2, 3, 4)], "t%d" % n) for n in range(17)],  # more than 16 entries
])
def test_bad_dihedrals_are_value_errors(dihedrals):
    for call in (calc_dihedral_distribution, calc_dihedral_correlation):
        with pytest.raises(ValueError):
            call(dihedrals, "none.*", [5, 2], [4, 6], save_mode=False)


def test_other_host_errors():
    good = [(1, 1, 2, 3, 4)]
    for call in (calc_dihedral_distribution, calc_dihedral_correlation):
        with pytest.raises(ValueError, match="coords"):
            call(good, "none.*", [5, 2], [4, 6], coords="scaled", save_mode=False)
        with pytest.raises(ValueError, match="one entry per molecule type"):
            call(good, "none.*", [5, 2], [4], save_mode=False)
    for bad in (0.0, -1.0, 0.2, 0.125, 7.0, 0.7, 181.0, 360.0, float("nan")):
        with pytest.raises(ValueError, match="bin_size"):
            calc_dihedral_distribution(good, "none.*", [5, 2], [4, 6], bin_size=bad, save_mode=False)
    assert [M._n_bins(v) for v in (0.25, 0.5, 1, 1.0, 5, 7.5, 90, 180)] == [1440, 720, 360, 360, 72, 48, 4, 2]
    for states in ({}, {"a": (0, 0.5)}, {"a": (10, 10)}, {"a": (-190, 0)}, {"a": (0, 181)}, {"a": 3}, {"a": (1, 2, 3)}):
        with pytest.raises(ValueError, match="state"):
            calc_dihedral_distribution(good, "none.*", [5, 2], [4, 6], states=states, save_mode=False)
    assert len(M._checked([(2, [(1, 2, 3, 4)], "t%d" % n) for n in range(16)], [4, 6])) == 16
    entries = M._checked([(1, 1, 2, 3, 4), (2, [(1, 2, 3, 4), (3, 4, 5, 6)]), (2, 6, 5, 4, 3)], [4, 6])
    M._refuse_degenerate(entries, [0, 0, 0])
    with pytest.raises(ValueError, match=r"2:6-5-4-3 \(7\)") as err:
        M._refuse_degenerate(entries, [0, 0, 7])
    assert "1:1-2-3-4" not in str(err.value) and "+1" not in str(err.value)


def test_labels_jobs_and_rows_of_pooled_entries():
    entries = M._checked([(1, 1, 2, 3, 4), (2, [(1, 2, 3, 4), (2, 3, 4, 5), (6, 5, 4, 3)]), (2, [[3, 4, 5, 6]], "tail"),
                          (1, 4, 3, 2, 1)], [4, 6])
    assert [e[2] for e in entries] == ["1:1-2-3-4", "2:1-2-3-4+2", "tail", "1:4-3-2-1"]
    a0, mols, length, quads, rows = M._jobs(entries, [5, 2], [4, 6])
    assert a0.tolist() == [0, 20, 20, 20, 20, 0] and mols.tolist() == [5, 2, 2, 2, 2, 5]
    assert length.tolist() == [4, 6, 6, 6, 6, 4] and rows.tolist() == [0, 1, 1, 1, 2, 3]
    assert quads.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [1, 2, 3, 4], [5, 4, 3, 2], [2, 3, 4, 5], [3, 2, 1, 0]]
    assert a0.dtype == mols.dtype == np.int64 and length.dtype == quads.dtype == rows.dtype == np.int32


def test_header_declares_the_entry_point_and_the_library_exports_it():
    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    assert re.search(r"\bint mdhip_dihedral_angles\s*\(mdhip_ctx \*ctx,", text)
    flat = text.replace("\n * ", " ")
    assert "NEGATIVE HALF IS RIGHT-CLOSED" in flat and "wrapped on its own" in flat and "no acos, no atan2" in flat
    from mdproptools_amd import _lib, build

    assert "mdhip_dihedral_angles" in _lib.PROTOTYPES and "dihedrals.hip" in build.SOURCES
    assert len(_lib.PROTOTYPES["mdhip_dihedral_angles"][1]) == 19
    assert callable(_lib.load().mdhip_dihedral_angles)


# ---- the restatement on known geometry ---------------------------------------------------------------------------------


def _one(points, n_bins, box=None):
    """(hist row, U [3], degenerate) of one quadruple given as [4,3] points."""
    x = np.ascontiguousarray(np.asarray(points, dtype=np.float64).T[None])          # [1,3,4]
    hist, U, deg = R.dihedral_angles(x, box, [0], [1], [4], [(0, 1, 2, 3)], n_bins=n_bins)
    return hist[0], U[0, :, 0], int(deg[0])


def test_restatement_on_the_lattice():
    """b1 = e_x, b2 = e_y and b3 in {-e_x, +e_x, +e_z, -e_z}: phi = 0, 180, +90, -90 with (c, sn) exact; n_bins = 4 shows
    the mirrored edge rule: 0 in bin 2, 180 in bin 3, +90 in bin 3 (left-closed) and -90 in bin 0 (right-closed)."""
    ex, ey, ez = np.eye(3)
    want = [(-ex, (1.0, 0.0), 2), (ex, (-1.0, 0.0), 3), (ez, (0.0, 1.0), 3), (-ez, (0.0, -1.0), 0)]
    for b3, (c, sn), bin4 in want:
        pts = np.cumsum([np.zeros(3), ex, ey, b3], axis=0)
        hist, u, deg = _one(pts, 4)
        assert u.tolist() == [c, sn, 0.0] and deg == 0, (b3, u)
        assert hist.tolist() == [int(b == bin4) for b in range(4)], (b3, hist)
        b = [tuple(np.array([v]) for v in d) for d in (ex, ey, b3)]
        cc, s, _, _, lb = R.torsion_terms(*b)
        n1, n2 = R._cross(b[0], b[1]), R._cross(b[1], b[2])
        phi = np.arctan2(lb * s, R._dot(n1, n2))[0]
        assert phi == np.arctan2(sn, c) and phi in (0.0, np.pi, np.pi / 2, -np.pi / 2)      # the sign is atan2's
    # s == -0 counts as the positive side too
    assert R.bins_of(np.array([-1.0, 1.0]), np.array([-0.0, -0.0]), 4).tolist() == [3, 2]
    # a cosine an ulp outside +-1 lands in the first or last half-bin, whatever n_bins
    for nb in (2, 4, 360, 1440):
        out = R.bins_of(np.array([np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)] * 2), np.array([1.0, 1.0, -1.0, -1.0]), nb)
        assert out.tolist() == [nb // 2, nb - 1, nb // 2 - 1, 0]


def test_restatement_on_a_butane_like_chain():
    for phi in (60.5, -60.5, 179.5, -179.5, 0.5):
        hist, u, deg = _one(R.chain(phi), 360)
        assert deg == 0 and hist.sum() == 1 and hist[int(np.floor(phi + 180.0))] == 1, (phi, np.flatnonzero(hist))
        assert abs(np.degrees(np.arctan2(u[1], u[0])) - phi) < 1e-12 and u[2] == 0.0
    # seen through a periodic box that cuts every bond: the same bits (grid coordinates: the wraps are exact)
    pts = np.rint(R.chain(60.5) * 1024) / 1024 + np.array([3.0, 3.5, 0.25])
    L = np.array([[4.0, 5.0, 6.0]])
    assert (np.abs(np.diff(np.mod(pts, L), axis=0)) > L / 2).any()
    assert RR.same_bits(_one(np.mod(pts, L), 360, box=L)[1], _one(pts, 360)[1])


def test_restatement_against_atan2_on_gaussian_quadruples():
    """2 x 10^6 Gaussian quadruples (seed 0): the cosine-table bin equals floor((degrees(atan2) + 180) / D) at every
    one, at n_bins 2, 72, 360 and 1440; |c| <= 1 throughout."""
    B = np.random.default_rng(0).normal(size=(3, 3, 2_000_000))
    b = [tuple(B[i]) for i in range(3)]
    c, s, sn, den, _ = R.torsion_terms(*b)
    assert np.abs(c).max() <= 1.0 and (den > 0).all()
    for nb in (2, 72, 360, 1440):
        assert int((R.bins_of(c, s, nb) != R.atan2_bins(*b, nb)).sum()) == 0, nb


def test_restatement_counts_every_finite_quadruple_once():
    """Row total + degenerate = jobs in the row x molecules x frames; degenerate and NaN rules; unnamed atoms unread."""
    rng = np.random.default_rng(4)
    F, mols = 9, 13
    x = rng.normal(size=(F, 3, 5 * mols + 4 * 3))
    x[2, :, 5 * 4 + 3] = 2 * x[2, :, 5 * 4 + 1] - x[2, :, 5 * 4]      # molecule 4, frame 2: atoms 0, 1, 3 collinear
    x[7, :, 5 * 6 + 4] = x[7, :, 5 * 6 + 3]                           # molecule 6, frame 7: atoms 3 and 4 coincide
    x[:, :, 2::5][:, :, :mols] = np.nan                               # atom 2 of the first type is never named
    a0, m, length = [0, 0, 5 * mols, 0], [mols, mols, 3, mols], [5, 5, 4, 5]
    quads = [(0, 1, 3, 4), (4, 3, 1, 0), (0, 1, 2, 3), (1, 0, 3, 4)]
    rows = [0, 0, 1, 2]
    hist, U, deg = R.dihedral_angles(x, None, a0, m, length, quads, job_row=rows, n_bins=72)
    assert deg.tolist() == [2, 2, 0, 2] and not np.isnan(U).any()     # (1, 0, 3, 4) has b1 along b2 in molecule 4 as well
    assert hist.sum(axis=1).tolist() == [2 * mols * F - 4, 3 * F, mols * F - 2]
    assert not U[4, :, 2].any() and not U[6, :, 7].any() and U[5, :2, 2].all()
    # the reversed quadruple sees the same angle: equal histograms, equal cosines
    h_f, U_f, _ = R.dihedral_angles(x, None, a0[:1], m[:1], length[:1], quads[:1], n_bins=72)
    h_r, U_r, _ = R.dihedral_angles(x, None, a0[:1], m[:1], length[:1], quads[1:2], n_bins=72)
    assert np.array_equal(h_f, h_r) and np.abs(U_f - U_r).max() < 1e-12
    # a NaN in a named atom: NaN in that (series, frame) only, not counted anywhere
    y = x.copy()
    y[3, 1, 5 * 2 + 1] = np.nan
    h2, U2, deg2 = R.dihedral_angles(y, None, a0, m, length, quads, job_row=rows, n_bins=72)
    hit = np.zeros(U.shape, dtype=bool)
    hit[[2, mols + 2, 2 * mols + 3 + 2], :2, 3] = True                # molecule 2 in the series of jobs 0, 1 and 3
    assert deg2.tolist() == deg.tolist() and (hist.sum(axis=1) - h2.sum(axis=1)).tolist() == [2, 0, 1]
    assert np.array_equal(np.isnan(U2), hit) and U2[2, 2, 3] == 0.0 and RR.same_bits(U2[~hit], U[~hit])
    # only one of the two results
    assert R.dihedral_angles(x, None, a0, m, length, quads, n_bins=None)[0] is None
    assert R.dihedral_angles(x, None, a0, m, length, quads, n_bins=4, want_series=False)[1] is None


# ---- tables and files, the backend replaced by the restatement ------------------------------------------------------------

ENTRIES = [(1, 1, 2, 3, 4), (2, [(1, 2, 3, 4), (2, 3, 4, 5), (6, 5, 4, 3)], "backbone"), (1, 4, 3, 2, 1)]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("dihedral_cpu")
    traj = R.synthetic_trajectory(n_frames=6)
    return {"dir": d, "traj": traj, "pattern": R.write_dumps(d, traj, file_order=[3, 0, 5, 1, 4, 2])}


def _restated(monkeypatch):
    calls = []

    def dihedral_angles(x, box, a0, mols, length, quads, job_row=None, n_bins=None, want_series=False, out=None, ctx=None):
        calls.append((np.asarray(x).shape[0], None if box is None else np.asarray(box).shape, n_bins, want_series))
        return R.dihedral_angles(np.array(x), None if box is None else np.array(box), a0, mols, length,
                                 [tuple(q) for q in quads], job_row=job_row, n_bins=n_bins, want_series=want_series)

    monkeypatch.setattr(backend, "dihedral_angles", dihedral_angles)
    return calls


@pytest.mark.parametrize("stream", [False, True])
def test_distribution_tables_and_files(monkeypatch, dumps, tmp_path, stream):
    calls = _restated(monkeypatch)
    monkeypatch.setattr(M, "STREAM", stream)
    monkeypatch.setattr(M, "BATCH_BYTES", 2 * 334 * 24)               # two frames per streamed batch
    traj = dumps["traj"]
    dist, pop = calc_dihedral_distribution(ENTRIES, dumps["pattern"], R.NUM_MOLS, R.ATOMS_PER_MOL, bin_size=5,
                                           working_dir=str(tmp_path))
    assert sum(c[0] for c in calls) == 6 and all(c[1:] == ((c[0], 3), 72, False) for c in calls)   # no series asked for
    assert (len(calls) == 3) if stream else (len(calls) == 1)
    assert list(dist.columns) == ["phi (deg)", "p_1:1-2-3-4", "p_backbone", "p_1:4-3-2-1"]
    assert np.array_equal(dist["phi (deg)"], -177.5 + 5.0 * np.arange(72))
    assert list(pop.columns) == ["dihedral", "g-", "g+", "t", "n", "n_degenerate"]
    assert pop["dihedral"].tolist() == ["1:1-2-3-4", "backbone", "1:4-3-2-1"]
    a0, mols, length, quads, rows, _ = R.entry_jobs([(1, [(1, 2, 3, 4)]), (2, ENTRIES[1][1]), (1, [(4, 3, 2, 1)])])
    hist, _, deg = R.dihedral_angles(traj["x"], traj["L"], a0, mols, length, quads, job_row=rows, n_bins=72)
    assert pop["n"].tolist() == hist.sum(axis=1).tolist() == [70 * 6, 3 * 9 * 6, 70 * 6] and not pop["n_degenerate"].any()
    for e, lab in enumerate(["1:1-2-3-4", "backbone", "1:4-3-2-1"]):
        assert np.array_equal(dist["p_" + lab], R.density(hist[e], 72))
        assert abs(dist["p_" + lab].sum() * 5.0 - 1.0) < 1e-14                               # integrates to 1
        for name, (lo, hi) in M.DEFAULT_STATES.items():
            assert pop[name][e] == R.population(hist[e], lo, hi, 72)
        assert abs(pop["g-"][e] + pop["g+"][e] + pop["t"][e] - 1.0) < 1e-15
    assert np.array_equal(dist["p_1:1-2-3-4"], dist["p_1:4-3-2-1"])                          # the reversed quadruple
    back = pd.read_csv(tmp_path / "dihedral_distribution.csv", index_col=0, float_precision="round_trip")
    assert list(back.columns) == list(dist.columns) and np.array_equal(back.to_numpy(), dist.to_numpy())
    back = pd.read_csv(tmp_path / "dihedral_populations.csv", index_col=0, float_precision="round_trip")
    assert list(back.columns) == list(pop.columns) and back["n"].tolist() == pop["n"].tolist()
    # unwrapped coordinates of the same frames: the same counts; windows that wrap through +-180; nothing written
    os.remove(tmp_path / "dihedral_distribution.csv"), os.remove(tmp_path / "dihedral_populations.csv")
    states = {"trans": (150, -150), "rest": (-150, 150), "upper": (90, 180), "all": (-180, 180)}
    dist_u, pop_u = calc_dihedral_distribution(ENTRIES, dumps["pattern"], R.NUM_MOLS, R.ATOMS_PER_MOL, bin_size=5,
                                               states=states, coords="unwrapped", save_mode=False)
    assert calls[-1][1] is None and not os.listdir(tmp_path)
    assert np.array_equal(dist_u.to_numpy(), dist.to_numpy())
    cnt = hist[1].astype(np.int64)
    assert pop_u["trans"][1] == (cnt[66:].sum() + cnt[:6].sum()) / cnt.sum() and pop_u["all"].tolist() == [1.0] * 3
    assert abs(pop_u["trans"][1] + pop_u["rest"][1] - 1.0) < 1e-15 and pop_u["upper"][1] == cnt[54:].sum() / cnt.sum()


def test_a_row_without_counts_and_degenerate_counts(monkeypatch, tmp_path):
    _restated(monkeypatch)
    traj = R.synthetic_trajectory(n_frames=2)
    x = traj["x"].copy()
    x[:, :, 2:280:4] = 2 * x[:, :, 1:280:4] - x[:, :, 0:280:4]        # every chain of type 1: atoms 1, 2, 3 collinear
    x[1, :, 280 + 6 * 4 + 3] = x[1, :, 280 + 6 * 4 + 2]               # one coincident pair in type 2
    traj = dict(traj, x=x, img=np.zeros_like(x), lo=traj["lo"] - 50.0, hi=traj["hi"] + 50.0)
    pattern = R.write_dumps(tmp_path, traj)
    dist, pop = calc_dihedral_distribution(ENTRIES[:2], pattern, R.NUM_MOLS, R.ATOMS_PER_MOL, bin_size=60, save_mode=False)
    assert np.isnan(dist["p_1:1-2-3-4"]).all() and np.isnan(pop.loc[0, ["g-", "g+", "t"]].to_numpy(dtype=float)).all()
    assert pop["n"].tolist() == [0, 3 * 9 * 2 - 3] and pop["n_degenerate"].tolist() == [140, 3]   # all three name the pair
    assert not os.path.exists(tmp_path / "dihedral_distribution.csv")


def test_correlation_table_of_a_two_state_series(monkeypatch, tmp_path):
    """Series that sit at phi = +60 or at 180 (a quarter of the time) and hop at random: C decays from 1 to the plateau
    p = <cos>^2 + <sin>^2 and Cn = (C - p) / (1 - p) from 1 to 0."""
    rng = np.random.default_rng(2)
    S, F = 40, 400
    state = np.zeros((S, F), dtype=bool)
    state[:, 0] = rng.random(S) < 0.25
    for t in range(1, F):                                              # hop rates 0.03 and 0.09: stationary share 1/4
        hop = rng.random(S) < np.where(state[:, t - 1], 0.09, 0.03)
        state[:, t] = state[:, t - 1] ^ hop
    phi = np.where(state, np.pi, np.pi / 3)
    U = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1)             # [S,3,F]
    off = np.array([0, 30, 40], dtype=np.int64)
    seen = {}

    def load(entries, filename, num_mols, per, dt, coords):
        seen.update(labels=[e[2] for e in entries], dt=dt, coords=coords)
        return U, 7.0 + 0.5 * np.arange(F), off, np.zeros(2, dtype=np.uint64)

    def orient_corr(U_, off_, max_lag, out=None, ctx=None):
        seen["max_lag"] = max_lag
        S1, S2, _, _ = RR.orient_truth(U_, off_, max_lag)
        return np.stack([S1, S2], axis=2)

    monkeypatch.setattr(M, "_load_series", load)
    monkeypatch.setattr(M, "refuse_triclinic", lambda filename: None)
    monkeypatch.setattr(backend, "orient_corr", orient_corr)
    entries = [(1, 1, 2, 3, 4), (2, [(1, 2, 3, 4), (3, 4, 5, 6)])]
    df = calc_dihedral_correlation(entries, "none.*", [30, 5], [4, 6], dt=2, working_dir=str(tmp_path))
    assert seen == {"labels": ["1:1-2-3-4", "2:1-2-3-4+1"], "dt": 2, "coords": "wrapped", "max_lag": 199}
    assert list(df.columns) == ["Time (ps)", "C_1:1-2-3-4", "Cn_1:1-2-3-4", "C_2:1-2-3-4+1", "Cn_2:1-2-3-4+1"]
    assert len(df) == 200 and np.array_equal(df["Time (ps)"], 0.5 * np.arange(200))
    S1 = RR.orient_truth(U, off, 199)[0]
    W = RR.windows(F, off, 199)
    for g, lab in enumerate(["1:1-2-3-4", "2:1-2-3-4+1"]):
        C = df["C_" + lab].to_numpy()
        assert np.array_equal(C, S1[:, g] / W[:, g]) and abs(C[0] - 1.0) < 1e-14
        grp = U[off[g]:off[g + 1]]
        p = grp[:, 0].mean() ** 2 + grp[:, 1].mean() ** 2
        assert np.array_equal(df["Cn_" + lab], (C - p) / (1.0 - p)) and 0.3 < p < 0.9
    C, Cn = df["C_1:1-2-3-4"].to_numpy(), df["Cn_1:1-2-3-4"].to_numpy()
    assert abs(Cn[0] - 1.0) < 1e-14 and abs(Cn[60:].mean()) < 0.1 < C[60:].mean()        # the plateau is removed
    back = pd.read_csv(tmp_path / "dihedral_correlation.csv", index_col=0, float_precision="round_trip")
    assert list(back.columns) == list(df.columns) and np.array_equal(back.to_numpy(), df.to_numpy())
    os.remove(tmp_path / "dihedral_correlation.csv")
    assert len(calc_dihedral_correlation(entries, "none.*", [30, 5], [4, 6], max_lag=399, save_mode=False)) == 400
    for bad in (-1, 400):
        with pytest.raises(ValueError, match="max_lag"):
            calc_dihedral_correlation(entries, "none.*", [30, 5], [4, 6], max_lag=bad, save_mode=False)
    assert not os.listdir(tmp_path)
    # a torsion that never moves: p == 1 and Cn is NaN; a degenerate one is refused by name
    U[:30] = U[0:1, :, 0:1]
    df = calc_dihedral_correlation(entries, "none.*", [30, 5], [4, 6], max_lag=5, save_mode=False)
    if float(U[:30, 0].mean()) ** 2 + float(U[:30, 1].mean()) ** 2 == 1.0:
        assert np.isnan(df["Cn_1:1-2-3-4"]).all()
    monkeypatch.setattr(M, "_load_series", lambda *a: (U, np.arange(F) * 1.0, off, np.array([0, 3], dtype=np.uint64)))
    with pytest.raises(ValueError, match=r"2:1-2-3-4\+1 \(3\)"):
        calc_dihedral_correlation(entries, "none.*", [30, 5], [4, 6], save_mode=False)
