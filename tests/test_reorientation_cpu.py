"""
Host side of `Reorientation` (mdproptools_amd/dynamical/reorientation.py) and the numpy restatement the GPU tests
compare against (tests/reorientation_ref.py); no GPU. The two library calls are replaced by the restatement where a
method needs them, so what is checked here is the host code around them: arguments, labels, tables, files, fits.
"""
import inspect
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

import reorientation_ref as R
from conftest import REPO
from mdproptools_amd import backend
from mdproptools_amd.common import trajectory as T
from mdproptools_amd.dynamical import reorientation as M
from mdproptools_amd.dynamical.reorientation import Reorientation


def test_signature():
    assert str(inspect.signature(Reorientation)) == (
        "(vectors, filename, num_mols, num_atoms_per_mol, dt=1, working_dir=None, coords='wrapped')")
    corr = inspect.signature(Reorientation.calc_correlation).parameters
    assert list(corr)[:2] == ["self", "max_lag"] and corr["max_lag"].default is None
    relax = inspect.signature(Reorientation.calc_relaxation_times).parameters
    assert list(relax) == ["self", "t_cut", "fit_floor"]
    assert relax["t_cut"].default is None and relax["fit_floor"].default == math.exp(-2)
    r = Reorientation([(1, 1, 2)], "none.*", [4], [3], dt=2, working_dir="/somewhere")
    assert r.dt == 2e-3 and r.working_dir == "/somewhere" and r.coords == "wrapped" and r.save_mode is True
    assert Reorientation([(1, 1, 2)], "none.*", [4], [3]).working_dir == os.getcwd()


@pytest.mark.parametrize("vectors", [
    [(0, 1, 2)], [(3, 1, 2)],                 # molecule type out of range
    [(1, 0, 2)], [(1, 1, 4)], [(2, 6, 1)],    # tail or head outside the molecule
    [(1, 2, 2)],                              # tail == head
    [(1, 1, 2)] * 17,                         # more than 16 vectors
    [], [(1, 1)], [(1, "quadrupole")], [(1, 1, 2, 3)],
])
def test_bad_vectors_are_value_errors(vectors):
    with pytest.raises(ValueError):
        Reorientation(vectors, "none.*", [4, 2], [3, 5])


def test_other_host_errors():
    with pytest.raises(ValueError):
        Reorientation([(1, 1, 2)], "none.*", [4, 2], [3, 5], coords="scaled")
    with pytest.raises(ValueError):
        Reorientation([(1, 1, 2)], "none.*", [4, 2], [3])
    with pytest.raises(ValueError):
        Reorientation([(2, "dipole")], "none.*", [4, 2], [3, 1])       # a one-atom molecule has no dipole about itself
    assert len(Reorientation([(1, 1, 2)] * 16, "none.*", [4, 2], [3, 5]).vectors) == 16
    r = Reorientation([(1, 1, 3), (2, "dipole"), (2, 5, 2)], "none.*", [4, 2], [3, 5])
    r._refuse_degenerate([0, 0, 0])
    with pytest.raises(ValueError, match=r"2:5-2 \(7\)") as err:
        r._refuse_degenerate([0, 0, 7])
    assert "1:1-3" not in str(err.value) and "2:dipole" not in str(err.value)
    assert r.degenerate.tolist() == [0, 0, 7]
    with pytest.raises(ValueError, match="same charges"):
        r._terms(np.array([0.1] * 12 + [1, 2, 3, 4, 5, 1, 2, 3, 4, 6.0]))


def test_labels_jobs_and_terms():
    r = Reorientation([(1, 1, 3), (2, "dipole"), (2, 5, 2), (1, 2, 1)], "none.*", [4, 2], [3, 5])
    assert r.labels == ["1:1-3", "2:dipole", "2:5-2", "1:2-1"]
    a0, mols, length = r._jobs()
    assert a0.tolist() == [0, 12, 12, 0] and mols.tolist() == [4, 2, 2, 4] and length.tolist() == [3, 5, 5, 3]
    q = np.array([0.0] * 12 + [9.0, 1.0, -2.0, 3.0, -4.0] * 2)
    # the first atom's term is dropped (it contributes zero); k ascends whatever the direction of the vector
    assert r._terms(q) == [[(2, 1.0)], [(1, 1.0), (2, -2.0), (3, 3.0), (4, -4.0)], [(1, 1.0), (4, -1.0)], [(1, -1.0)]]


def _with_restatement(monkeypatch, r, U, times, group_off):
    """The instance holds U already; the library's lag sums and running integral come from numpy."""
    r._traj = (U, np.asarray(times, dtype=np.float64), np.asarray(group_off, dtype=np.int64))
    calls = []

    def orient_corr(U_, off, max_lag, out=None, ctx=None):
        calls.append(("orient_corr", max_lag))
        S1, S2, _, _ = R.orient_truth(U_, off, max_lag)
        return np.stack([S1, S2], axis=2)

    def cumtrapz(y, dx, leading_zero=False, **kw):
        calls.append(("cumtrapz", y.shape, dx, leading_zero))
        steps = 0.5 * dx * (y[:, 1:] + y[:, :-1])
        return np.concatenate([np.zeros((len(y), 1))] * bool(leading_zero) + [np.cumsum(steps, axis=1)], axis=1)

    monkeypatch.setattr(backend, "orient_corr", orient_corr)
    monkeypatch.setattr(backend, "cumtrapz", cumtrapz)
    return calls


def test_table_and_csv_layout(monkeypatch, tmp_path):
    rng = np.random.default_rng(0)
    U = rng.normal(size=(6, 3, 21))
    U /= np.linalg.norm(U, axis=1)[:, None, :]
    r = Reorientation([(1, 1, 3), (2, "dipole")], "none.*", [4, 2], [3, 5], dt=2, working_dir=str(tmp_path))
    calls = _with_restatement(monkeypatch, r, U, 100.0 + 0.5 * np.arange(21), [0, 4, 6])
    df = r.calc_correlation()
    assert calls == [("orient_corr", 10)]                       # the default max_lag is (F - 1) // 2
    assert list(df.columns) == ["Time (ps)", "C1_1:1-3", "C2_1:1-3", "C1_2:dipole", "C2_2:dipole"]
    assert df is r.corr_df and len(df) == 11
    assert np.array_equal(df["Time (ps)"], 0.5 * np.arange(11))
    assert np.all(np.abs(df.iloc[0, 1:].to_numpy() - 1.0) <= 16 * R.EPS)   # unit vectors: C1(0) = C2(0) = 1 up to rounding
    S1, S2, _, _ = R.orient_truth(U, [0, 4, 6], 10)
    C1, C2 = R.correlation(S1, S2, R.windows(21, [0, 4, 6], 10))
    assert np.array_equal(df["C1_2:dipole"], C1[:, 1]) and np.array_equal(df["C2_1:1-3"], C2[:, 0])
    back = pd.read_csv(tmp_path / "reorientation.csv", index_col=0, float_precision="round_trip")
    assert list(back.columns) == list(df.columns) and np.array_equal(back.to_numpy(), df.to_numpy())
    assert len(r.calc_correlation(max_lag=20)) == 21 and len(r.calc_correlation(max_lag=0)) == 1
    for bad in (-1, 21):
        with pytest.raises(ValueError):
            r.calc_correlation(max_lag=bad)
    r.save_mode = False
    os.remove(tmp_path / "reorientation.csv")
    r.calc_correlation()
    r.calc_relaxation_times()
    assert not os.listdir(tmp_path)


def test_relaxation_times_of_exponentials(monkeypatch, tmp_path):
    t = 0.25 * np.arange(400)
    a1, tau1, a2, tau2 = 0.93, 7.5, 0.81, 2.75
    r = Reorientation([(1, 1, 2)], "none.*", [4], [3], working_dir=str(tmp_path))
    calls = _with_restatement(monkeypatch, r, None, t, [0, 4])
    r.corr_df = pd.DataFrame({"Time (ps)": t, "C1_1:1-2": a1 * np.exp(-t / tau1), "C2_1:1-2": a2 * np.exp(-t / tau2)})
    df = r.calc_relaxation_times()
    assert calls == [("cumtrapz", (2, 400), 0.25, True)]         # ONE call for every column
    assert df is r.relax_df and df["vector"].tolist() == ["1:1-2"] * 2 and df["rank"].tolist() == [1, 2]
    for row, (a, tau) in zip(df.itertuples(index=False), ((a1, tau1), (a2, tau2))):
        c = a * np.exp(-t / tau)
        run = int(np.argmin(c >= math.exp(-2)))
        assert row[6] == run and 2 <= run < 400
        assert abs(row[4] - tau) <= 1e-12 * tau, (row[4], tau)
        assert abs(row[5] - a) <= 1e-12 * a
        assert row[2] == t[-1]                                    # never <= 0: the last lag
        trapezoid = math.fsum(0.5 * 0.25 * (c[1:] + c[:-1]))
        assert abs(row[3] - trapezoid) <= 400 * R.EPS * trapezoid  # (399 additions, in whatever order)
    assert list(pd.read_csv(tmp_path / "reorientation_times.csv", index_col=0).columns) == [
        "vector", "rank", "t_cut (ps)", "tau_integral (ps)", "tau_fit (ps)", "amplitude", "fit_lags"]
    # an explicit t_cut is rounded down to a lag; the default stops at the first lag with C <= 0
    cut = r.calc_relaxation_times(t_cut=3.1)
    c = a1 * np.exp(-t / tau1)
    assert cut["t_cut (ps)"].tolist() == [3.0, 3.0]
    assert abs(cut["tau_integral (ps)"][0] - np.sum(0.125 * (c[1:13] + c[:12]))) <= 1e-14
    osc = np.cos(0.5 * t) * np.exp(-t / 9.0)
    r.corr_df = pd.DataFrame({"Time (ps)": t, "C1_1:1-2": osc, "C2_1:1-2": np.full(400, 0.05)})
    df = r.calc_relaxation_times()
    first = int(np.flatnonzero(osc <= 0)[0])
    assert df["t_cut (ps)"][0] == t[first]
    assert abs(df["tau_integral (ps)"][0] - np.sum(0.125 * (osc[1:first + 1] + osc[:first]))) <= 1e-14
    # fewer than two lags above the floor: no fit
    assert np.isnan(df["tau_fit (ps)"][1]) and np.isnan(df["amplitude"][1]) and df["fit_lags"][1] == 0
    strict = r.calc_relaxation_times(fit_floor=0.999)
    assert strict["fit_lags"][0] == 1 and np.isnan(strict["tau_fit (ps)"][0])


def test_restatement_on_a_uniformly_turning_molecule():
    """A diatomic turning by phi per frame about a fixed axis, seen through a wrapped box: C1(k) = cos k phi and
    C2(k) = (3 cos^2 k phi - 1) / 2 at every lag."""
    F, phi, L = 90, 0.173, 6.0
    f = np.arange(F)
    x = np.zeros((F, 3, 3))
    x[:, :, 0] = np.array([5.5, 0.25, 3.0])                               # next to the x and y faces
    bond = 1.1 * np.stack([np.cos(phi * f), np.sin(phi * f), np.zeros(F)], axis=1)
    x[:, :, 2] = np.mod(x[:, :, 0] + bond, L)                             # the head, folded into the box
    x[:, :, 1] = np.nan                                                   # an atom no term names
    box = np.full((F, 3), L)
    U, deg = R.axis_vectors(x, box, [0], [1], [3], [[(2, 1.0)]])
    assert U.shape == (1, 3, F) and deg.tolist() == [0]
    assert np.abs(U[0].T - bond / 1.1).max() < 1e-14
    S1, S2, A1, A2 = R.orient_truth(U, [0, 1], F - 1)
    C1, C2 = R.correlation(S1, S2, R.windows(F, [0, 1], F - 1))
    k = np.arange(F)
    assert np.abs(C1[:, 0] - np.cos(k * phi)).max() <= 1e-12
    assert np.abs(C2[:, 0] - (3 * np.cos(k * phi) ** 2 - 1) / 2).max() <= 1e-12
    assert np.all(A1 >= np.abs(S1) * (1 - 4 * R.EPS)) and A2 is S2   # (A1 adds the leading parts of c only)


def test_restatement_counts_integers_the_same_way_twice():
    """orient_sums_int (transform route and direct route) against orient_truth, and the degenerate / NaN rules of
    axis_vectors."""
    rng = np.random.default_rng(5)
    off = np.array([0, 0, 1, 9], dtype=np.int64)
    for n in (1, 2, 64, 65, 200):
        U = R.axis_series(rng, 9, n)
        S1, S2, A1, _ = R.orient_truth(U, off, n - 1)
        got = R.orient_sums_int(U, off, n - 1)
        assert np.array_equal(got[:, :, 0], S1) and np.array_equal(got[:, :, 1], S2) and np.array_equal(A1, S2)
        assert np.array_equal(S2[0], n * np.diff(off))
    x = np.zeros((2, 3, 4))
    x[0, :, 1] = [1e200, 0, 0]     # n2 overflows
    x[1, :, 3] = [0, 3.0, 4.0]
    U, deg = R.axis_vectors(x, None, [0], [2], [2], [[(1, 1.0)]])
    assert deg.tolist() == [2]                                            # (frame 1, molecule 0) and (frame 0, molecule 1)
    assert np.isnan(U[0, :, 0]).all() and not U[0, :, 1].any() and not U[1, :, 0].any()
    assert U[1, :, 1].tolist() == [0.0, 0.6, 0.8]
    assert R.same_bits(U, U.copy()) and not R.same_bits(np.array([0.0]), np.array([-0.0]))


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    for name in ("mdhip_axis_vectors", "mdhip_orient_corr"):
        assert re.search(r"\bint %s\s*\(mdhip_ctx \*ctx," % name, text), name
    assert "half a box edge" in text and "about the molecule's first atom" in text.replace("\n * ", " ")
    from mdproptools_amd import _lib, build

    assert {"mdhip_axis_vectors", "mdhip_orient_corr"} <= set(_lib.PROTOTYPES)
    assert "reorient.hip" in build.SOURCES


@pytest.mark.parametrize("stream", [False, True])
def test_attribute_batches_hand_out_the_box(tmp_path, stream):
    """`with_box` adds the edge lengths of every frame to the batches of either route and changes nothing else."""
    traj = R.synthetic_trajectory(n_frames=5)
    pattern = R.write_dumps(tmp_path, traj)
    streamed, batches = T.attribute_batches(pattern, ("q", "type"), ["x", "y", "z"], n_atoms=150, stream=stream,
                                            with_box=True)
    assert streamed == stream
    got = [tuple(np.array(part) for part in b) for b in batches]
    assert all(len(b) == 5 for b in got)
    steps, q, types, xyz, box = (np.concatenate([b[i] for b in got]) for i in range(5))
    assert steps.tolist() == traj["steps"].tolist()
    assert np.array_equal(box, traj["hi"] - traj["lo"]) and np.array_equal(xyz, traj["x"])
    assert np.array_equal(q[0], traj["q"]) and np.array_equal(types[-1], traj["types"])
    _, plain = T.attribute_batches(pattern, ("q", "type"), ["x", "y", "z"], n_atoms=150, stream=stream)
    assert all(len(b) == 4 for b in plain)


def test_module_keeps_its_switches():
    assert M.STREAM is True and M.BATCH_BYTES is None and M.MAX_VECTORS == 16
