"""
Displacement without a GPU: the numpy restatement of mdhip_displacement_hist (tests/displacement_ref.py) against a
plain Python loop and against a true unwrapped walk, the host logic of the class with backend.displacement_hist
replaced by the restatement (lag rounding, overlap, r_max, the CSV files, every ValueError), and the argument checks of
backend.displacement_hist, which raise before the library is called.
"""
import os
import types

import numpy as np
import pandas as pd
import pytest

import displacement_ref as R


def _hand_system():
    """7 frames, 5 atoms, box 8 x 8 x 8 (frame 4: 8.5): hand-placed crossings in both directions."""
    box = np.full((7, 3), 8.0)
    box[4] = 8.5
    x = np.zeros((7, 3, 5))
    x[:, 0, 0] = [7.0, 7.5, 0.25, 0.5, 8.25, 7.75, 0.5]   # out through +x, back, out again
    x[:, 0, 1] = [0.5, 7.75, 7.5, 0.25, 0.5, 0.75, 1.0]   # out through -x and back
    x[:, 1, 2] = [1.0, 5.0, 1.0, 5.0, 1.0, 5.0, 1.0]      # d == +-L/2 exactly (8.5 / 2 in frame 4): never shifts
    x[:, 2, 3] = [1.0, 5.5, 2.0, 6.5, 3.0, 7.5, 4.0]      # +4.5 shifts, -3.5 does not
    x[:, :, 4] = np.linspace(0.0, 3.0, 7)[:, None]        # never crosses
    x[:, 1, 0] = 3.0
    x[:, 2, 1] = [0.5, 0.5, 7.9, 7.9, 0.125, 0.125, 0.125]
    return x, box


def test_restatement_against_python_loops():
    x, box = _hand_system()
    off = np.array([0, 2, 2, 5])
    jobs = [(0, 1, 1), (0, 2, 2), (2, 3, 1), (2, 6, 1), (1, 1, 1), (2, 2, 3)]
    for bx in (box, None):
        for n_bins in (1, 7, 40):
            hist, overflow, windows, moments, crossings = R.displacement_hist(x, bx, off, jobs, 0.25, n_bins)
            want, want_cross = R.displacement_hist_loops(x, bx, off, jobs, 0.25, n_bins)
            assert crossings == want_cross
            for j, (h, ovf, win, m) in enumerate(want):
                assert hist[j].tolist() == h and int(overflow[j]) == ovf and int(windows[j]) == win
                assert np.allclose(moments[j], m, rtol=1e-14, atol=0.0)
    assert R.unwrap(x, box)[1] == 3 + 2 + 0 + 3 + 2  # atoms 0, 1, 2, 3 and the z column of atom 1
    assert windows.tolist() == [12, 6, 12, 3, 0, 6]
    n, _ = R.image_counts(x, box)
    assert n[:, 0, 0].tolist() == [0, 0, 1, 1, 0, 0, 1] and n[:, 0, 1].tolist() == [0, -1, -1, 0, 0, 0, 0]
    assert not n[:, 1, 2].any() and n[:, 2, 3].tolist() == [0, -1, -1, -2, -2, -3, -3]


def test_restatement_against_true_unwrapped_walk():
    x, box, true = R.fractional_walk(3, 400, 12)
    xu, crossings = R.unwrap(x, box)
    assert crossings > 100
    for k in (1, 7, 399):
        d, want = xu[k:] - xu[:-k], true[k:] - true[:-k]
        assert np.max(np.abs(d - want)) <= 1e-12 * np.max(np.abs(true))
    got = R.displacement_hist(x, box, [0, 12], [(0, 7, 1)], 0.5, 30)
    want = R.displacement_hist(true, None, [0, 12], [(0, 7, 1)], 0.5, 30)
    assert got[2] == want[2] and np.allclose(got[3], want[3], rtol=1e-12)


# ---- the class on dumps, the library call replaced by the restatement ---------------------------------------------

TYPES = np.array([1] * 20 + [2] * 30 + [3] * 10)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("displacement_dumps"))
    x, box, true = R.fractional_walk(11, 12, 60, max_step=0.1)
    return R.write_dumps(path, x, true, box, TYPES), x, box


@pytest.fixture()
def D(monkeypatch):
    from mdproptools_amd import backend
    from mdproptools_amd.dynamical import residence_time

    calls = []

    def fake(r, box, group_off, jobs, bin_size, n_bins, ctx=None):
        calls.append((None if box is None else np.array(box), np.array(jobs), bin_size, n_bins))
        return R.displacement_hist(r, box, group_off, jobs, bin_size, n_bins)

    monkeypatch.setattr(backend, "displacement_hist", fake)
    return types.SimpleNamespace(Displacement=residence_time.Displacement, calls=calls)


def _frames_equal(df, cols):
    assert list(df.columns) == list(cols)
    for c in cols:
        assert np.array_equal(np.asarray(df[c]), np.asarray(cols[c]), equal_nan=True), c


def test_constructor_is_the_references():
    import inspect

    from mdproptools_amd.dynamical.residence_time import Displacement

    p = inspect.signature(Displacement.__init__).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [
        ("atom_types", inspect.Parameter.empty), ("residence_time", inspect.Parameter.empty),
        ("filename", inspect.Parameter.empty), ("dt", 1), ("save_mode", True), ("working_dir", None),
        ("bin_size", 0.1), ("r_max", None), ("overlap", False), ("coords", "wrapped")]


@pytest.mark.parametrize("overlap", [False, True])
def test_calc_dist_lags_windows_and_files(D, dumps, tmp_path, overlap):
    pattern, x, box = dumps
    # frames are 100 steps of 2 fs apart: 0.2 ps. tau / delta = 2.5 -> 3 frames, 0.2 -> max(1, 0) = 1 frame
    tau = {2: 0.5, 1: 0.04}
    d = D.Displacement([2, 1], tau, pattern, dt=2, working_dir=str(tmp_path), bin_size=0.5, overlap=overlap)
    df = d.calc_dist()
    assert df is d.dist_df
    assert df["lag (frames)"].tolist() == [3, 1]
    assert df["windows"].tolist() == ([9 * 30, 11 * 20] if overlap else [3 * 30, 11 * 20])
    (bx, jobs, bin_size, n_bins), = D.calls
    assert jobs.tolist() == ([[0, 3, 1], [1, 1, 1]] if overlap else [[0, 3, 3], [1, 1, 1]])
    assert n_bins == int(np.ceil(0.5 * box.min() / 0.5)) and bin_size == 0.5  # r_max=None: half the smallest edge
    r, rbox, off, steps = R.read_dumps(pattern, [2, 1], ["x", "y", "z"])
    assert off.tolist() == [0, 30, 50] and np.array_equal(bx, rbox)
    want_dist, want_hist = R.dist_tables(r, rbox, off, [2, 1], tau, 100 * 2e-3, 0.5, n_bins, overlap)
    _frames_equal(df, want_dist)
    _frames_equal(d.hist_df, want_hist)
    assert list(df.columns) == ["type", "residence time (ps)", "lag (frames)", "windows", "mean distance",
                                "rms distance", "alpha2", "beyond r_max"]
    a = pd.read_csv(tmp_path / "displacement.csv", index_col=0)
    b = pd.read_csv(tmp_path / "displacement_distribution.csv", index_col=0)
    assert list(a.columns) == list(df.columns) and list(b.columns) == ["r", "2", "1"]
    assert np.allclose(a.to_numpy(), df.to_numpy(dtype=float), rtol=1e-12, equal_nan=True)
    assert np.allclose(b.to_numpy(), d.hist_df.to_numpy(), rtol=1e-12)
    # the densities integrate to the share of the windows inside r_max
    inside = 1.0 - df["beyond r_max"].to_numpy() / df["windows"].to_numpy()
    assert np.allclose(d.hist_df[[2, 1]].to_numpy().sum(axis=0) * 0.5, inside, rtol=1e-12)


def test_van_hove_unwrapped_r_max_and_save_mode(D, dumps, tmp_path):
    pattern, x, box = dumps
    d = D.Displacement([1, 3], {}, pattern, dt=2, save_mode=False, working_dir=str(tmp_path), bin_size=0.25,
                       r_max=3.1, coords="unwrapped")
    gs, a2 = d.calc_van_hove([0.2, 0.25, 1.0, 0.0, 2.2])  # 1, 1 (dropped), 5, 1 (dropped), 11 frames
    (bx, jobs, bin_size, n_bins), = D.calls
    assert bx is None and n_bins == 13
    assert jobs.tolist() == [[g, k, 1] for g in (0, 1) for k in (1, 5, 11)]
    r, rbox, off, steps = R.read_dumps(pattern, [1, 3], ["xu", "yu", "zu"])
    want_gs, want_a2 = R.van_hove_tables(r, None, off, [1, 3], [1, 5, 11], 100 * 2e-3, 0.25, 13)
    _frames_equal(a2, want_a2)
    assert list(gs) == [1, 3]
    for t in gs:
        _frames_equal(gs[t], want_gs[t])
    assert os.listdir(tmp_path) == []
    d.save_mode = True
    d.calc_van_hove([0.2])
    assert sorted(os.listdir(tmp_path)) == ["alpha2.csv", "van_hove_1.csv", "van_hove_3.csv"]
    d2 = D.Displacement([3], {3: 0.2}, pattern, dt=2, save_mode=False, working_dir=str(tmp_path / "none"))
    d2.calc_dist()
    assert not os.path.exists(tmp_path / "none")


def test_value_errors(D, dumps, tmp_path):
    from mdproptools_amd import io as mio

    pattern, x, box = dumps
    with pytest.raises(ValueError, match="type 2"):  # 12 frames: the longest lag is 11
        D.Displacement([1, 2], {1: 0.2, 2: 2.31}, pattern, dt=2, save_mode=False).calc_dist()
    D.Displacement([1, 2], {1: 0.2, 2: 2.29}, pattern, dt=2, save_mode=False).calc_dist()
    with pytest.raises(ValueError):
        D.Displacement([1], {}, pattern, dt=2, save_mode=False).calc_van_hove([2.4])
    with pytest.raises(ValueError):
        D.Displacement([1], {}, pattern, coords="scaled")

    def write(sub, steps, ids=None):
        os.makedirs(tmp_path / sub)
        for f, ts in enumerate(steps):
            table = np.column_stack([np.arange(1, 5) if ids is None else ids[f], [1, 1, 2, 2],
                                     np.full((4, 3), 0.5 + 0.1 * f)])
            mio.write_dump(str(tmp_path / sub / ("dump.%d.lammpstrj" % ts)), ts, [(0.0, 5.0)] * 3,
                           ["id", "type", "x", "y", "z"], table)
        return str(tmp_path / sub / "dump.*.lammpstrj")

    with pytest.raises(ValueError, match="uniform"):
        D.Displacement([1], {1: 0.1}, write("gap", [0, 100, 300]), save_mode=False).calc_dist()
    with pytest.raises(ValueError, match="same atom ids"):
        D.Displacement([1], {1: 0.1}, write("ids", [0, 100, 200], ids=[[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 5]]),
                       save_mode=False).calc_dist()
    with pytest.raises(ValueError, match="two frames"):
        D.Displacement([1], {1: 0.1}, write("one", [0]), save_mode=False).calc_dist()
    assert D.Displacement([1], {1: 0.1}, write("ok", [0, 100, 200]), save_mode=False).calc_dist()["windows"][0] == 4


def test_backend_checks_before_the_library(monkeypatch):
    from mdproptools_amd import backend

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(backend, "default_context", boom)
    r = np.zeros((4, 3, 5))
    ok = dict(box=np.ones((4, 3)), group_off=[0, 2, 5], jobs=[(0, 1, 1)], bin_size=0.1, n_bins=10)

    def bad(**kw):
        a = dict(ok, **kw)
        with pytest.raises(ValueError):
            backend.displacement_hist(a.pop("r", r), a["box"], a["group_off"], a["jobs"], a["bin_size"], a["n_bins"])

    bad(r=np.zeros((4, 2, 5)))
    bad(r=np.zeros((4, 15)))
    bad(box=np.ones((3, 3)))
    bad(box=np.ones((4, 2)))
    bad(group_off=[0, 6])
    bad(group_off=[0, 3, 2])
    bad(group_off=[-1, 3])
    bad(jobs=[(0, 1)])
    bad(jobs=[0, 1, 1])
    bad(jobs=[(2, 1, 1)])
    bad(jobs=[(-1, 1, 1)])
    bad(jobs=[(0, 0, 1)])
    bad(jobs=[(0, 4, 1)])
    bad(jobs=[(0, 1, 0)])
    bad(n_bins=0)
    bad(n_bins=(1 << 20) + 1)
    bad(bin_size=0.0)
    bad(bin_size=float("nan"))
    with pytest.raises(AssertionError, match="the library was reached"):
        backend.displacement_hist(r, ok["box"], ok["group_off"], ok["jobs"], 0.1, 10)
