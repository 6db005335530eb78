"""
StructuralRelaxation without a GPU: the numpy restatement of mdhip_self_relaxation (tests/relaxation_ref.py) against a
plain Python loop on hand systems (the crossing cases and the fractional walk of the displacement tests), the host
logic of the class with backend.self_relaxation replaced by the restatement (column names, the default max_lag, dict
and scalar forms of q and a, CSV files, the 1/e interpolation, the chi4 peak, the nonfinite ValueError), chi4 from
counts near 2^40 whose float64 numerator would be wrong, every ValueError of backend.self_relaxation (raised before
the library is called), the ABI triple (header, ctypes table, build recipe) and the compiler's resource report of the
kernels: no scratch.
"""
import math
import os
import re
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

import displacement_ref as D
import relaxation_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- restatement == loops ---------------------------------------------------------------------------------------------

def _same_as_loops(x, box, off, max_lag, stride, a, q):
    got = R.self_relaxation(x, box, off, max_lag, stride, a, q)
    want = R.self_relaxation_loops(x, box, off, max_lag, stride, a, q)
    for k in range(max_lag + 1):
        for g in range(len(off) - 1):
            o, c1, c2, fs, bad = want[k][g]
            assert (int(got[0][k]), int(got[1][k, g]), int(got[2][k, g]), [int(v) for v in got[3][k, g]],
                    int(got[4][k, g])) == (o, c1 if a is not None else 0, c2 if a is not None else 0, fs, bad), (k, g)


@pytest.mark.parametrize("stride", [1, 2, 5, 11, 12])
def test_restatement_is_the_loops(stride):
    x, box, _ = D.fractional_walk(3, 12, 9, max_step=0.2)
    off = [0, 4, 4, 9]
    _same_as_loops(x, box, off, 11, stride, [1.5, 1.0, 6.0], [[0.3, 2.0], [0.0, 1.0], [4.0, 0.7]])
    _same_as_loops(x, box, off, 5, stride, None, [0.9])
    _same_as_loops(x, box, off, 0, stride, 2.0, None)
    _same_as_loops(x, None, off, 11, stride, 40.0, [0.05])


def test_restatement_on_the_crossing_cases():
    """The grid walk of the displacement tests: steps of up to 0.45 box edges, a box per frame, NaN in one entity."""
    x, box = D.grid_walk(5, 10, 6)
    x[4, 1, 2] = np.nan
    x[7, 0, 5] = np.inf
    _same_as_loops(x, box, [0, 3, 6], 9, 1, 3.0, [0.5])
    got = R.self_relaxation(x, box, [0, 3, 6], 9, 1, 3.0, [0.5])
    assert got[4][0].tolist() == [1, 1] and got[4][:, 0].sum() > 1


def test_wrapped_walk_is_the_true_walk():
    """Integer coordinates in an integer box, steps of at most 3 (below half an edge), a * a = 10.5 between integers:
    every xu and rsq is exact, so the wrapped trajectory gives what the true unwrapped walk gives, ==."""
    rng = np.random.default_rng(9)
    box = np.tile(np.array([8.0, 9.0, 11.0]), (30, 1))
    steps = rng.integers(-3, 4, size=(30, 3, 12))
    steps[0] = rng.integers(0, 8, size=(3, 12))
    true = np.cumsum(steps, axis=0).astype(np.float64)
    x = np.mod(true, box[:, :, None])
    a = R.self_relaxation(x, box, [0, 5, 12], 29, 1, math.sqrt(10.5), [0.5])
    b = R.self_relaxation(true, None, [0, 5, 12], 29, 1, math.sqrt(10.5), [0.5])
    assert D.image_counts(x, box)[1] > 0
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert a[1][1:].any() and (a[1][5:] < a[0][5:, None] * np.array([5, 7], dtype=np.uint64)).all()  # (some moved beyond a)


# ---- the class on dumps, the library call replaced by the restatement ---------------------------------------------

TYPES = np.array([1] * 12 + [2] * 20 + [3] * 8)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("relaxation_dumps"))
    x, box, true = D.fractional_walk(13, 16, 40, max_step=0.05)
    return D.write_dumps(path, x, true, box, TYPES), x, box


@pytest.fixture()
def S(monkeypatch):
    from mdproptools_amd import backend
    from mdproptools_amd.dynamical import relaxation

    calls = []

    def fake(r, box, group_off, max_lag, origin_stride=1, a=None, q=None, ctx=None):
        calls.append(dict(box=box, max_lag=max_lag, stride=origin_stride, a=a, q=q))
        return R.self_relaxation(r, box, group_off, max_lag, origin_stride, a, q)

    monkeypatch.setattr(backend, "self_relaxation", fake)
    return types.SimpleNamespace(cls=relaxation.StructuralRelaxation, mod=relaxation, calls=calls)


def test_constructor_and_export():
    import inspect

    from mdproptools_amd.dynamical.relaxation import StructuralRelaxation

    p = inspect.signature(StructuralRelaxation.__init__).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [
        ("atom_types", inspect.Parameter.empty), ("filename", inspect.Parameter.empty), ("dt", 1), ("save_mode", True),
        ("working_dir", None), ("coords", "wrapped")]
    with pytest.raises(ValueError):
        StructuralRelaxation([1], "x", coords="scaled")
    with pytest.raises(ValueError):
        StructuralRelaxation(list(range(17)), "x")


def test_columns_default_max_lag_and_files(S, dumps, tmp_path):
    pattern, x, box = dumps
    s = S.cls([2, 1], pattern, dt=2, working_dir=str(tmp_path))
    df = s.calc_relaxation(q={2: [0.5, 1.0], 1: [2.0, 0.25]}, a={2: 1.5, 1: 2.5})
    assert df is s.relax_df
    assert list(df.columns) == ["Time (ps)", "origins", "Fs_2_q0.5", "Fs_2_q1", "Q_2", "chi4_2", "Fs_1_q2",
                                "Fs_1_q0.25", "Q_1", "chi4_1"]
    call, = S.calls
    assert call["max_lag"] == 7 and call["stride"] == 1            # 16 frames: (F - 1) // 2
    assert call["a"] == [1.5, 2.5] and call["q"] == [[0.5, 1.0], [2.0, 0.25]]
    r, rbox, off, _ = D.read_dumps(pattern, [2, 1], ["x", "y", "z"])
    assert np.array_equal(call["box"], rbox)
    want = R.tables(r, rbox, off, [2, 1], 100 * 2e-3, 7, 1, {2: 1.5, 1: 2.5}, {2: [0.5, 1.0], 1: [2.0, 0.25]})
    for c in want:
        assert np.array_equal(np.asarray(df[c]), np.asarray(want[c])), c
    assert df["origins"].tolist() == list(range(16, 8, -1)) and np.allclose(df["Time (ps)"], 0.2 * np.arange(8))
    assert (df["Fs_2_q0.5"][0], df["Q_2"][0], df["chi4_2"][0]) == (1.0, 1.0, 0.0)
    csv = pd.read_csv(tmp_path / "relaxation.csv", index_col=0)
    assert list(csv.columns) == list(df.columns) and np.allclose(csv.to_numpy(), df.to_numpy(dtype=float), rtol=1e-12)
    times = s.calc_relaxation_times()
    assert list(times.columns) == ["type", "q", "tau_alpha (ps)", "tau_Q (ps)", "t_star (ps)", "chi4_max"]
    assert times["type"].tolist() == [2, 2, 2, 1, 1, 1] and len(times) == 6
    assert (tmp_path / "relaxation_times.csv").exists()


def test_scalar_forms_unwrapped_stride_and_save_mode(S, dumps, tmp_path):
    pattern, x, box = dumps
    s = S.cls([3, 1], pattern, dt=2, save_mode=False, working_dir=str(tmp_path), coords="unwrapped")
    df = s.calc_relaxation(q=0.75, max_lag=15, origin_stride=4)
    call = S.calls[-1]
    assert call["box"] is None and call["a"] is None and call["q"] == [[0.75], [0.75]] and call["stride"] == 4
    assert list(df.columns) == ["Time (ps)", "origins", "Fs_3_q0.75", "Fs_1_q0.75"]
    assert df["origins"].tolist() == [4, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1]
    df = s.calc_relaxation(a=2.0, max_lag=3)
    assert S.calls[-1]["q"] is None and S.calls[-1]["a"] == [2.0, 2.0]
    assert list(df.columns) == ["Time (ps)", "origins", "Q_3", "chi4_3", "Q_1", "chi4_1"]
    df = s.calc_relaxation(q=[0.5, 1.5, 2.5, 3.5], a={3: 1.0, 1: 2.0}, max_lag=2)
    assert len(df.columns) == 2 + 2 * (4 + 2)
    times = s.calc_relaxation_times()
    assert len(times) == 10
    assert os.listdir(tmp_path) == []
    for kw in (dict(), dict(q=[1, 2, 3, 4, 5]), dict(q={3: 1.0}), dict(q=[1.0, 2.0, 1.0]),
               dict(q={3: [0.5, 0.7], 1: [1.0000001, 1.0000002]}), dict(a=[1.0, 2.0]), dict(a={1: 2.0}),
               dict(q={3: [1.0], 1: [1.0, 2.0]}), dict(q=1.0, max_lag=16), dict(q=1.0, max_lag=-1)):
        with pytest.raises(ValueError):
            s.calc_relaxation(**kw)
    with pytest.raises(ValueError):
        S.cls([1], pattern).calc_relaxation_times()   # nothing computed yet


def test_displacement_uses_the_same_loader(dumps):
    from mdproptools_amd.common import trajectory
    from mdproptools_amd.dynamical.relaxation import StructuralRelaxation
    from mdproptools_amd.dynamical.residence_time import Displacement

    pattern, x, box = dumps
    a = Displacement([2, 1], {}, pattern, dt=2)._load()
    b = StructuralRelaxation([2, 1], pattern, dt=2)._load()
    c = trajectory.load_typed_positions(pattern, [2, 1], "wrapped", 2e-3)
    for u, v, w in zip(a, b, c):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    assert a[2].tolist() == [0, 20, 32] and a[3] == 100 * 2e-3


def test_first_crossing_interpolates_between_the_two_lags():
    from mdproptools_amd.dynamical.relaxation import first_crossing

    t = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    e = math.exp(-1.0)
    assert first_crossing(t, [1.0, 0.8, 0.5, 0.3, 0.1], e) == 2.0 + (0.5 - e) / (0.5 - 0.3)
    assert first_crossing(t, [1.0, 0.5, 0.2, 0.6, 0.1], 0.35) == 1.5            # the FIRST crossing
    assert math.isnan(first_crossing(t, [1.0, 0.9, 0.8, 0.7, 0.6], e))           # never crosses
    assert math.isnan(first_crossing(t, [1.0, 0.9, e, e, e], e))                 # reaches, never falls below
    assert first_crossing(t, [0.2, 0.1, 0.0, 0.0, 0.0], e) == 0.0
    assert math.isnan(first_crossing(t, [1.0, np.nan, np.nan, np.nan, np.nan], e))


def test_relaxation_times_on_a_hand_made_curve(S, tmp_path):
    s = S.cls([5, 7], "unused", working_dir=str(tmp_path))
    t = 0.5 * np.arange(6)
    s._q = [[1.0], [1.0]]
    s.relax_df = pd.DataFrame({
        "Time (ps)": t, "origins": [6, 5, 4, 3, 2, 1],
        "Fs_5_q1": [1.0, 0.7, 0.4, 0.2, 0.1, 0.05], "Q_5": [1.0, 0.9, 0.3, 0.2, 0.1, 0.0],
        "chi4_5": [0.0, 0.5, 2.5, 1.0, 0.2, 0.0],
        "Fs_7_q1": [1.0, 0.99, 0.98, 0.97, 0.96, 0.95], "Q_7": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
        "chi4_7": [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]})
    out = s.calc_relaxation_times()
    e = float(np.exp(-1.0))   # the level the class uses
    row = out[(out["type"] == 5) & (out["q"] == 1.0)].iloc[0]
    # 0.4 is still above 1/e = 0.368: the crossing lies between lags 2 and 3
    assert row["tau_alpha (ps)"] == 1.0 + 0.5 * (0.4 - e) / (0.4 - 0.2) and math.isnan(row["tau_Q (ps)"])
    row = out[(out["type"] == 5) & out["q"].isna()].iloc[0]
    assert row["tau_Q (ps)"] == 0.5 + 0.5 * (0.9 - e) / (0.9 - 0.3)
    assert (row["t_star (ps)"], row["chi4_max"]) == (1.0, 2.5)
    seven = out[out["type"] == 7]
    assert math.isnan(seven.iloc[0]["tau_alpha (ps)"]) and math.isnan(seven.iloc[1]["tau_Q (ps)"])
    assert (seven.iloc[1]["t_star (ps)"], seven.iloc[1]["chi4_max"]) == (0.0, 0.0)
    assert (tmp_path / "relaxation_times.csv").exists()


def test_nonfinite_counts_raise(S, dumps, monkeypatch):
    from mdproptools_amd import backend

    pattern, x, box = dumps

    def fake(r, box, group_off, max_lag, origin_stride=1, a=None, q=None, ctx=None):
        out = R.self_relaxation(r, box, group_off, max_lag, origin_stride, a, q)
        out[4][3:, 1] = 2
        return out

    monkeypatch.setattr(backend, "self_relaxation", fake)
    with pytest.raises(ValueError, match=r"type 1: 2 displacements at lag 3 .*not finite"):
        S.cls([2, 1], pattern, save_mode=False).calc_relaxation(q=1.0)


def test_chi4_is_formed_in_exact_integers():
    """O = 2^20 + 1 origins and counts near 2^40 (count1 = 2^39, count2 = 2^58): O count2 and count1^2 are near 2^78 and
    differ by 36 O = 3.8e7 — about the 2^26 spacing of float64 there, so the float64 difference is wrong."""
    from mdproptools_amd.dynamical.relaxation import chi4_exact

    O, N = (1 << 20) + 1, 1 << 20
    n = [(1 << 19) + (3 if i % 2 else -3) for i in range(4)]         # what a few origins hold; the rest hold 2^19
    c1 = (O - 4) * (1 << 19) + sum(n)
    c2 = (O - 4) * (1 << 38) + sum(v * v for v in n)
    assert 1 << 39 <= c1 < 1 << 41 and O * c2 > 1 << 78
    exact = O * c2 - c1 * c1
    assert exact == O * 36 and float(O) * float(c2) - float(c1) * float(c1) != exact   # the float numerator is wrong
    got = chi4_exact(np.array([O, 1, 0], dtype=np.uint64), np.array([c1, 5, 0], dtype=np.uint64),
                     np.array([c2, 25, 0], dtype=np.uint64), N)
    assert got[0] == exact / (O * O * N) and got[0] == 36 / (O * N)
    assert got[1] == 0.0 and got[2] == 0.0                            # one origin, or none: no variance
    assert chi4_exact(np.array([2], dtype=np.uint64), np.array([3], dtype=np.uint64), np.array([5], dtype=np.uint64),
                      2)[0] == (2 * 5 - 9) / (4 * 2)


# ---- the backend wrapper ----------------------------------------------------------------------------------------------

def test_backend_checks_before_the_library(monkeypatch):
    from mdproptools_amd import backend

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(backend, "default_context", boom)
    r = np.zeros((4, 3, 5))
    ok = dict(box=np.ones((4, 3)), group_off=[0, 2, 5], max_lag=3, origin_stride=1, a=1.0, q=[0.5, 1.0])

    def bad(**kw):
        c = dict(ok, **kw)
        with pytest.raises(ValueError):
            backend.self_relaxation(c.pop("r", r), c["box"], c["group_off"], c["max_lag"], c["origin_stride"], c["a"],
                                    c["q"])

    bad(r=np.zeros((4, 2, 5)))
    bad(r=np.zeros((4, 15)))
    bad(r=np.zeros((0, 3, 5)), max_lag=0)
    bad(box=np.ones((3, 3)))
    bad(group_off=[0, 6])
    bad(group_off=[0, 3, 2])
    bad(group_off=[-1, 3])
    bad(group_off=[0])
    bad(group_off=list(range(0, 18)), r=np.zeros((4, 3, 20)))
    bad(max_lag=-1)
    bad(max_lag=4)
    bad(origin_stride=0)
    bad(a=None, q=None)
    bad(a=None, q=[])
    bad(a=-1.0)
    bad(a=float("nan"))
    bad(a=[1.0, 2.0, 3.0])
    bad(q=[-0.5])
    bad(q=[float("inf")])
    bad(q=[float("nan")])
    bad(q=[1, 2, 3, 4, 5])
    bad(q=[[1.0], [2.0], [3.0]])
    bad(q=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="origin_stride"):      # 2^15 origins of 2^15 entities: the guard, by its remedy
        backend.self_relaxation(np.broadcast_to(np.zeros(1), (1 << 15, 3, 1 << 15)), None, [0, 1 << 15], 0, 1, 1.0)
    with pytest.raises(AssertionError, match="the library was reached"):
        backend.self_relaxation(np.broadcast_to(np.zeros(1), (1 << 15, 3, (1 << 15) - 1)), None, [0, (1 << 15) - 1], 0, 1,
                                1.0)
    for kw in (dict(), dict(a=None), dict(q=None), dict(a=[1.0, 2.0], q=[[1.0], [2.0]]), dict(box=None),
               dict(origin_stride=1 << 70)):   # (any stride beyond F - 1 is handed over as F)
        c = dict(ok, **kw)
        with pytest.raises(AssertionError, match="the library was reached"):
            backend.self_relaxation(r, c["box"], c["group_off"], c["max_lag"], c["origin_stride"], c["a"], c["q"])


# ---- header == ctypes table == build recipe; the kernels' resources -----------------------------------------------

def test_abi_and_build_recipe():
    from mdproptools_amd import _lib, build

    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    m = re.search(r"int mdhip_self_relaxation\(([^;]*)\);", text)
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    restype, argtypes = _lib.PROTOTYPES["mdhip_self_relaxation"]
    assert len(params) == len(argtypes) == 18
    assert "relaxation.hip" in build.SOURCES
    for h in ("relaxation_plan.h", "image_counts.h", "fixed_point.h"):
        assert os.path.join(build.CSRC, h) in build.HEADERS          # (their changes rebuild the library)
    assert "2^-34" in text and "2^-8" in text                          # the promise and the switch point are stated
    plan = open(os.path.join(build.CSRC, "relaxation_plan.h")).read()
    for name, value in (("TO", R.TO), ("CELLS", R.CELLS), ("EB", R.EB)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), plan), name
    assert R.TK == R.TO * 0 + (256 // R.TO) * R.CELLS


def test_kernels_use_no_scratch():
    """The compiler's resource report (the assembly's metadata, as tests/test_codegen_cpu.py reads it): every kernel of
    relaxation.hip without scratch and without a spilled register; the LDS-window instances within 168 registers (three
    workgroups per CU is what their 48 KiB of LDS allow)."""
    import test_codegen_cpu as CG

    text = CG._asm("relaxation.hip")
    kern = CG._kernels(text)
    tiles = {k: meta for k, (_, meta) in kern.items() if "rx_tile_kernel" in k}
    assert len(tiles) == 10
    for k, (_, meta) in kern.items():
        assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, (k, meta)
    for k, meta in tiles.items():
        if k.endswith("ELb1EEEvNS_6RxArgsE"):
            assert int(meta["vgpr_count"]) <= 168, (k, meta)
    assert len(re.findall(r"\.amdhsa_group_segment_fixed_size 49152\b", text)) == 5   # the five window instances' LDS
