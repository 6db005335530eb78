"""
mdhip_axis_vectors and mdhip_orient_corr (csrc/reorient.hip) and `Reorientation` on the GPU, against the numpy
restatement (tests/reorientation_ref.py).

The unit vectors are compared bit for bit: the header states every operation. The lag sums of series whose vectors are
+-e_x, +-e_y, +-e_z are integers and compared with `==`; those of random unit vectors within bounds derived from the
number of terms W of a sum and its absolute sum, never measured, and valid for any order of summation:
|S1 - truth| <= (W + 3) 2^-53 sum |c| (three roundings per c, W - 1 additions, and the truth's own) and
|S2 - truth| <= (W + 7) 2^-53 sum c^2 (two more per square). Shapes are the smallest at which the kernels can go wrong:
either side of the axis kernel's 64 x 64 tile, of the lag tile (1024), the time stage (128) and the lags per lane (4),
odd numbers of lag tiles, groups of no, one and more molecules than a slab (8) holds, 16 groups, and the two launch
dimensions beyond 65 535.
"""
import ctypes as C

import numpy as np
import pytest

import reorientation_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


# ---- axis vectors ------------------------------------------------------------------------------------------------------


def _check_axis(B, x, box, a0, mols, length, terms, want_deg=None):
    want, deg = R.axis_vectors(x, box, a0, mols, length, terms)
    U, got_deg = B.axis_vectors(x, box, a0, mols, length, terms)
    assert U.shape == want.shape
    bad = np.argwhere(~((U == want) | (np.isnan(U) & np.isnan(want))))
    print("series", U.shape[0], "frames", U.shape[2], "mismatches", len(bad), bad[:5].tolist())
    assert R.same_bits(U, want)
    assert got_deg.tolist() == deg.tolist()
    if want_deg is not None:
        assert got_deg.tolist() == list(want_deg)
    return U


def _molecules(rng, F, mols, per, L):
    """Wrapped coordinates [F,3,mols*per] of molecules about 2 wide placed anywhere in boxes L [F,3]."""
    centre = rng.random((F, 3, mols, 1)) * L[:, :, None, None]
    x = centre + rng.normal(0.0, 0.7, size=(F, 3, mols, per))
    return np.ascontiguousarray(np.mod(x, L[:, :, None, None]).reshape(F, 3, mols * per))


@pytest.mark.parametrize("mols", [1, 63, 64, 65])
@pytest.mark.parametrize("F", [1, 63, 65, 130])
def test_axis_vectors_either_side_of_the_tile(B, mols, F):
    rng = np.random.default_rng(1000 * mols + F)
    L = 9.0 + rng.random((F, 3))                                    # the box varies per frame and axis
    x = _molecules(rng, F, mols, 4, L)
    one = np.array([0], dtype=np.int64)
    U = _check_axis(B, x, L, one, [mols], [4], [[(1, -1.0), (3, 1.0)]], want_deg=[0])
    assert np.abs(np.sum(U * U, axis=1) - 1.0).max() < 1e-15
    if mols == 65 and F == 130:   # some molecule must have been put together across a face
        d = x[:, :, 3::4] - x[:, :, 1::4]
        assert (np.abs(d) > L[:, :, None] / 2).any()


def test_axis_vectors_a_job_without_molecules_between_two_others(B):
    """job_mols = (65, 0, 1): the empty job has no tile, and the tiles behind it still find their own job."""
    rng = np.random.default_rng(6501)
    F = 65
    L = 9.0 + rng.random((F, 3))
    x = _molecules(rng, F, 66, 4, L)
    U = _check_axis(B, x, L, [0, 260, 260], [65, 0, 1], [4, 4, 4], [[(1, -1.0), (3, 1.0)], [(2, 1.0)], [(1, 1.0)]],
                    want_deg=[0, 0, 0])
    assert U.shape == (66, 3, F) and np.abs(np.sum(U * U, axis=1) - 1.0).max() < 1e-15


def test_axis_vectors_at_the_faces(B):
    """d just above, exactly at and just below +-L/2 on every axis: the wrap is strict."""
    F = 7
    L = np.array([[8.0, 10.0, 12.0]] * F) + np.arange(F)[:, None] * 0.5
    half = L / 2
    cases = []
    for ax in range(3):
        for sign in (1.0, -1.0):
            for pick in (lambda h: h, lambda h: np.nextafter(h, np.inf), lambda h: np.nextafter(h, 0.0)):
                d = np.full((F, 3), 0.25)
                d[:, ax] = sign * pick(half[:, ax])
                cases.append(d)
    d = np.stack(cases, axis=2)                                        # [F,3,M]
    M = d.shape[2]
    x = np.zeros((F, 3, 2 * M))                                        # the first atom at the origin: d is x[a+1] itself
    x[:, :, 1::2] = d
    U = _check_axis(B, x, L, [0], [M], [2], [[(1, 1.0)]], want_deg=[0])
    # exactly at the half edge nothing shifts; just beyond it the image on the other side is taken
    assert np.all(np.sign(U[0::3, 0, :][:2]) == [[1.0], [-1.0]]) and np.all(np.sign(U[1::3, 0, :][:2]) == [[-1.0], [1.0]])


def test_axis_vectors_unwrapped_dipole_and_two_jobs_over_one_type(B):
    rng = np.random.default_rng(7)
    F, mols = 70, 37
    x = np.cumsum(rng.normal(0.0, 0.4, size=(F, 3, 5 * mols + 3 * 11)), axis=0) + rng.normal(0, 30, (1, 3, 1))
    a0 = np.array([0, 0, 5 * mols, 0], dtype=np.int64)
    terms = [[(1, 0.41), (3, -0.82), (4, 0.37)],      # a three-term dipole
             [(2, 1.0), (4, -1.0)],                   # a second job over the same molecules
             [(2, 1.0)],                              # another type
             [(1, -0.25), (2, 0.5), (3, -0.75), (4, 1.5)]]
    U = _check_axis(B, x, None, a0, [mols, mols, 11, mols], [5, 5, 3, 5], terms, want_deg=[0, 0, 0, 0])
    assert U.shape == (3 * mols + 11, 3, F)
    # a device tensor in and out gives the same bytes
    import torch

    dev = torch.device("cuda", B.default_context().device)
    out = torch.full((3 * mols + 11, 3, F), 7.0, dtype=torch.float64, device=dev)
    _, deg = B.axis_vectors(torch.as_tensor(x, device=dev), None, a0, [mols, mols, 11, mols], [5, 5, 3, 5], terms, out=out)
    assert out.cpu().numpy().tobytes() == U.tobytes() and not deg.any()


def test_axis_vectors_zero_vectors_and_nan(B):
    rng = np.random.default_rng(8)
    F, mols = 66, 70
    L = np.full((F, 3), 11.0)
    x = _molecules(rng, F, mols, 3, L)
    a0, terms = np.array([0, 0], dtype=np.int64), [[(2, 1.0)], [(1, 2.0), (2, -1.0)]]
    base = _check_axis(B, x, L, a0, [mols, mols], [3, 3], terms, want_deg=[0, 0])
    # a zero vector: counted, zeros out
    z = x.copy()
    z[5, :, 3 * 9 + 2] = z[5, :, 3 * 9]
    z[65, :, 3 * 69 + 2] = z[65, :, 3 * 69]
    U = _check_axis(B, z, L, a0, [mols, mols], [3, 3], terms, want_deg=[2, 0])
    assert not U[9, :, 5].any() and not U[69, :, 65].any()
    # a NaN in an atom no term names: no effect, bit for bit
    y = x.copy()
    y[:, :, 1::3] = np.nan
    U = _check_axis(B, y, L, a0[:1], [mols], [3], terms[:1], want_deg=[0])
    assert U.tobytes() == base[:mols].tobytes()
    # a NaN in a named atom: that series NaN at that frame, nothing counted, every other value unchanged
    y = x.copy()
    y[40, 1, 3 * 64 + 2] = np.nan
    U = _check_axis(B, y, L, a0, [mols, mols], [3, 3], terms, want_deg=[0, 0])
    hit = np.zeros(U.shape, dtype=bool)
    hit[64, :, 40] = hit[mols + 64, :, 40] = True
    assert np.isnan(U[hit]).all() and np.array_equal(U[~hit], base[~hit])
    # an overflowing n2 is not a direction either
    y = x.copy()
    y[3, 0, 2] = 1e300
    U = _check_axis(B, y, None, a0[:1], [mols], [3], [[(2, 1.0)]], want_deg=[0])
    assert np.isnan(U[0, :, 3]).all() and not np.isnan(U[1:]).any()


def test_axis_vectors_invalid_arguments(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    x = np.zeros((4, 3, 12))
    good = dict(n_jobs=2, a0=[0, 6], mols=[2, 2], length=[3, 3], t_off=[0, 2, 3], atom=[1, 2, 1], F=4, A=12)
    bad = [dict(n_jobs=0), dict(n_jobs=-1), dict(a0=[0, 7]), dict(mols=[2, 3]), dict(mols=[-1, 2]), dict(a0=[-1, 6]),
           dict(length=[3, 0]), dict(atom=[0, 2, 1]), dict(atom=[1, 3, 1]), dict(atom=[2, 1, 1]), dict(atom=[1, 1, 1]),
           dict(t_off=[0, 2, 2]), dict(t_off=[1, 2, 3]), dict(F=0), dict(A=0), dict(A=11),
           dict(null="x"), dict(null="U"), dict(null="degenerate"), dict(null="a0"), dict(null="mols"),
           dict(null="length"), dict(null="t_off"), dict(null="atom"), dict(null="w")]
    for change in bad:
        c = dict(good, **{k: v for k, v in change.items() if k != "null"})
        a0, mols = np.array(c["a0"], dtype=np.int64), np.array(c["mols"], dtype=np.int64)
        length, t_off = np.array(c["length"], dtype=np.int32), np.array(c["t_off"], dtype=np.int64)
        atom, w = np.array(c["atom"], dtype=np.int32), np.ones(3)
        U = np.full((4, 3, 4), 77.0)
        deg = np.full(2, 77, dtype=np.uint64)
        args = {"x": vp(x), "a0": ptr(a0, C.c_int64), "mols": ptr(mols, C.c_int64), "length": ptr(length, C.c_int32),
                "t_off": ptr(t_off, C.c_int64), "atom": ptr(atom, C.c_int32), "w": ptr(w), "U": vp(U),
                "degenerate": ptr(deg, C.c_uint64)}
        if "null" in change:
            args[change["null"]] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_axis_vectors(ctx.h, c["F"], c["A"], args["x"], 0, None, c["n_jobs"], args["a0"],
                                                 args["mols"], args["length"], args["t_off"], args["atom"], args["w"],
                                                 args["U"], 0, args["degenerate"]))
        assert err.value.code == -1, change
        assert (U == 77.0).all() and (deg == 77).all(), change
    # ... and the arguments these were derived from are fine
    U, deg = B.axis_vectors(x + np.arange(12.0), None, good["a0"], good["mols"], good["length"],
                            [[(1, 1.0), (2, 1.0)], [(1, 1.0)]])
    assert U.shape == (4, 3, 4) and not deg.any()


# ---- lag sums: exact integers ----------------------------------------------------------------------------------------------


def _exact(B, U, off, max_lag):
    want = R.orient_sums_int(U, off, max_lag)
    got = B.orient_corr(U, off, max_lag)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    print("n", U.shape[2], "lags", max_lag + 1, "mismatches", len(bad), bad[:5].tolist())
    assert np.array_equal(got, want)
    return got


OFF3 = np.array([0, 0, 1, 12], dtype=np.int64)   # an empty group, one molecule, eleven (a slab of 8 and one of 3)


@pytest.mark.parametrize("n", [1, 2, R.LPT + 1, R.TT - 1, R.TT, R.TT + 1, R.KT - 1, R.KT, R.KT + 1, R.KT + R.TT + 1,
                               2 * R.KT - 1, 2 * R.KT, 2 * R.KT + 1, 3 * R.KT - 5])
def test_exact_integers_at_every_lag(B, n):
    """max_lag = n - 1: one, two and three lag tiles (the middle one pairs with itself), every predicated step."""
    U = R.axis_series(np.random.default_rng(n), 12, n)
    got = _exact(B, U, OFF3, n - 1)
    assert not got[:, 0, :].any()
    assert np.array_equal(got[0, :, 1], n * np.diff(OFF3))


@pytest.mark.parametrize("max_lag", [0, 1, R.LPT - 1, R.LPT, R.KT - 2, R.KT - 1, R.KT, 2 * R.KT - 1, 2 * R.KT])
def test_exact_integers_at_some_lags(B, max_lag):
    """max_lag either side of the tile inside a longer series (n = 2 KT + TT + 3): the fast steps of every tile."""
    n = 2 * R.KT + R.TT + 3
    U = R.axis_series(np.random.default_rng(max_lag), 12, n)
    _exact(B, U, OFF3, max_lag)


def test_exact_integers_16_groups_and_the_same_bits_twice(B):
    rng = np.random.default_rng(16)
    sizes = [1, 0, 8, 9, 7, 16, 17, 2, 0, 3, 1, 1, 24, 5, 0, 4]
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    U = R.axis_series(rng, int(off[-1]), 1500)
    got = _exact(B, U, off, 1499)
    assert np.array_equal(got[0, :, 1], 1500.0 * np.array(sizes))
    assert B.orient_corr(U, off, 1499).tobytes() == got.tobytes()
    # series outside every group weigh nothing
    inner = np.array([3, 20, 41], dtype=np.int64)
    _exact(B, U, inner, 700)


def test_exact_integers_beyond_the_launch_limits(B):
    rng = np.random.default_rng(70001)
    U = R.axis_series(rng, 70001, 8)
    _exact(B, U, np.array([0, 40000, 70001], dtype=np.int64), 7)
    U = R.axis_series(rng, 2, 70001)
    _exact(B, U, np.array([0, 2], dtype=np.int64), 3)


def test_axis_vectors_beyond_the_launch_limits(B):
    """70 001 frames of three molecules, and one frame of 65 535 x 64 + 1 diatomics: one molecule tile more than a
    launch dimension holds, so the call takes two launches (as many frame tiles would take 4.2 million frames of any
    trajectory: the same loop, out of a test's reach)."""
    rng = np.random.default_rng(3)
    x = rng.normal(size=(70001, 3, 6))
    _check_axis(B, x, None, [0], [3], [2], [[(1, 1.0)]], want_deg=[0])
    mols = 65535 * R.TM + 1
    x = rng.random(size=(1, 3, 2 * mols)) + 0.5
    x[0, :, 2 * (mols - 1) + 1] = x[0, :, 2 * (mols - 1)]            # the last molecule, alone in the second launch
    U = _check_axis(B, x, None, [0], [mols], [2], [[(1, 1.0)]], want_deg=[1])
    assert not U[-1].any() and U[-2].any()


# ---- lag sums: floating point ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def units():
    rng = np.random.default_rng(21)
    U = rng.normal(size=(14, 3, 700))
    U[3:] = np.cumsum(U[3:], axis=2) + 10.0 * rng.normal(size=(11, 3, 1))     # these turn slowly; the first three jump
    U /= np.linalg.norm(U, axis=1)[:, None, :]
    off = np.array([0, 2, 11, 14], dtype=np.int64)
    S1, S2, A1, A2 = R.orient_truth(U, off, 699)
    return {"U": np.ascontiguousarray(U), "off": off, "S1": S1, "S2": S2, "A1": A1, "A2": A2,
            "W": R.windows(700, off, 699)}


def test_floating_point_within_the_derived_bounds(B, units):
    got = B.orient_corr(units["U"], units["off"], 699)
    W = units["W"]
    b1, b2 = (W + 3.0) * R.EPS * units["A1"], (W + 7.0) * R.EPS * units["A2"]
    e1, e2 = np.abs(got[:, :, 0] - units["S1"]), np.abs(got[:, :, 1] - units["S2"])
    print("S1: worst share of the bound", (e1 / b1).max(), "S2:", (e2 / b2).max())
    assert np.all(e1 <= b1) and np.all(e2 <= b2)
    assert B.orient_corr(units["U"], units["off"], 699).tobytes() == got.tobytes()
    import torch

    dev = torch.device("cuda", B.default_context().device)
    out = torch.full((700, 3, 2), 7.0, dtype=torch.float64, device=dev)
    B.orient_corr(torch.as_tensor(units["U"], device=dev), units["off"], 699, out=out)
    assert out.cpu().numpy().tobytes() == got.tobytes()


def test_a_nan_stays_in_its_group(B, units):
    clean = B.orient_corr(units["U"], units["off"], 699)
    U = units["U"].copy()
    U[6, 1, 350] = np.nan
    got = B.orient_corr(U, units["off"], 699)
    assert got[:, 0, :].tobytes() == clean[:, 0, :].tobytes() and got[:, 2, :].tobytes() == clean[:, 2, :].tobytes()
    assert np.isnan(got[0, 1, :]).all()
    # lags that never pair sample 350 with anything do not see it: k > 350 needs t + k = 350 or t = 350 < n - k
    assert np.isnan(got[:351, 1, :]).all() and not np.isnan(got[351:, 1, :]).any()


def test_orient_corr_invalid_arguments(B):
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    U = np.zeros((6, 3, 8))
    good = dict(n=8, S=6, G=2, off=[0, 3, 6], max_lag=3)
    bad = [dict(G=0), dict(G=17, off=list(range(18))), dict(n=0, max_lag=0), dict(n=1 << 29), dict(max_lag=8),
           dict(max_lag=-1), dict(off=[0, 4, 3]), dict(off=[0, 3, 7]), dict(off=[-1, 3, 6]), dict(S=-1),
           dict(null="U"), dict(null="off"), dict(null="sums")]
    for change in bad:
        c = dict(good, **{k: v for k, v in change.items() if k != "null"})
        off = np.array(c["off"], dtype=np.int64)
        sums = np.full((9, 17, 2), 77.0)
        args = {"U": vp(U), "off": ptr(off, C.c_int64), "sums": vp(sums)}
        if "null" in change:
            args[change["null"]] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_orient_corr(ctx.h, c["n"], c["S"], args["U"], 0, c["G"], args["off"], c["max_lag"],
                                                args["sums"], 0))
        assert err.value.code == -1, change
        assert (sums == 77.0).all(), change
    assert B.orient_corr(U, good["off"], 3).shape == (4, 2, 2)
    assert not B.orient_corr(np.zeros((0, 3, 8)), [0, 0], 7).any()      # no series at all: zeros


# ---- end to end ------------------------------------------------------------------------------------------------------------

VECTORS = [(1, 2, 3), (1, "dipole"), (2, 1, 5), (2, "dipole"), (2, 4, 2)]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("reorientation")
    traj = R.synthetic_trajectory()
    a0, mols, length, terms, off = R.vector_jobs(VECTORS)
    U, deg = R.axis_vectors(traj["x"], traj["hi"] - traj["lo"], a0, mols, length, terms)
    assert not deg.any()
    S1, S2, A1, A2 = R.orient_truth(U, off, 59)
    return {"dir": d, "pattern": R.write_dumps(d, traj), "traj": traj, "U": U, "off": off, "S1": S1, "S2": S2,
            "A1": A1, "A2": A2}


def _within_the_bounds(df, dumps, max_lag):
    """C1 and C2 of the table against the restatement's: the bounds of the sums divided by W, plus the roundings of the
    host's operations — one rounding of the division for C1; for C2 a product, a division and a subtraction on either
    side, each at most 2^-53 of an intermediate value of at most 1.5 S2 / W <= 1.5 (1 + 2^-50)."""
    W = R.windows(60, dumps["off"], max_lag)
    C1, C2 = R.correlation(dumps["S1"][: max_lag + 1], dumps["S2"][: max_lag + 1], W)
    b1 = (W + 3.0) * R.EPS * dumps["A1"][: max_lag + 1] / W + R.EPS * np.abs(C1)
    b2 = 1.5 * (W + 7.0) * R.EPS * dumps["A2"][: max_lag + 1] / W + 6 * R.EPS * 1.6
    worst = 0.0
    for g, v in enumerate(VECTORS):
        lab = "%d:dipole" % v[0] if v[1] == "dipole" else "%d:%d-%d" % v
        e1, e2 = np.abs(df["C1_" + lab].to_numpy() - C1[:, g]), np.abs(df["C2_" + lab].to_numpy() - C2[:, g])
        worst = max(worst, (e1 / b1[:, g]).max(), (e2 / b2[:, g]).max())
        assert np.all(e1 <= b1[:, g]) and np.all(e2 <= b2[:, g]), lab
    print("worst share of the bound", worst)


@pytest.mark.parametrize("stream", [True, False])
def test_reorientation_end_to_end(B, dumps, stream, monkeypatch):
    from mdproptools_amd.dynamical import reorientation as M

    traj = dumps["traj"]
    # molecules do cross faces: the wrapped coordinates of some bond differ by more than half an edge
    assert (np.abs(traj["x"][:, :, 2:75:3] - traj["x"][:, :, 1:75:3]) > traj["L"][:, :, None] / 2).any()
    monkeypatch.setattr(M, "STREAM", stream)
    monkeypatch.setattr(M, "BATCH_BYTES", 7 * 150 * 24)             # seven frames per streamed batch: nine batches
    r = M.Reorientation(VECTORS, dumps["pattern"], R.NUM_MOLS, R.ATOMS_PER_MOL, dt=2, working_dir=str(dumps["dir"]))
    df = r.calc_correlation()
    assert len(df) == 30 and np.array_equal(df["Time (ps)"], (500 * np.arange(30)).astype(np.float64) * 2e-3)
    U, times, off = r._load()
    assert R.same_bits(U.cpu().numpy(), dumps["U"]) and off.tolist() == dumps["off"].tolist()
    assert r.degenerate.tolist() == [0] * 5
    _within_the_bounds(df, dumps, 29)
    _within_the_bounds(r.calc_correlation(max_lag=59), dumps, 59)
    # unwrapped coordinates of the same trajectory: the same vectors bit for bit (every coordinate is a multiple of
    # 1 / 1024, so both routes form the same differences exactly)
    ru = M.Reorientation(VECTORS, dumps["pattern"], R.NUM_MOLS, R.ATOMS_PER_MOL, dt=2, working_dir=str(dumps["dir"]),
                         coords="unwrapped")
    ru.save_mode = False
    assert R.same_bits(ru._load()[0].cpu().numpy(), dumps["U"])
    # the relaxation times of the table, through the library's running integral
    relax = r.calc_relaxation_times()
    assert len(relax) == 10 and relax["vector"].tolist()[:2] == ["1:2-3", "1:2-3"]
    c = r.corr_df["C1_1:2-3"].to_numpy()
    i_cut = int(np.flatnonzero(c <= 0)[0]) if (c <= 0).any() else 59
    want = np.sum(0.5 * (c[1:i_cut + 1] + c[:i_cut])) * 1.0
    assert abs(relax["tau_integral (ps)"][0] - want) <= 1e-12 * max(1.0, abs(want))


def test_reorientation_refuses_what_has_no_direction(B, dumps, tmp_path):
    from mdproptools_amd.dynamical.reorientation import Reorientation

    traj = dict(dumps["traj"])
    x = traj["x"].copy()
    x[4, :, 3 * 7 + 2] = x[4, :, 3 * 7 + 1]          # atoms 2 and 3 of molecule 8 of type 1 coincide in frame 4
    traj["x"] = x
    pattern = R.write_dumps(tmp_path, traj, frames=range(8))
    r = Reorientation([(1, 1, 2), (1, 2, 3)], pattern, R.NUM_MOLS, R.ATOMS_PER_MOL, working_dir=str(tmp_path))
    with pytest.raises(ValueError, match=r"1:2-3 \(1\)"):
        r.calc_correlation()
    assert r.degenerate.tolist() == [0, 1]
    with pytest.raises(ValueError, match="q"):       # a dipole without charges in the dump
        other = tmp_path / "noq"
        other.mkdir()
        with open(tmp_path / "traj.0.dump") as fh, open(other / "traj.0.dump", "w") as out:
            for line in fh:
                parts = line.split()
                out.write(line.replace(" q ", " ") if line.startswith("ITEM: ATOMS") else
                          " ".join(parts[:2] + parts[3:]) + "\n" if len(parts) == 12 else line)
        Reorientation([(2, "dipole")], str(other / "traj.*.dump"), R.NUM_MOLS, R.ATOMS_PER_MOL,
                      working_dir=str(other)).calc_correlation()
