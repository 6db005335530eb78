"""
mdhip_self_relaxation (csrc/relaxation.hip) and the StructuralRelaxation drop-in on the GPU, against the numpy
restatement (tests/relaxation_ref.py). origins, count1, count2 and nonfinite by equality; the fixed-point sinc sums fs
within the bound derived in relaxation_ref.fs_bound of math.fsum of the float64 sinc terms — and by equality wherever
the terms are exactly 1 (q = 0, or nothing moves).

Shapes are the smallest at which the kernel can go wrong, from the constants of csrc/relaxation_plan.h (a tile is
TO = 32 origins x TK = 64 lags, a stage EB = 16 entities, a lane holds CELLS = 8 consecutive lags): frame counts 1, 2,
TO - 1 .. TO + 2, TK .. TK + 2, TO + TK, TO + TK + 1 and 2 TK + 1 with max_lag = F - 1 (origin and lag tiles that are
full, one short, one over); max_lag 0 and in the middle of a lane's run of lags; groups of 0, 1, EB - 1, EB, EB + 1 and
2 EB + 1 entities; 16 groups; n_q = 0, 1, 4; no overlap part; origin strides that do not divide F - 1 and that pass
F - 1, up to 2^63 - 1 (the route without the LDS window); 65 536 origin tiles (F = 2 097 122, one entity, lags 0 and 1) and 65 536 lag
tiles (F = 4 194 242, one entity, one origin per lag): one more than a launch dimension holds, both ways.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import displacement_ref as D
import relaxation_ref as R

pytestmark = pytest.mark.gpu

TO, TK, EB = R.TO, R.TK, R.EB


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _same_ints(got, want):
    for k, name in enumerate(("origins", "count1", "count2")):
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, name
        assert np.array_equal(got[k], want[k]), name
    assert got[4].dtype == np.uint64 and np.array_equal(got[4], want[4]), "nonfinite"
    assert got[3].dtype == np.int64 and got[3].shape == want[3].shape


def _check(got, r, box, off, max_lag, stride, a, q):
    """Integers == the restatement; fs within the derived bound of the fsum truth (exact rational arithmetic)."""
    want = R.self_relaxation(r, box, off, max_lag, stride, a, q, want_truth=True)
    _same_ints(got, want)
    truth, x_max = want[5], want[6]
    assert x_max.max(initial=0.0) <= 100.0
    bound = R.fs_bound(want[0], np.diff(np.asarray(off)), x_max)
    worst = 0.0
    for idx in np.ndindex(*truth.shape):
        err = abs(Fraction(int(got[3][idx]), R.UNIT) - Fraction(float(truth[idx])))
        lim = Fraction(float(bound[idx[0], idx[1]]))
        if lim:
            worst = max(worst, float(err / lim))
        assert err <= lim, (idx, float(err), float(lim))
    print("fs: largest error / bound = %.3g" % worst)
    return want


def _walk(seed, n_frames, n_ent, max_step=0.02):
    x, box, _ = D.fractional_walk(seed, n_frames, n_ent, max_step=max_step)
    return np.ascontiguousarray(x), box


@pytest.mark.parametrize("n_frames", [1, 2, TO - 1, TO, TO + 1, TO + 2, TK, TK + 1, TK + 2, TO + TK, TO + TK + 1,
                                      2 * TK + 1])
def test_frame_counts_around_the_tiles(B, n_frames):
    x, box = _walk(n_frames, n_frames, 21)
    off = np.array([0, 9, 9, 21])
    a, q = [2.0, 1.0, 3.5], [[0.4, 1.5], [0.0, 0.1], [2.5, 0.9]]
    got = B.self_relaxation(x, box, off, n_frames - 1, 1, a, q)
    _check(got, x, box, off, n_frames - 1, 1, a, q)
    assert got[0].tolist() == list(range(n_frames, 0, -1))


@pytest.mark.parametrize("max_lag", [0, 3, R.CELLS, TK - 1, TK])
def test_max_lag_inside_a_tile(B, max_lag):
    x, box = _walk(50 + max_lag, 90, 20)
    off = np.array([0, 20])
    got = B.self_relaxation(x, box, off, max_lag, 1, 1.5, [1.0])
    _check(got, x, box, off, max_lag, 1, 1.5, [1.0])


def test_group_sizes_around_the_stage(B):
    sizes = [0, 1, EB - 1, EB, EB + 1, 2 * EB + 1, 0]
    off = np.concatenate([[0], np.cumsum(sizes)])
    x, box = _walk(7, 70, int(off[-1]))
    a = [1.0 + 0.3 * g for g in range(len(sizes))]
    got = B.self_relaxation(x, box, off, 69, 1, a, [0.8, 2.0])
    _check(got, x, box, off, 69, 1, a, [0.8, 2.0])
    assert not got[1][:, 0].any() and not got[3][:, 0].any()   # the empty groups
    assert not got[1][:, 6].any() and not got[3][:, 6].any()


def test_sixteen_groups(B):
    off = np.arange(0, 17 * 3, 3)
    x, box = _walk(8, 40, 48)
    a = [0.5 + 0.25 * g for g in range(16)]
    q = [[0.1 * g, 1.0] for g in range(16)]
    got = B.self_relaxation(x, box, off, 39, 1, a, q)
    _check(got, x, box, off, 39, 1, a, q)


@pytest.mark.parametrize("n_q", [0, 1, 4])
def test_wave_number_counts(B, n_q):
    x, box = _walk(9 + n_q, 75, 40)
    off = np.array([0, 17, 40])
    q = None if n_q == 0 else [[0.0, 0.5, 1.7, 3.0][:n_q], [2.2, 0.3, 0.0, 1.1][:n_q]]
    got = B.self_relaxation(x, box, off, 74, 1, [2.0, 3.0], q)
    _check(got, x, box, off, 74, 1, [2.0, 3.0], q)
    assert got[3].shape == (75, 2, n_q)


def test_without_the_overlap_part(B):
    x, box = _walk(12, 70, 30)
    off = np.array([0, 30])
    got = B.self_relaxation(x, box, off, 40, 1, None, [1.2, 0.4])
    _check(got, x, box, off, 40, 1, None, [1.2, 0.4])
    assert not got[1].any() and not got[2].any()


@pytest.mark.parametrize("stride", [2, 3, 7, TO + 1, 69, 70, 75, 1 << 61, (1 << 62) + 1])
def test_origin_strides(B, stride):
    """F = 70: strides 3 and 7 divide F - 1 = 69 unevenly or evenly, 2 leaves a remainder, 69 = F - 1 has two origins at
    lag 0, 70 and 75 pass F - 1: one origin; so do 2^61 and 2^62 + 1, whose products with an origin index would
    overflow int64 (the library works with min(stride, F))."""
    x, box = _walk(20 + stride, 70, 35)
    off = np.array([0, 18, 35])
    for bx in (box, None):
        got = B.self_relaxation(x, bx, off, 69, stride, [2.5, 1.0], [[0.6], [1.4]])
        _check(got, x, bx, off, 69, stride, [2.5, 1.0], [[0.6], [1.4]])


def _lattice(seed, n_frames, n_ent):
    """Integer coordinates in an integer box, steps of at most 3 < half an edge: every xu and rsq is an exact integer."""
    rng = np.random.default_rng(seed)
    box = np.tile(np.array([8.0, 9.0, 11.0]), (n_frames, 1))
    steps = rng.integers(-3, 4, size=(n_frames, 3, n_ent))
    steps[0] = rng.integers(0, 8, size=(3, n_ent))
    xu = np.cumsum(steps, axis=0).astype(np.float64)
    return np.ascontiguousarray(np.mod(xu, box[:, :, None])), box, np.ascontiguousarray(xu)


@pytest.mark.parametrize("stride", [1, 4])
def test_integer_lattice_against_the_displacement_histogram(B, stride):
    """a * a = 10.5 lies between integers, so the strict compare has no edge case: the wrapped call == the unwrapped
    call, and count1[k] is bin 0 of mdhip_displacement_hist with bin_size = a for the job (g, k, stride)."""
    x, box, xu = _lattice(3, 80, 37)
    off = np.array([0, 20, 37])
    a = float(np.sqrt(10.5))
    assert 10.0 < a * a < 11.0
    wrapped = B.self_relaxation(x, box, off, 79, stride, a, [0.5])
    plain = B.self_relaxation(xu, None, off, 79, stride, a, [0.5])
    for u, v in zip(wrapped, plain):
        assert np.array_equal(u, v)
    _check(wrapped, x, box, off, 79, stride, a, [0.5])
    jobs = [(g, k, stride) for k in range(1, 80) for g in range(2)]
    hist, _, windows, _, _ = B.displacement_hist(x, box, off, jobs, a, 4)
    assert np.array_equal(hist[:, 0].reshape(79, 2), wrapped[1][1:])
    assert np.array_equal(windows.reshape(79, 2), wrapped[0][1:, None] * np.diff(off).astype(np.uint64)[None, :])


def test_exact_sums(B):
    """Nothing moves, or q = 0: every sinc term is exactly 1 and fs == W 2^32. At lag 0 every entity overlaps itself:
    count1 == O N and count2 == O N^2."""
    x, box = _walk(31, 100, 45)
    off = np.array([0, 13, 45])
    sizes = np.diff(off).astype(np.uint64)
    for stride in (1, 3):
        got = B.self_relaxation(x, box, off, 99, stride, 0.75, [0.0, 1.3])
        w = got[0][:, None] * sizes[None, :]
        assert np.array_equal(got[3][:, :, 0], (w * np.uint64(R.UNIT)).astype(np.int64))
        assert np.array_equal(got[1][0], got[0][0] * sizes) and np.array_equal(got[2][0], got[0][0] * sizes * sizes)
        still = np.ascontiguousarray(np.broadcast_to(x[:1], x.shape))
        got = B.self_relaxation(still, box[:1].repeat(100, axis=0), off, 99, stride, 0.75, [2.0, 1.3])
        assert np.array_equal(got[3], np.repeat((w * np.uint64(R.UNIT)).astype(np.int64)[:, :, None], 2, axis=2))
        assert np.array_equal(got[1], w) and np.array_equal(got[2], w * sizes[None, :])


def test_order_independence_and_repeatability(B):
    x, box = _walk(41, 90, 50)
    off = np.array([0, 21, 50])
    args = (off, 89, 1, [2.0, 1.0], [[0.3, 2.0], [1.0, 0.0]])
    first = B.self_relaxation(x, box, *args)
    again = B.self_relaxation(x, box, *args)
    rng = np.random.default_rng(2)
    perm = np.concatenate([rng.permutation(21), 21 + rng.permutation(29)])
    shuffled = B.self_relaxation(np.ascontiguousarray(x[:, :, perm]), box, *args)
    B.displacement_hist(x, box, off, [(0, 3, 1), (1, 50, 2)], 0.5, 20)       # another family on the same context
    after = B.self_relaxation(x, box, *args)
    for other in (again, shuffled, after):
        for u, v in zip(first, other):
            assert u.tobytes() == v.tobytes()


def test_nan_and_inf(B):
    x, box = _walk(51, 60, 30)
    off = np.array([0, 10, 20, 30])
    a, q = [1.0, 2.0, 3.0], [0.5, 1.5]
    clean = B.self_relaxation(x, box, off, 59, 1, a, q)
    assert not clean[4].any()
    bad = x.copy()
    bad[17, 1, 14] = np.nan            # entity 14 is in group 1
    bad[40, 0, 14] = np.inf
    bad[41, 0, 14] = np.inf            # (inf - inf is a NaN)
    got = B.self_relaxation(bad, box, off, 59, 1, a, q)
    want = _check(got, bad, box, off, 59, 1, a, q)
    # frame 17 is an end of a window up to lag 42 (17 + 42 = 59); frames 40 and 41 up to lag 41
    assert got[4][:43, 1].all() and not got[4][43:, 1].any() and not got[4][:, 0].any() and not got[4][:, 2].any()
    assert got[4][0, 1] == 3 and want[4][1, 1] == 5    # lag 0: the three frames; lag 1: 16-17, 17-18, 39-40, 40-41, 41-42
    for k in (1, 2, 3):
        assert np.array_equal(got[k][:, [0, 2]], clean[k][:, [0, 2]])
    # a NaN next to a box face shifts nothing: the entity's other frames keep the image counts they had
    edge = x.copy()
    edge[:, 2, 3] = np.where(np.arange(60) % 2 == 0, 0.01, box[:, 2] - 0.01)   # back and forth across the face
    edge[30, 2, 3] = np.nan
    got = B.self_relaxation(edge, box, off, 59, 1, a, q)
    _check(got, edge, box, off, 59, 1, a, q)
    assert got[4][:31, 0].all() and not got[4][31:, 0].any()   # frame 30 ends windows up to lag 30


def test_input_forms(B):
    import torch

    x, box = _walk(61, 80, 33)
    off = np.array([0, 16, 33])
    host = B.self_relaxation(x, box, off, 50, 2, 1.5, [0.9])
    dev = B.self_relaxation(torch.from_numpy(x).cuda(), box, off, 50, 2, 1.5, [0.9])
    for u, v in zip(host, dev):
        assert np.array_equal(u, v)


def _one_entity_truth(fs, q, dist):
    """One entity, one term per (lag, origin): |fs / 2^32 - sinc| <= 2^-33 + 2^-34 + x 2^-52 (values below 2^32 are
    exact in float64)."""
    xq = q * dist
    err = np.abs(fs.astype(np.float64) / float(R.UNIT) - R.sinc(xq))
    assert xq.max() <= 100.0
    assert np.all(err <= 2.0 ** -33 + 2.0 ** -34 + xq * 2.0 ** -52)


def test_more_origin_tiles_than_a_launch_dimension(B):
    """65 535 * TO + 2 frames of one entity, lags 0 and 1: 65 536 origin tiles, two launches."""
    F = 65535 * TO + 2
    rng = np.random.default_rng(71)
    x = np.ascontiguousarray(np.cumsum(rng.uniform(-0.5, 0.5, size=(F, 3, 1)), axis=0))
    a, q = 0.4, 3.0
    origins, c1, c2, fs, bad = B.self_relaxation(x, None, [0, 1], 1, 1, a, [q])
    d = x[1:] - x[:-1]
    rsq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).ravel()
    n = int(np.count_nonzero(rsq < a * a))
    assert origins.tolist() == [F, F - 1] and not bad.any()
    assert c1.ravel().tolist() == [F, n] and c2.ravel().tolist() == [F, n]
    assert int(fs[0, 0, 0]) == F * R.UNIT
    v = R.sinc(q * np.sqrt(rsq))
    assert q * np.sqrt(rsq).max() <= 100.0
    bound = (F - 1) * (2.0 ** -33 + 2.0 ** -34 + 3.0 * 2.0 ** -52)
    assert abs(Fraction(int(fs[1, 0, 0]), R.UNIT) - Fraction(float(np.sum(v.astype(np.longdouble))))) <= bound + F * 2.0 ** -60


def test_more_lag_tiles_than_a_launch_dimension(B):
    """65 535 * TK + 2 frames of one entity, every lag, origin_stride = F - 1: one origin per lag (two at lag 0), 65 536
    lag tiles, two launches."""
    F = 65535 * TK + 2
    rng = np.random.default_rng(72)
    x = np.ascontiguousarray(np.cumsum(rng.uniform(-0.01, 0.01, size=(F, 3, 1)), axis=0))
    a, q = 2.0, 1.0
    origins, c1, c2, fs, bad = B.self_relaxation(x, None, [0, 1], F - 1, F - 1, a, [q])
    d = x - x[:1]
    rsq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).ravel()
    n = (rsq < a * a).astype(np.uint64)
    n[0] = 2
    assert origins[0] == 2 and np.all(origins[1:] == 1) and not bad.any()
    assert np.array_equal(c1.ravel(), n) and np.array_equal(c2.ravel(), n)
    assert int(fs[0, 0, 0]) == 2 * R.UNIT
    _one_entity_truth(fs[1:, 0, 0], q, np.sqrt(rsq[1:]))


def test_refusals(B):
    """Straight to the C entry point: every refusal of include/mdhip.h is MDHIP_EINVAL, and the outputs, pre-filled
    with a pattern, are untouched."""
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    F, E, G = 6, 4, 2
    r = np.zeros((F, 3, E))
    good = dict(F=F, E=E, r=r, G=G, off=np.array([0, 2, 4], dtype=np.int64), max_lag=3, stride=1,
                a_sq=np.array([1.0, 2.0]), n_q=2, q=np.array([[0.5, 1.0], [2.0, 0.0]]), null=())
    bad = [dict(G=0), dict(G=17, off=np.arange(18, dtype=np.int64) // 5), dict(n_q=-1), dict(n_q=5), dict(F=0),
           dict(F=1 << 29), dict(max_lag=-1), dict(max_lag=F), dict(stride=0), dict(stride=-3),
           dict(off=np.array([0, 3, 2], dtype=np.int64)), dict(off=np.array([0, 2, 5], dtype=np.int64)),
           dict(off=np.array([-1, 2, 4], dtype=np.int64)),
           dict(q=np.array([[0.5, -1.0], [2.0, 0.0]])), dict(q=np.array([[0.5, np.inf], [2.0, 0.0]])),
           dict(q=np.array([[np.nan, 1.0], [2.0, 0.0]])), dict(a_sq=np.array([1.0, -2.0])),
           dict(a_sq=np.array([np.nan, 2.0])), dict(a_sq=None, n_q=0),
           dict(null=("origins",)), dict(null=("count1",)), dict(null=("count2",)), dict(null=("fs",)),
           dict(null=("nonfinite",)), dict(null=("q",)), dict(null=("off",)), dict(null=("r",))]

    def call(c):
        out = {"origins": np.full(4, 77, dtype=np.uint64), "count1": np.full((4, 2), 77, dtype=np.uint64),
               "count2": np.full((4, 2), 77, dtype=np.uint64), "fs": np.full((4, 2, 2), 77, dtype=np.int64),
               "nonfinite": np.full((4, 2), 77, dtype=np.uint64)}

        def arg(name, value, ctype):
            return None if name in c["null"] or value is None else ptr(value, ctype)

        rc = ctx.lib.mdhip_self_relaxation(
            ctx.h, c["F"], c["E"], None if "r" in c["null"] else C.c_void_p(c["r"].ctypes.data), 0, None, c["G"],
            arg("off", c["off"], C.c_int64), c["max_lag"], c["stride"], arg("a_sq", c["a_sq"], C.c_double), c["n_q"],
            arg("q", c["q"], C.c_double), arg("origins", out["origins"], C.c_uint64),
            arg("count1", out["count1"], C.c_uint64), arg("count2", out["count2"], C.c_uint64),
            arg("fs", out["fs"], C.c_int64), arg("nonfinite", out["nonfinite"], C.c_uint64))
        return rc, out

    for change in bad:
        rc, out = call(dict(good, **change))
        with pytest.raises(MdhipError) as err:
            ctx.check(rc)
        assert err.value.code == -1, change   # MDHIP_EINVAL
        for name, arr in out.items():
            assert (arr == 77).all(), (change, name)
    rc, out = call(good)
    ctx.check(rc)
    assert out["origins"].tolist() == [6, 5, 4, 3] and (out["count1"] == out["origins"][:, None] * 2).all()
    # strides near 2^63 are accepted as they are (no Python wrapper in between): one origin per lag, counted once
    for stride in (F, 1 << 58, 1 << 61, (1 << 62) + 1, (1 << 63) - 1):
        rc, out = call(dict(good, stride=stride))
        ctx.check(rc)
        assert out["origins"].tolist() == [1, 1, 1, 1] and (out["count1"] == 2).all() and (out["count2"] == 4).all()
        assert (out["fs"] == R.UNIT * 2).all() and not out["nonfinite"].any()
    # the size guard at its boundary, with NULL coordinates so that nothing can be read: 32 768 origins times 32 768
    # entities is 2^30 and is refused with the remedy in the text; 32 767 entities pass the guard (and then stop at the
    # NULL coordinates)
    for size, guarded in ((32768, True), (32767, False)):
        c = dict(good, F=32768, E=size, off=np.array([0, 0, size], dtype=np.int64), null=("r",))
        rc, out = call(c)
        with pytest.raises(MdhipError) as err:
            ctx.check(rc)
        assert err.value.code == -1 and ("origin_stride" in str(err.value)) == guarded, str(err.value)
        assert all((arr == 77).all() for arr in out.values())
    c = dict(good, F=32768, E=32768, stride=2, off=np.array([0, 0, 32768], dtype=np.int64), null=("r",))
    with pytest.raises(MdhipError) as err:
        ctx.check(call(c)[0])
    assert "origin_stride" not in str(err.value)   # 16 384 origins: inside the guard


@pytest.mark.parametrize("coords", ["wrapped", "unwrapped"])
def test_dropin_on_dumps(coords, tmp_path):
    """50 frames, 45 atoms, 2 of 3 types requested: the DataFrames of the class against those built from the
    restatement on the parsed arrays. Q and chi4 are quotients of the same integers: ==. F_s within the fs bound
    divided by W."""
    from mdproptools_amd.dynamical.relaxation import StructuralRelaxation

    types = np.array([1] * 20 + [2] * 10 + [3] * 15)
    x, box, true = D.fractional_walk(19, 50, 45, max_step=0.05)
    pattern = D.write_dumps(str(tmp_path), x, true, box, types)
    cols = ["x", "y", "z"] if coords == "wrapped" else ["xu", "yu", "zu"]
    r, rbox, off, _ = D.read_dumps(pattern, [3, 1], cols)
    bx = rbox if coords == "wrapped" else None
    a, q = {3: 2.0, 1: 3.0}, {3: [0.5, 1.0], 1: [0.8, 0.2]}
    s = StructuralRelaxation([3, 1], pattern, dt=2, working_dir=str(tmp_path), coords=coords)
    for stride in (1, 4):
        df = s.calc_relaxation(q=q, a=a, origin_stride=stride)
        want = R.tables(r, bx, off, [3, 1], 0.2, 24, stride, a, q)
        truth = R.self_relaxation(r, bx, off, 24, stride, [a[3], a[1]], [q[3], q[1]], want_truth=True)
        per_w = R.fs_bound(truth[0], np.diff(off), truth[6]) / (truth[0].astype(np.float64)[:, None] * np.diff(off))
        assert list(df.columns) == list(want)
        for c in want:
            got_c, want_c = np.asarray(df[c], dtype=np.float64), np.asarray(want[c], dtype=np.float64)
            if c.startswith("Fs_"):
                g = 0 if c.startswith("Fs_3_") else 1
                j = q[[3, 1][g]].index(float(c.split("_q")[1]))
                exact = truth[5][:, g, j] / (truth[0].astype(np.float64) * np.diff(off)[g])
                assert np.all(np.abs(got_c - exact) <= per_w[:, g] + 2.0 ** -52), c
            else:
                assert np.array_equal(got_c, want_c), c
    times = s.calc_relaxation_times()
    assert len(times) == 6 and (tmp_path / "relaxation.csv").exists() and (tmp_path / "relaxation_times.csv").exists()
