"""
mdhip_displacement_hist (csrc/displacement.hip) and the Displacement drop-in on the GPU, against the numpy restatement
(tests/displacement_ref.py): hist, overflow, windows and crossings by equality, the moments within windows * 2^-52
relative (the terms are identical non-negative doubles, so two summation orders differ by at most 2 (n - 1) 2^-53),
and bit-identical from call to call. Shapes are the smallest at which the kernel can go wrong: entity counts either
side of a wave and a block, an empty group, frame counts either side of the image-count chunk, 70 001 frames (1094
chunks, 70 000 origins), more jobs than one launch dimension, rows that fit LDS and that do
not, displacements on a bin edge and one ulp below, steps of exactly half a box edge and just past, a box per frame,
NaN. The independent check is the full-lag MSD kernel.
"""
import numpy as np
import pytest

import displacement_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _same(got, want):
    hist, overflow, windows, moments, crossings = got
    assert hist.dtype == np.uint64 and overflow.dtype == np.uint64 and windows.dtype == np.uint64
    assert hist.shape == want[0].shape
    assert np.array_equal(hist, want[0])
    assert np.array_equal(overflow, want[1])
    assert np.array_equal(windows, want[2])
    assert crossings == want[4]
    print("moments", moments.tolist(), "want", want[3].tolist())
    assert R.moments_close(moments, want[3], want[2])
    assert np.array_equal(hist.sum(axis=1) + overflow, windows)


def _jobs(n_frames, groups=3):
    """Lags 1 and F - 1; stride 1, the lag, and one that leaves a remainder; every group."""
    lags = sorted({1, max(1, n_frames // 3), n_frames - 1})
    return [(g, k, s) for g in range(groups) for k in lags for s in sorted({1, k, 4})]


@pytest.mark.parametrize("n_ent", [1, 63, 64, 65, 257])
def test_entity_counts(B, n_ent):
    x, box = R.grid_walk(n_ent, 23, n_ent)
    off = R.three_groups(n_ent)
    jobs = _jobs(23)
    got = B.displacement_hist(x, box, off, jobs, 0.5, 40)
    _same(got, R.displacement_hist(x, box, off, jobs, 0.5, 40))
    assert got[4] > 0 or n_ent == 1
    again = B.displacement_hist(x, box, off, jobs, 0.5, 40)
    assert again[3].tobytes() == got[3].tobytes()


@pytest.mark.parametrize("n_frames", [2, 3, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, R.CHUNK + 2, 2 * R.CHUNK + 1])
def test_frame_counts_around_the_chunk(B, n_frames):
    x, box = R.grid_walk(100 + n_frames, n_frames, 70)
    off = R.three_groups(70)
    jobs = _jobs(n_frames)
    _same(B.displacement_hist(x, box, off, jobs, 0.25, 64), R.displacement_hist(x, box, off, jobs, 0.25, 64))


def test_70001_frames_of_3_entities(B):
    """1094 chunks through the chunk scan, lags up to F - 1, and at lag 1 more origins than 65 535."""
    x, box = R.grid_walk(7, 70001, 3, vary_box=False)
    off = np.array([0, 1, 1, 3])
    jobs = [(0, 1, 1), (2, 1, 1), (2, 70000, 1), (2, 35000, 35000), (0, 7, 4), (2, 64, 64)]
    got = B.displacement_hist(x, box, off, jobs, 0.5, 30)
    _same(got, R.displacement_hist(x, box, off, jobs, 0.5, 30))
    assert got[2].tolist() == [70000, 140000, 2, 4, 17499, 2 * 1093]


def test_eight_jobs_on_one_group(B):
    x, box = R.grid_walk(8, 40, 90)
    jobs = [(0, k, 1) for k in (1, 2, 3, 5, 8, 13, 21, 39)]
    _same(B.displacement_hist(x, box, [0, 90], jobs, 0.3, 50), R.displacement_hist(x, box, [0, 90], jobs, 0.3, 50))


def test_more_jobs_than_a_launch_dimension(B):
    """65 535 jobs fill the job dimension of one launch: 65 541 take two."""
    x, box = R.grid_walk(9, 3, 2)
    off = np.array([0, 1, 2])
    kinds = [(0, 1, 1), (1, 2, 1), (1, 1, 2), (0, 2, 5), (1, 1, 1)]
    jobs = np.array([kinds[j % 5] for j in range(65541)], dtype=np.int32)
    got = B.displacement_hist(x, box, off, jobs, 0.5, 1)
    want = R.displacement_hist(x, box, off, kinds, 0.5, 1)
    for j in (0, 1, 2, 3, 4, 65534, 65535, 65536, 65540):
        assert np.array_equal(got[0][j], want[0][j % 5]) and got[1][j] == want[1][j % 5]
    for k in range(5):
        assert np.array_equal(got[0][k::5], np.broadcast_to(want[0][k], got[0][k::5].shape))
        assert np.all(got[1][k::5] == want[1][k]) and np.all(got[2][k::5] == want[2][k])
        assert np.all(got[3][k::5] == got[3][k])  # the same job: the same launch geometry, the same bits
        assert R.moments_close(got[3][k:k + 1], want[3][k:k + 1], want[2][k:k + 1])
    assert got[4] == want[4]


def _half_box_system():
    """Box 8: atoms stepping by exactly +L/2 and -L/2 (no shift) and by one ulp more (a shift), then standing."""
    up = np.nextafter(5.0, np.inf)
    x = np.zeros((3, 3, 4))
    x[:, 0, 0] = [1.0, 5.0, 5.0]   # d == +L/2
    x[:, 0, 1] = [5.0, 1.0, 1.0]   # d == -L/2
    x[:, 0, 2] = [1.0, up, up]     # d just above +L/2
    x[:, 0, 3] = [up, 1.0, 1.0]    # d just below -L/2
    return x, np.full((3, 3), 8.0)


def test_steps_of_exactly_half_a_box_edge(B):
    x, box = _half_box_system()
    jobs = [(g, 1, 1) for g in range(4)]
    off = np.arange(5)
    got = B.displacement_hist(x, box, off, jobs, 0.5, 20)
    _same(got, R.displacement_hist(x, box, off, jobs, 0.5, 20))
    assert got[4] == 2
    first = np.sqrt(got[3][:, 1] - 0.0)  # one window of the two is the standing one: sum rsq = the step squared
    assert first[0] == 4.0 and first[1] == 4.0  # not shifted: the atom went half a box
    assert abs(first[2] - 4.0) < 1e-14 and first[2] < 4.0 and abs(first[3] - 4.0) < 1e-14 and first[3] < 4.0


def test_nan_shifts_nothing_and_overflows(B):
    x, box = R.grid_walk(21, 9, 10)
    x[4, 1, 7] = np.nan
    off = np.array([0, 5, 10])
    jobs = [(0, 2, 1), (1, 2, 1), (1, 8, 1)]
    got = B.displacement_hist(x, box, off, jobs, 0.5, 16)
    want = R.displacement_hist(x, box, off, jobs, 0.5, 16)
    _same(got, want)
    assert not np.isnan(got[3][0]).any() and np.isnan(got[3][1]).all() and not np.isnan(got[3][2]).any()
    assert got[1][1] >= 2  # frame 4 is the end of the window from frame 2 and the start of the one to frame 6


def _edge_system(seed):
    """Two frames, the first at the origin: five hand-placed displacements around 5 * 0.25, then random ones."""
    x = np.zeros((2, 3, 300))
    rng = np.random.default_rng(seed)
    x[1] = rng.integers(0, 1 << 16, size=(3, 300)) / 1024.0  # up to 64 * sqrt(3) = 110.9 < 20000 * 0.25
    x[1, :, 0] = [0.75, 1.0, 0.0]
    x[1, :, 1] = [np.nextafter(0.75, 0.0), 1.0, 0.0]
    x[1, :, 2] = [0.75, np.nextafter(1.0, 0.0), 0.0]
    x[1, :, 3] = [-1.0, 0.0, -0.75]
    x[1, :, 4] = [np.nextafter(1.25, 0.0), 0.0, 0.0]
    return x, np.array([0, 1, 2, 3, 4, 5, 300])


def test_edge_system_under_the_binning_rule():
    """What bin = (int64)(sqrt(rsq) / bin_size) makes of the hand-placed displacements, in numpy: (3, 4, 0) * 0.25 is
    bin 5 exactly. One ulp less on x (0.75) is lost when rsq is rounded, one ulp less on y (1.0) leaves rsq the double
    below 1.5625 but its correctly rounded sqrt is 1.25 again: the rule puts both in bin 5, not in bin 4. The largest
    distance that is in bin 4 is the double below 1.25 along one axis."""
    x, off = _edge_system(6)
    d = x[1, :, :5]
    rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert rsq.tolist() == [1.5625, 1.5625, np.nextafter(1.5625, 0.0), 1.5625, 1.5625 - 2.0 ** -51]
    assert (np.sqrt(rsq) / 0.25).astype(np.int64).tolist() == [5, 5, 5, 5, 4]


@pytest.mark.parametrize("n_bins", [1, 5, 6, R.LDS_WORDS, R.LDS_WORDS + 1, 20000])
def test_bin_edges_and_rows_in_and_out_of_lds(B, n_bins):
    """The edge system (test_edge_system_under_the_binning_rule) through the kernel: a distance of exactly 5 bins is bin
    5, the double below it bin 4; with n_bins = 5 the first lands at n_bins exactly, which is overflow. Rows of 16 128
    bins live in LDS, longer ones in global memory."""
    x, off = _edge_system(n_bins)
    jobs = [(g, 1, 1) for g in range(6)]
    got = B.displacement_hist(x, None, off, jobs, 0.25, n_bins)
    _same(got, R.displacement_hist(x, None, off, jobs, 0.25, n_bins))
    assert got[4] == 0
    if n_bins >= 6:
        assert got[0][:4, 5].tolist() == [1, 1, 1, 1] and got[0][4, 4] == 1
    else:
        assert got[1][:4].tolist() == [1, 1, 1, 1] and got[1][4] == (n_bins < 5)
    assert got[3][0].tolist() == [1.25, 1.5625, 1.5625 ** 2]
    assert got[3][2][:2].tolist() == [1.25, np.nextafter(1.5625, 0.0)]


def test_input_forms(B):
    import torch

    x, box = R.grid_walk(33, 30, 100)
    off = R.three_groups(100)
    jobs = _jobs(30)
    host = B.displacement_hist(x, box, off, jobs, 0.5, 24)
    dev = B.displacement_hist(torch.from_numpy(x).cuda(), box, off, jobs, 0.5, 24)
    for a, b in zip(host[:3], dev[:3]):
        assert np.array_equal(a, b)
    assert host[4] == dev[4] and host[3].tobytes() == dev[3].tobytes()
    xu, _ = R.unwrap(x, box)
    raw = B.displacement_hist(xu, None, off, jobs, 0.5, 24)
    assert raw[4] == 0
    for a, b in zip(host[:3], raw[:3]):
        assert np.array_equal(a, b)
    assert raw[3].tobytes() == host[3].tobytes()  # xu is the kernel's own x + n * L
    _same(host, R.displacement_hist(x, box, off, jobs, 0.5, 24))


def test_invalid_arguments_are_refused_by_the_library(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    import ctypes as C

    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    r = np.zeros((4, 3, 2))
    off = np.array([0, 2], dtype=np.int64)
    for job, nb in (((0, 0, 1), 4), ((0, 4, 1), 4), ((0, 1, 0), 4), ((1, 1, 1), 4), ((0, 1, 1), 0),
                    ((0, 1, 1), (1 << 20) + 1)):
        jb = np.array([job], dtype=np.int32)
        hist = np.full((1, 4), 77, dtype=np.uint64)
        out = np.full(3, 77, dtype=np.uint64)
        mom = np.full(3, 77.0)
        with pytest.raises(MdhipError):
            ctx.check(ctx.lib.mdhip_displacement_hist(
                ctx.h, 4, 2, C.c_void_p(r.ctypes.data), 0, None, 1, ptr(off, C.c_int64), 1, ptr(jb, C.c_int32), 0.5,
                nb, None, ptr(hist, C.c_uint64), ptr(out[0:], C.c_uint64), ptr(out[1:], C.c_uint64), ptr(mom),
                ptr(out[2:], C.c_uint64)))
        assert (hist == 77).all() and (out == 77).all() and (mom == 77.0).all()


def test_second_moment_is_the_full_lag_msd(B):
    """An independent kernel: moments[:, 1] / windows at stride 1 is the total column of the full-lag MSD, to the
    rtol 1e-10 include/mdhip.h states for mdhip_lag_msd."""
    rng = np.random.default_rng(4)
    xu = np.ascontiguousarray(np.cumsum(rng.normal(0.0, 0.3, size=(1000, 3, 50)), axis=0))
    off = np.array([0, 20, 50], dtype=np.int64)
    lags = [1, 2, 10, 100, 500, 998, 999]
    jobs = [(g, k, 1) for g in range(2) for k in lags]
    _, _, windows, moments, _ = B.displacement_hist(xu, None, off, jobs, 0.5, 10)
    msd = B.lag_msd(xu, 999, off)
    got = (moments[:, 1] / windows).reshape(2, len(lags))
    want = np.asarray(msd)[lags][:, :, 3].T
    print("msd", got.tolist(), want.tolist())
    assert np.allclose(got, want, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("coords", ["wrapped", "unwrapped"])
def test_dropin_on_dumps(coords, tmp_path):
    """40 frames, 60 atoms, 2 of 3 types requested: the DataFrames of the class against those built from the
    restatement on the parsed arrays."""
    from mdproptools_amd.dynamical.residence_time import Displacement

    types = np.array([1] * 25 + [2] * 20 + [3] * 15)
    x, box, true = R.fractional_walk(17, 40, 60, max_step=0.15)
    pattern = R.write_dumps(str(tmp_path), x, true, box, types)
    cols = ["x", "y", "z"] if coords == "wrapped" else ["xu", "yu", "zu"]
    r, rbox, off, steps = R.read_dumps(pattern, [3, 1], cols)
    bx = rbox if coords == "wrapped" else None
    tau = {3: 1.3, 1: 0.04}  # frames 0.2 ps apart: 6.5 -> 7 frames, 0.2 -> 1 frame
    n_bins = int(np.ceil(0.5 * rbox.min() / 0.2))

    def same(df, want, alpha2=("alpha2",)):
        # at most 39 * 25 windows: a mean is within 975 * 2^-52 = 2.2e-13 relative of the restatement's, the ratio
        # <r^4> / <r^2>^2 within three times that, and alpha2 + 1 = 0.6 * ratio stays below 3 here: 2e-12 absolute
        assert list(df.columns) == list(want)
        for c in want:
            a, b = np.asarray(df[c], dtype=np.float64), np.asarray(want[c], dtype=np.float64)
            if c in alpha2:
                assert np.all(b < 2.0) and np.allclose(a, b, rtol=0.0, atol=2e-12), c
            elif c in ("mean distance", "rms distance"):
                assert np.allclose(a, b, rtol=2.2e-13, atol=0.0), c
            else:
                assert np.array_equal(a, b), c

    for overlap in (False, True):
        d = Displacement([3, 1], tau, pattern, dt=2, working_dir=str(tmp_path), bin_size=0.2, overlap=overlap,
                         coords=coords)
        df = d.calc_dist()
        want_dist, want_hist = R.dist_tables(r, bx, off, [3, 1], tau, 0.2, 0.2, n_bins, overlap)
        same(df, want_dist)
        same(d.hist_df, want_hist)
        assert df["lag (frames)"].tolist() == [7, 1] and df["windows"].tolist()[1] == 39 * 25
    gs, a2 = d.calc_van_hove([0.2, 1.0, 7.8])
    want_gs, want_a2 = R.van_hove_tables(r, bx, off, [3, 1], [1, 5, 39], 0.2, 0.2, n_bins)
    same(a2, want_a2, alpha2=(3, 1))
    for t in (3, 1):
        same(gs[t], want_gs[t])
    for name in ("displacement.csv", "displacement_distribution.csv", "van_hove_3.csv", "van_hove_1.csv",
                 "alpha2.csv"):
        assert (tmp_path / name).exists()
