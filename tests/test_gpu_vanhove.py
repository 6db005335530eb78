"""
mdhip_van_hove_distinct (csrc/vanhove.hip) and Displacement.calc_van_hove_distinct on the GPU. Every output of the
kernel is an integer, so everything is held to equality: against the numpy restatement (tests/vanhove_ref.py), against
the pair sweep of mdhip_rdf_sites on two shifted views of the trajectory (an independent kernel), and against the self
part, mdhip_displacement_hist, through the doubled-trajectory identity hist(A, B) - hist(A, A) (another one).
hist.sum(1) + beyond == pairs is asserted in every case. Shapes are the smallest at which the kernel can go wrong: group
sizes either side of a wave and a block, an empty group, rows that fit LDS and that do not, a distance on a bin edge
and the double below, |d| of exactly half a box edge and one ulp more, a bin that receives more than 2^32 pairs, more
jobs than one launch dimension, 70 001 frames, more uniform entities than one chunk of 2^20, NaN and +inf.
"""
import numpy as np
import pytest

import vanhove_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(got):
    hist, beyond, pairs = got
    assert hist.dtype == np.uint64 and beyond.dtype == np.uint64 and pairs.dtype == np.uint64
    assert np.array_equal(hist.sum(axis=1) + beyond, pairs)
    return got


def _same(got, want):
    _check(got)
    assert got[0].shape == want[0].shape
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_ent", [1, 63, 64, 65, 257])
def test_group_sizes(B, n_ent):
    """Groups (n // 3, 0, the rest): (a, a), (a, b), (b, a) and everything with the empty group, lags 0, 1, F - 1,
    strides 1, 2, 4, in a box that changes every frame."""
    x, box = R.grid_walk(n_ent, 7, n_ent)
    off = R.three_groups(n_ent)
    jobs = [(a, b, k, s) for a, b in ((0, 0), (2, 2), (0, 2), (2, 0), (0, 1), (1, 1), (1, 2))
            for k in (0, 1, 6) for s in (1, 2, 4)]
    got = B.van_hove_distinct(x, box, off, jobs, 0.25, 24)
    _same(got, R.van_hove_distinct(x, box, off, jobs, 0.25, 24))
    assert np.array_equal(got[2], R.expected_pairs(7, off, jobs))
    again = B.van_hove_distinct(x, box, off, jobs, 0.25, 24)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_symmetries_at_lag_zero(B):
    x, box = R.grid_walk(3, 5, 130)
    off = np.array([0, 70, 130])
    hist, _, _ = _check(B.van_hove_distinct(x, box, off, [(0, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (1, 1, 0, 2)],
                                            0.25, 20))
    assert hist[0].sum() > 0 and np.array_equal(hist[0], hist[1])
    assert hist[2].sum() > 0 and not (hist[2] % 2).any() and not (hist[3] % 2).any()


@pytest.mark.parametrize("k", [0, 1, 5])
def test_against_the_pair_sweep_on_shifted_views(B, k):
    """An independent kernel: the atoms x sites sweep of mdhip_rdf_sites on r[:F-k] of group a and r[k:] of group b,
    with the boxes of the origin frames, summed over the frames. r_cut = 14 * 0.25 = 3.5: r_cut^2 is exact."""
    F = 12
    x, box = R.grid_walk(31, F, 150)
    off = np.array([0, 60, 150])
    n_bins, bin_size = 14, 0.25
    xa = np.ascontiguousarray(x[:F - k, :, :60])
    xb = np.ascontiguousarray(x[k:, :, 60:])
    part, ov = B.rdf_mol_loop(xa, np.ones(60, dtype=np.int32), xb, np.ones(90, dtype=np.int32), box[:F - k],
                              np.array([[1, 1]]), n_bins * bin_size, bin_size, n_bins, per_frame=False)
    hist, beyond, pairs = _check(B.van_hove_distinct(x, box, off, [(0, 1, k, 1)], bin_size, n_bins))
    assert hist[0].sum() > 1000
    assert np.array_equal(hist[0], np.asarray(part).reshape(n_bins))
    assert int(pairs[0]) == (F - k) * 60 * 90


@pytest.mark.parametrize("k", [1, 5, 10])
def test_against_the_self_part_on_a_doubled_trajectory(B, k):
    """Another independent kernel. Entities doubled, A = [0, E), B = [E, 2E) the same atoms again: hist(A, B, k) has
    every pair of hist(A, A, k) and the pairs (i at t0, i at t0 + k), so the difference is the histogram of the
    minimum-image self displacement: that of mdhip_displacement_hist while no atom travels half an edge in the lag."""
    E = 65
    x, box = R.grid_walk(3, 30, E, max_step=0.02, vary_box=False)
    xx = np.ascontiguousarray(np.concatenate([x, x], axis=2))
    hist, beyond, pairs = _check(B.van_hove_distinct(xx, box, [0, E, 2 * E], [(0, 1, k, 1), (0, 0, k, 1)], 0.25, 16))
    self_hist, overflow, windows, _, _ = B.displacement_hist(x, box, [0, E], [(0, k, 1)], 0.25, 16)
    assert self_hist.sum() > 0
    assert np.array_equal(hist[0] - hist[1], self_hist[0])
    assert beyond[0] - beyond[1] == overflow[0] and pairs[0] - pairs[1] == windows[0]


def _edge_system(seed):
    """Two frames. Entity 300 stands at the origin; at frame 1 entities 0..4 sit at five hand-placed displacements
    around 5 * 0.25 from it, the others at random ones (up to 64 * sqrt(3) = 110.9 < 20000 * 0.25). Box 512: no wrap."""
    x = np.zeros((2, 3, 301))
    rng = np.random.default_rng(seed)
    x[1, :, :300] = rng.integers(0, 1 << 16, size=(3, 300)) / 1024.0
    x[1, :, 0] = [0.75, 1.0, 0.0]
    x[1, :, 1] = [np.nextafter(0.75, 0.0), 1.0, 0.0]
    x[1, :, 2] = [0.75, np.nextafter(1.0, 0.0), 0.0]
    x[1, :, 3] = [-1.0, 0.0, -0.75]
    x[1, :, 4] = [np.nextafter(1.25, 0.0), 0.0, 0.0]
    return x, np.full((2, 3), 512.0), np.array([0, 1, 2, 3, 4, 5, 300, 301])


@pytest.mark.parametrize("n_bins", [1, 5, 6, R.LDS_WORDS, R.LDS_WORDS + 1, 20000])
def test_bin_edges_and_rows_in_and_out_of_lds(B, n_bins):
    """A distance of exactly 5 bins is bin 5 (also where rounding hides an ulp: tests/test_gpu_displacement.py), the
    double below it bin 4; with n_bins = 5 the first is at n_bins exactly, which is beyond. Rows of 16 128 bins live
    in LDS, longer ones in global memory."""
    x, box, off = _edge_system(n_bins)
    jobs = [(6, g, 1, 1) for g in range(6)] + [(5, 6, 1, 1), (5, 5, 1, 1)]
    got = B.van_hove_distinct(x, box, off, jobs, 0.25, n_bins)
    _same(got, R.van_hove_distinct(x, box, off, jobs, 0.25, n_bins))
    if n_bins >= 6:
        assert got[0][:4, 5].tolist() == [1, 1, 1, 1] and got[0][4, 4] == 1
    else:
        assert got[1][:4].tolist() == [1, 1, 1, 1] and got[1][4] == (n_bins < 5)


def test_exactly_half_a_box_edge_and_one_ulp_more(B):
    """Box 8, bins of 0.5: |d| == L/2 is not shifted (distance 4, bin 8), one ulp more is (just below 4, bin 7)."""
    up = np.nextafter(5.0, np.inf)
    x = np.zeros((2, 3, 4))
    x[0, 0] = [1.0, 1.0, 5.0, up]
    x[1, 0] = [5.0, up, 1.0, 1.0]
    box = np.full((2, 3), 8.0)
    jobs = [(0, 1, 1, 1), (1, 0, 1, 1), (2, 3, 1, 1), (3, 2, 1, 1)]
    got = B.van_hove_distinct(x, box, [0, 1, 2, 3, 4], jobs, 0.5, 9)
    _same(got, R.van_hove_distinct(x, box, [0, 1, 2, 3, 4], jobs, 0.5, 9))
    assert [int(np.flatnonzero(h)[0]) for h in got[0]] == [7, 8, 8, 7]


def test_a_bin_that_receives_more_than_2_to_the_32(B):
    """Two groups of 2048 entities at one point, 1101 frames, lag 1, one bin: 1100 * 2048^2 = 4 613 734 400 pairs in
    one word's place. Expected from the formula."""
    import torch

    x = torch.full((1101, 3, 4096), 1.0, dtype=torch.float64, device="cuda")
    box = np.full((1101, 3), 8.0)
    hist, beyond, pairs = _check(B.van_hove_distinct(x, box, [0, 2048, 4096], [(0, 1, 1, 1), (1, 1, 1, 1)], 1.0, 1))
    assert int(hist[0, 0]) == 1100 * 2048 ** 2 == 4613734400 and int(hist[0, 0]) > 1 << 32
    assert int(hist[1, 0]) == 1100 * 2048 * 2047
    assert not beyond.any() and pairs.tolist() == [4613734400, 1100 * 2048 * 2047]


def test_more_jobs_than_a_launch_dimension(B):
    """65 535 jobs fill the job dimension of one launch: 65 541 take two."""
    x, box = R.grid_walk(9, 3, 2)
    off = np.array([0, 1, 2])
    kinds = [(0, 1, 1, 1), (1, 1, 0, 1), (1, 0, 2, 1), (0, 0, 1, 1), (1, 0, 0, 2)]
    jobs = np.array([kinds[j % 5] for j in range(65541)], dtype=np.int32)
    got = _check(B.van_hove_distinct(x, box, off, jobs, 0.5, 12))
    want = R.van_hove_distinct(x, box, off, kinds, 0.5, 12)
    assert want[0].sum() > 0
    for j in (0, 1, 2, 3, 4, 65534, 65535, 65536, 65540):
        assert np.array_equal(got[0][j], want[0][j % 5]) and got[1][j] == want[1][j % 5]
    for k in range(5):
        assert np.array_equal(got[0][k::5], np.broadcast_to(want[0][k], got[0][k::5].shape))
        assert np.all(got[1][k::5] == want[1][k]) and np.all(got[2][k::5] == want[2][k])


def test_70001_frames_of_3_entities(B):
    """More origins than 65 535 at lag 1, and the longest lag."""
    x, box = R.grid_walk(7, 70001, 3, vary_box=False)
    off = np.array([0, 1, 1, 3])
    jobs = [(0, 2, 1, 1), (2, 2, 1, 1), (2, 0, 70000, 1), (2, 2, 70000, 1), (2, 2, 35000, 35000), (0, 2, 7, 4)]
    got = B.van_hove_distinct(x, box, off, jobs, 0.5, 16)
    _same(got, R.van_hove_distinct(x, box, off, jobs, 0.5, 16))
    assert got[2].tolist() == [140000, 140000, 2, 2, 4, 2 * 17499]


def test_past_one_chunk_of_uniform_entities(B):
    """One frame in a box of edge 64, group a of 64 entities and group b of 2^20 + 65, the last 65 of them within 2 of
    entity 0: the long group is the uniform side of both jobs, the lanes holding a (job (a, b)) and holding b (job
    (b, a)), two chunks per tile. Every output equals the sum over b1 | b2 = b split at 2^20 - 7, one chunk each."""
    rng = np.random.default_rng(41)
    n_b = (1 << 20) + 65
    E = 64 + n_b
    x = rng.random((1, 3, E)) * 64.0
    x[0, :, -65:] = np.mod(x[0, :, :1] + rng.uniform(-1.0, 1.0, size=(3, 65)), 64.0)
    box = np.full((1, 3), 64.0)
    got = _check(B.van_hove_distinct(x, box, np.array([0, 64, E]), [(0, 1, 0, 1), (1, 0, 0, 1)], 0.25, 16))
    part = _check(B.van_hove_distinct(x, box, np.array([0, 64, 64 + (1 << 20) - 7, E]),
                                      [(0, 1, 0, 1), (0, 2, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)], 0.25, 16))
    for g, p in zip(got, part):
        assert np.array_equal(p[0] + p[1], g[0]) and np.array_equal(p[2] + p[3], g[1])
    hist, beyond, pairs = got
    assert pairs.tolist() == [64 * n_b] * 2 and np.array_equal(hist[0], hist[1])
    # the last 65 entities are all within reach of entity 0, and they are counted
    assert part[0][1].sum() >= 65 and part[0][0].sum() > 1000 and hist[0].sum() == part[0][0].sum() + part[0][1].sum()


def test_nan_and_inf_leave_with_their_atoms(B):
    """One atom NaN and one +inf throughout: hist is that of the trajectory without the two atoms, and `beyond` grows
    by exactly the pairs they are in."""
    x, box = R.grid_walk(21, 9, 40)
    off = np.array([0, 15, 40])
    jobs = [(a, b, k, 1) for a in (0, 1) for b in (0, 1) for k in (0, 2)]
    clean = B.van_hove_distinct(np.ascontiguousarray(np.delete(x, [7, 22], axis=2)), box, [0, 14, 38], jobs, 0.25, 20)
    bad = x.copy()
    bad[:, 1, 7] = np.nan
    bad[:, 0, 22] = np.inf
    got = _check(B.van_hove_distinct(bad, box, off, jobs, 0.25, 20))
    _check(clean)
    assert clean[0].sum() > 0 and np.array_equal(got[0], clean[0])
    assert np.array_equal(got[2], R.expected_pairs(9, off, jobs))
    assert np.array_equal(got[1] - clean[1], got[2] - clean[2])
    _same(got, R.van_hove_distinct(bad, box, off, jobs, 0.25, 20))


def test_input_forms(B):
    import torch

    x, box = R.grid_walk(33, 10, 100)
    off = R.three_groups(100)
    jobs = [(0, 2, 0, 1), (2, 0, 3, 2), (2, 2, 9, 1), (0, 0, 1, 1)]
    host = B.van_hove_distinct(x, box, off, jobs, 0.5, 12)
    dev = B.van_hove_distinct(torch.from_numpy(x).cuda(), box, off, jobs, 0.5, 12)
    _same(dev, host)
    _same(host, R.van_hove_distinct(x, box, off, jobs, 0.5, 12))


def test_invalid_arguments_are_refused_by_the_library(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    import ctypes as C

    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    r = np.zeros((4, 3, 2))
    box = np.ones((4, 3))
    good = dict(box=box, off=[0, 1, 2], job=(0, 1, 1, 1), bin_size=0.5, nb=4)
    bad = [dict(box=None), dict(job=(2, 0, 1, 1)), dict(job=(0, 2, 1, 1)), dict(job=(-1, 0, 1, 1)),
           dict(job=(0, 1, -1, 1)), dict(job=(0, 1, 4, 1)), dict(job=(0, 1, 1, 0)), dict(nb=0), dict(nb=(1 << 20) + 1),
           dict(bin_size=0.0), dict(bin_size=-0.5), dict(bin_size=float("nan")), dict(bin_size=float("inf")),
           dict(off=[0, 2, 1]), dict(off=[0, 1, 3]), dict(off=[-1, 1, 2])]

    def call(box, off, job, bin_size, nb):
        off = np.array(off, dtype=np.int64)
        jb = np.array([job], dtype=np.int32)
        hist = np.full((1, 4), 77, dtype=np.uint64)
        out = np.full(2, 77, dtype=np.uint64)
        rc = ctx.lib.mdhip_van_hove_distinct(
            ctx.h, 4, 2, C.c_void_p(r.ctypes.data), 0, None if box is None else ptr(box), 2, ptr(off, C.c_int64), 1,
            ptr(jb, C.c_int32), bin_size, nb, None, ptr(hist, C.c_uint64), ptr(out[0:], C.c_uint64),
            ptr(out[1:], C.c_uint64))
        return rc, hist, out

    for change in bad:
        rc, hist, out = call(**dict(good, **change))
        with pytest.raises(MdhipError):
            ctx.check(rc)
        assert (hist == 77).all() and (out == 77).all(), change
    rc, hist, out = call(**good)
    ctx.check(rc)
    assert out[1] == 3 and hist.sum() + out[0] == 3


TYPES = np.array([1] * 25 + [2] * 20 + [3] * 15)


def test_dropin_on_dumps(tmp_path):
    """40 frames, 60 atoms, three types: the tables of the class against those built from the restatement on the
    parsed arrays. The integers are equal; G_d is one product, one mean and one quotient away: 4 * 2^-52 relative."""
    from mdproptools_amd.dynamical.residence_time import Displacement

    x, box, true = R.fractional_walk(17, 40, 60, max_step=0.15)
    pattern = R.write_dumps(str(tmp_path), x, true, box, TYPES)
    r, rbox, off, steps = R.read_dumps(pattern, [3, 1, 2], ["x", "y", "z"])
    n_bins = int(np.ceil(0.5 * rbox.min() / 0.4))
    d = Displacement([3, 1, 2], {}, pattern, dt=2, working_dir=str(tmp_path), bin_size=0.4)
    gd, summary = d.calc_van_hove_distinct([0.0, 0.2, 1.0, 7.8], origin_stride=3)  # frames 0.2 ps apart
    pairs = R.default_pairs([3, 1, 2])
    want_gd, want_sum = R.distinct_tables(r, rbox, off, [3, 1, 2], pairs, [0, 1, 5, 39], 3, 0.2, 0.4, n_bins)
    assert list(gd) == pairs and list(summary.columns) == list(want_sum)
    for c in want_sum:
        assert np.array_equal(np.asarray(summary[c]), np.asarray(want_sum[c])), c
    assert sum(summary["pairs"]) > sum(summary["beyond r_max"]) > 0
    for p in pairs:
        assert list(gd[p].columns) == list(want_gd[p])
        for c in want_gd[p]:
            a, b = np.asarray(gd[p][c], dtype=np.float64), np.asarray(want_gd[p][c])
            assert np.all(np.abs(a - b) <= 4 * 2.0 ** -52 * np.abs(b)), (p, c)
        assert (tmp_path / ("van_hove_distinct_%s-%s.csv" % p)).exists()
    assert (tmp_path / "van_hove_distinct_pairs.csv").exists()


def test_zero_lag_column_is_the_atomic_rdf(tmp_path):
    """Constant box: the 0 ps column is g_a-b of calc_atomic_rdf for the same relation, r_cut and bin size. A mean of F
    per-frame quotients against one quotient of the summed integers, and their roundings: (F + 8) * 2^-52 relative."""
    from mdproptools_amd.dynamical.residence_time import Displacement
    from mdproptools_amd.structural.rdf_cn import calc_atomic_rdf

    F = 40
    x, box, true = R.fractional_walk(23, F, 60, max_step=0.15)
    const = np.tile(np.array([20.0, 25.0, 30.0]), (F, 1))
    xc = x / box[:, :, None] * const[:, :, None]
    pattern = R.write_dumps(str(tmp_path), xc, true, const, TYPES)
    pairs = [(1, 1), (1, 2), (3, 1), (2, 3)]
    d = Displacement([1, 2, 3], {}, pattern, dt=2, save_mode=False, bin_size=0.25, r_max=8.0)
    gd, _ = d.calc_van_hove_distinct([0.0], pairs=pairs)
    rdf = calc_atomic_rdf(8.0, 0.25, 3, [1.0, 1.0, 1.0], [[a for a, _ in pairs], [b for _, b in pairs]], pattern,
                          save_mode=False)
    assert len(rdf) == 32
    for a, b in pairs:
        got, want = np.asarray(gd[(a, b)][0.0]), np.asarray(rdf["g_%d-%d" % (a, b)])
        print((a, b), "largest relative difference", np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
        assert want.sum() > 0 and np.all(np.abs(got - want) <= (F + 8) * 2.0 ** -52 * np.abs(want)), (a, b)
