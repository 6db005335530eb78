"""
backend.angle_hist / calc_angular_distribution and their kernels (csrc/angles.hip) on the GPU: every integer compared
with == against the numpy restatement (tests/angular_ref.py) — the lattices with closed-form counts, randomised
systems built to hit every edge (rsq == r_cut**2 exactly, d == +-L/2 exactly, neighbours across each boundary, an atom
on a centre, collinear and perpendicular neighbours, a per-frame box), and the structural cases (centre counts around
the tile width, candidate counts around the chunk, rows around `cap`, eight triplets, molecule exclusion, the library's
limits, device input, more than 65 535 frames, repeated calls).
"""
import numpy as np
import pytest

import angular_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(B, xyz, box, types, trip, rc, bin_size=1.0, mol_of=None, cap=64, xin=None):
    """backend.angle_hist against the restatement; returns the restatement's (hist, n_degenerate, count)."""
    edges = B.angle_cos_edges(bin_size)
    assert np.array_equal(edges, R.cos_edges(bin_size))
    rc2 = np.asarray(rc, dtype=np.float64).reshape(len(trip), 2) ** 2
    hist, degen, count, centres = B.angle_hist(xin if xin is not None else xyz, box, types, trip, rc2, edges,
                                               mol_of=mol_of, cap=cap)
    wh, wd, wc, wcen = R.angle_hist(xyz, box, types, trip, rc2, edges, mol_of=mol_of)
    assert hist.dtype == np.uint64 and degen.dtype == np.uint64 and count.dtype == np.int32
    assert np.array_equal(centres, wcen)
    assert np.array_equal(count, wc)
    assert np.array_equal(hist.astype(np.int64), wh)
    assert np.array_equal(degen.astype(np.int64), wd)
    return wh, wd, wc


# ---- lattices ----

LATTICES = {"sc": (lambda: R.simple_cubic(4, 2.0), 2.5, {84: 768, 175: 192}),
            "fcc": (lambda: R.fcc(3, 2.0), 1.5, {56: 2592, 84: 1296, 119: 2592, 175: 648})}


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_lattice_backend_and_dropin(B, name, tmp_path):
    from mdproptools_amd.structural.angular_distribution import calc_angular_distribution

    make, r_cut, want = LATTICES[name]
    xyz, box = make()
    n = xyz.shape[2]
    types = np.ones(n, dtype=np.int64)
    wh, _, _ = _check(B, xyz, box, types, [(1, 1, 1)], [[r_cut, r_cut]], bin_size=7.0)
    assert {7 * m: int(h) for m, h in enumerate(wh[0]) if h} == want
    pattern = R.write_dumps(xyz, box, types, str(tmp_path))
    out = tmp_path / "adf.csv"
    adf, summary = calc_angular_distribution(r_cut, 7.0, [(1, 1, 1)], pattern, path_or_buff=str(out))
    assert list(adf.columns) == ["angle", "adf_1-1-1", "count_1-1-1"]
    assert np.array_equal(adf["count_1-1-1"].to_numpy(), wh[0])
    assert out.read_text().splitlines()[0] == "angle,adf_1-1-1,count_1-1-1"
    assert summary["n_angles"].iloc[0] == sum(want.values()) and summary["n_degenerate"].iloc[0] == 0
    if name == "sc":  # cos == 0 exactly against E[90]; the straight angles in the last bin
        wh, _, _ = _check(B, xyz, box, types, [(1, 1, 1)], [[r_cut, r_cut]], bin_size=1.0)
        assert {m: int(h) for m, h in enumerate(wh[0]) if h} == {90: 768, 179: 192}


# ---- randomised systems with the edge cases ----

def _edge_system(seed, n, n_frames=2):
    """Types 1 (centres), 2, 3 in turn; frame 0 carries the edges (r_cut 3.5, box 12 x 9 x 6); the box varies."""
    rng = np.random.default_rng(seed)
    box = np.array([[12.0, 9.0, 6.0], [12.5, 9.25, 6.5], [11.75, 9.5, 6.25]])[:n_frames]
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * np.array([11.5, 8.9, 5.9])[None, :, None], 3)
    types = np.arange(n) % 3 + 1
    c = lambda i: 3 * i        # noqa: E731  (the i-th centre)
    a = lambda i: 3 * i + 1    # noqa: E731  (the i-th atom of type 2)
    f = xyz[0]
    f[:, c(0)], f[:, a(0)] = [5.0, 5.0, 2.0], [8.5, 5.0, 2.0]          # exactly r_cut: left out
    f[:, c(1)], f[:, a(1)] = [4.0, 4.0, 1.0], [4.0, 4.5, 4.0]          # d_z == +L/2
    f[:, c(2)], f[:, a(2)] = [9.0, 4.0, 5.0], [9.5, 4.0, 2.0]          # d_z == -L/2
    f[:, c(3)] = [0.2, 0.3, 0.1]                                       # neighbours across each boundary
    f[:, a(3)], f[:, a(4)], f[:, a(5)] = [11.5, 0.3, 0.1], [0.2, 8.6, 0.1], [0.2, 0.3, 5.4]
    f[:, c(4)] = [6.0, 6.0, 3.0]                                       # collinear and perpendicular neighbours
    f[:, a(6)], f[:, a(7)], f[:, a(8)] = [7.0, 6.0, 3.0], [8.0, 6.0, 3.0], [5.0, 6.0, 3.0]
    f[:, a(9)], f[:, a(10)] = [6.0, 7.0, 3.0], [6.0, 6.0, 4.0]
    f[:, a(11)] = f[:, c(5)]                                           # an atom on a centre: NaN
    return xyz, box, types


@pytest.mark.parametrize("seed,n", [(1, 201), (2, 402), (3, 600)])
def test_random_systems_with_edges(B, seed, n):
    xyz, box, types = _edge_system(seed, n)
    wh, wd, wc = _check(B, xyz, box, types, [(2, 1, 2), (2, 1, 3)], [[3.5, 3.5], [3.5, 3.0]])
    assert wd[0] > 0 and wd[1] > 0                       # the atom on a centre
    assert wh[0][0] > 0 and wh[0][179] > 0 and wh[0][90] > 0  # cos +1, -1 and 0
    edges = R.cos_edges(1.0)
    full = R.angle_hist(xyz[:1], box[:1], types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges)[2][0]
    d = xyz[0][:, 1] - xyz[0][:, 0]
    assert float((d ** 2).sum()) == 3.5 ** 2             # the atom at exactly r_cut ...
    closer = xyz[:1].copy()
    closer[0, 0, 1] = 8.499
    assert R.angle_hist(closer, box[:1], types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges)[2][0, 0] == full[0] + 1  # ... is out


# ---- structural cases ----

@pytest.mark.parametrize("n_centres", [1, 15, 16, 17, 33])
def test_centre_counts_around_the_tile(B, n_centres):
    rng = np.random.default_rng(n_centres)
    n = n_centres + 150
    xyz = np.round(rng.uniform(0, 1, (2, 3, n)) * np.array([9.0, 8.0, 7.0])[None, :, None], 3)
    types = np.where(np.arange(n) < n_centres, 1, 2)
    _check(B, xyz, np.tile([9.0, 8.0, 7.0], (2, 1)), types, [(2, 1, 2)], [[3.0, 3.0]], bin_size=2.0)


@pytest.mark.parametrize("n_cand", [4095, 4096, 4097])
def test_candidate_counts_around_the_chunk(B, n_cand):
    """A dilute box: only the candidates placed next to the three centres are in a shell — the last ones of the
    candidate list among them."""
    rng = np.random.default_rng(n_cand)
    L = 200.0
    xyz = np.round(rng.uniform(0, 1, (1, 3, 3 + n_cand)) * L, 3)
    types = np.where(np.arange(3 + n_cand) < 3, 1, 2)
    xyz[0][:, :3] = [[50.0, 100.0, 150.0], [50.0, 100.0, 150.0], [50.0, 100.0, 150.0]]
    for k, at in enumerate([3, 4, 2 + n_cand, 1 + n_cand, 4098 if n_cand > 4096 else 2000]):
        xyz[0][:, at] = xyz[0][:, k % 3] + np.round(rng.uniform(-1.5, 1.5, 3), 3)
    wh, _, wc = _check(B, xyz, np.full((1, 3), L), types, [(2, 1, 2)], [[3.5, 3.5]])
    assert wc.max() <= 6 and wh.sum() >= 1


def _ball(rng, centre, k, r):
    """k points within r of `centre`, 3 decimals."""
    p = rng.normal(size=(3, k))
    p = p / np.linalg.norm(p, axis=0) * (r * rng.uniform(0.2, 0.95, k))
    return np.round(np.asarray(centre)[:, None] + p, 3)


def test_rows_around_cap_and_the_rerun(B):
    """Centres with 0, 1, 7, 8 and 9 neighbours and cap = 8: the batch is run again with cap = 9."""
    rng = np.random.default_rng(8)
    sizes = [0, 1, 7, 8, 9]
    spots = [[10.0 + 20.0 * i, 50.0, 50.0] for i in range(len(sizes))]
    cols = [np.array(spots).T] + [_ball(rng, s, k, 3.0) for s, k in zip(spots, sizes)]
    xyz = np.concatenate(cols, axis=1)[None]
    types = np.where(np.arange(xyz.shape[2]) < len(sizes), 1, 2)
    box = np.full((1, 3), 120.0)
    for cap in (8, 9, 64):
        wh, _, wc = _check(B, xyz, box, types, [(2, 1, 2)], [[3.5, 3.5]], cap=cap)
        assert list(wc[0]) == sizes and wh.sum() == sum(k * (k - 1) // 2 for k in sizes)


def test_more_than_512_neighbours_raise(B):
    rng = np.random.default_rng(513)
    xyz = np.concatenate([np.full((3, 1), 20.0), _ball(rng, [20.0] * 3, 520, 3.0)], axis=1)[None]
    types = np.where(np.arange(521) < 1, 1, 2)
    edges = B.angle_cos_edges(1.0)
    with pytest.raises(ValueError, match="frame 0, centre atom 0 has 520 neighbours"):
        B.angle_hist(xyz, np.full((1, 3), 40.0), types, [(2, 1, 2)], [[3.5 ** 2] * 2], edges)
    # 512 is fine: two tiles of the staged row and the re-run at the largest cap
    xyz, types = xyz[:, :, :513], types[:513]
    wh, _, wc = _check(B, xyz, np.full((1, 3), 40.0), types, [(2, 1, 2)], [[3.5, 3.5]], bin_size=3.0)
    assert wc.max() == 512 and wh.sum() == 512 * 511 // 2


def test_eight_triplets_and_exclusion(B):
    rng = np.random.default_rng(88)
    n = 360
    xyz = np.round(rng.uniform(0, 1, (3, 3, n)) * np.array([10.0, 9.0, 6.0])[None, :, None], 3)
    xyz[1][:, 5] = xyz[1][:, 0]  # an atom of type 2 on a centre of type 1
    box = np.array([[10.0, 9.0, 6.0], [10.0, 9.5, 6.0], [10.5, 9.0, 6.25]])
    types = np.arange(n) % 4 + 1
    mol_of = np.arange(n) // 4
    trip = [(1, 1, 1), (2, 1, 2), (2, 1, 3), (3, 1, 2), (2, 1, 2), (4, 2, 4), (1, 2, 4), (3, 3, 3)]
    rc = [[3.2, 3.2], [3.0, 3.0], [3.0, 2.5], [2.5, 3.0], [2.0, 3.4], [2.8, 2.8], [3.1, 2.2], [3.5, 3.5]]
    for mol in (None, mol_of):
        wh, wd, _ = _check(B, xyz, box, types, trip, rc, bin_size=1.0, mol_of=mol)
        assert all(wh[t].sum() > 0 for t in range(8))
    wh_all, wd_all, _ = _check(B, xyz, box, types, trip, rc, bin_size=0.5)  # 8 x 360 bins
    assert wd_all.sum() > 0


def test_library_limits(B):
    from mdproptools_amd._lib import MdhipError

    xyz, box = R.simple_cubic(2, 2.0)
    types = np.ones(8, dtype=np.int64)
    edges = B.angle_cos_edges(1.0)
    r2 = [[6.25, 6.25]]
    with pytest.raises(MdhipError, match="n_triplets must be"):
        B.angle_hist(xyz, box, types, [(1, 1, 1)] * 9, r2 * 9, edges)
    with pytest.raises(MdhipError, match="n_triplets \\* n_bins"):
        B.angle_hist(xyz, box, types, [(1, 1, 1)] * 8, r2 * 8, B.angle_cos_edges(0.3))
    with pytest.raises(MdhipError, match="n_triplets \\* n_bins"):
        B.angle_hist(xyz, box, types, [(1, 1, 1)], r2, np.linspace(1, -1, 4097))
    for cap in (0, 513):
        with pytest.raises(MdhipError, match="cap must be in"):
            B.angle_hist(xyz, box, types, [(1, 1, 1)], r2, edges, cap=cap)
    with pytest.raises(ValueError, match="strictly decreasing"):
        B.angle_hist(xyz, box, types, [(1, 1, 1)], r2, edges[::-1])
    # the library checks the table itself
    import ctypes as C

    from mdproptools_amd._lib import default_context, ptr

    ctx = default_context()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    cen, trip, bad = i32(np.arange(8)), i32([1, 1, 1]), np.array([1.0, 0.5, 0.5, -1.0])
    x, bx, r2a = np.ascontiguousarray(xyz), np.ascontiguousarray(box), np.array(r2[0])
    hist, degen, count = np.zeros(4, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(8, dtype=np.int32)
    rc = ctx.lib.mdhip_angle_hist(ctx.h, 1, 8, C.c_void_p(x.ctypes.data), 0, ptr(bx), 8, ptr(cen, C.c_int32),
                                  ptr(i32(types), C.c_int32), 8, ptr(cen, C.c_int32), ptr(i32(types), C.c_int32), None,
                                  1, ptr(trip, C.c_int32), ptr(r2a), 4, ptr(bad), 64, ptr(hist, C.c_uint64),
                                  ptr(degen, C.c_uint64), ptr(count, C.c_int32))
    assert rc == -1
    with pytest.raises(MdhipError, match="strictly decreasing"):
        ctx.check(rc)
    # at the limits: 4096 bins, cap 512
    big = B.angle_cos_edges(180.0 / 4096)
    assert len(big) == 4096
    hist, degen, count, _ = B.angle_hist(xyz, box, types, [(1, 1, 1)], r2, big, cap=512)
    want = R.angle_hist(xyz, box, types, [(1, 1, 1)], r2, big)
    assert np.array_equal(hist.astype(np.int64), want[0]) and np.array_equal(count, want[2])


def test_device_input_and_repeated_calls(B):
    import torch

    xyz, box, types = _edge_system(4, 300, n_frames=3)
    trip, rc = [(2, 1, 2), (3, 1, 2)], [[3.5, 3.5], [3.0, 3.5]]
    _check(B, xyz, box, types, trip, rc, cap=4, xin=torch.as_tensor(xyz, device="cuda"))  # re-run from the device
    edges = B.angle_cos_edges(1.0)
    rc2 = np.asarray(rc) ** 2
    first = B.angle_hist(xyz, box, types, trip, rc2, edges)
    second = B.angle_hist(xyz, box, types, trip, rc2, edges)  # (the workspaces are zeroed again)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


def test_more_than_65535_frames(B):
    rng = np.random.default_rng(9)
    F = 70001
    xyz = np.round(rng.uniform(0, 5, (F, 3, 5)), 3)
    wh, _, wc = _check(B, xyz, np.full((F, 3), 5.0), np.array([1, 2, 2, 2, 2]), [(2, 1, 2)], [[2.4, 2.4]],
                       bin_size=2.0)
    assert wh.sum() > F and wc.max() == 4
