"""
mdhip_free_volume (csrc/free_volume.hip, csrc/cell_plan.h) and structural/free_volume.py on the GPU, against the numpy
restatement (tests/free_volume_ref.py), which tests every grid point against every atom and knows nothing of cells.

The header states every operation, so every count is compared with `==` and the field (s, nearest) bit for bit. Shapes
are the smallest at which the kernel can go wrong: boxes that differ per frame, odd grids, one and two cells on an axis
(the neighbour offsets name a cell more than once), a search radius above half an edge, sparse and empty cells, a cell
with several staging chunks, bricks of more than 1024 points, frames beyond any launch dimension, several batches, rows
beyond the LDS bins, exact ties and atoms exactly on cell faces and exactly at the search radius, non-finite input.
"""
import ctypes as C

import numpy as np
import pytest

import dihedral_ref as DR
import free_volume_ref as R

pytestmark = pytest.mark.gpu

COUNTS = ("hist", "occupied", "n_free", "free_map")


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _same(got, want, F, G):
    for key in COUNTS:
        print(key, "mismatches", int((np.asarray(got[key]) != np.asarray(want[key])).sum()))
    print("beyond", got["beyond"], want["beyond"])
    bad = np.argwhere(np.asarray(got["s"]).view(np.uint64) != want["s"].view(np.uint64))
    print("s mismatches", len(bad), bad[:5].tolist(), "nearest mismatches", int((got["nearest"] != want["nearest"]).sum()))
    assert R.same_bits(got["s"], want["s"])
    assert got["nearest"].dtype == np.int32 and np.array_equal(got["nearest"], want["nearest"])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"])
    assert got["occupied"].dtype == np.uint64 and np.array_equal(got["occupied"], want["occupied"])
    assert got["beyond"] == want["beyond"]
    assert got["n_free"].dtype == np.int64 and np.array_equal(got["n_free"], want["n_free"])
    assert got["free_map"].dtype == np.uint32 and np.array_equal(got["free_map"], want["free_map"])
    assert int(got["hist"].sum()) + int(got["occupied"].sum()) + got["beyond"] == F * G


def _check(B, xyz, box, cls, radius, grid, r_search, edges, probe=(0.0,), want=None):
    """Every output of one call against the restatement; -> (library's dict, restatement's dict)."""
    want = want or R.free_volume(xyz, box, cls, radius, grid, r_search, edges, probe)
    got = B.free_volume(xyz, box, cls, radius, grid, r_search, edges, probe, want_map=True, field=True)
    _same(got, want, np.shape(xyz)[0], int(np.prod(grid)))
    return got, want


def _system(rng, F, n, L, n_classes=3, ignored=0):
    """Coordinates [F,3,n] anywhere within a box or two of the cell of edges L [F,3], classes with `ignored` atoms left out."""
    x = (rng.random((F, 3, n)) * 3.0 - 1.0) * L[:, :, None]
    cls = rng.integers(0, n_classes, size=n).astype(np.int32)
    cls[rng.choice(n, size=ignored, replace=False)] = -1
    return np.ascontiguousarray(x), cls


EDGES = np.arange(41) * 0.0625      # 40 bins up to 2.5
RADII = np.array([0.5, 1.0, 1.5])


def test_three_frames_with_different_boxes_on_an_odd_grid(B):
    rng = np.random.default_rng(1)
    L = np.array([11.3, 9.7, 13.1]) + rng.random((3, 3)) * 0.4
    x, cls = _system(rng, 3, 220, L, ignored=20)
    assert [R.cells(v, 4.0) for v in L[0]] == [2, 2, 3]
    got, _ = _check(B, x, L, cls, RADII, (17, 13, 19), 4.0, EDGES, probe=(0.0, 0.25, 1.0))
    assert got["occupied"].all() and got["hist"].sum() > 0 and (np.diff(got["n_free"], axis=1) < 0).all()


@pytest.mark.parametrize("box,nc", [((6.0, 14.0, 14.0), (1, 3, 3)), ((6.0, 7.0, 14.0), (1, 1, 3)), ((6.0, 6.5, 7.0), (1, 1, 1)),
                                    ((9.0, 14.0, 14.0), (2, 3, 3)), ((9.0, 9.5, 14.0), (2, 2, 3)), ((9.0, 9.5, 10.0), (2, 2, 2)),
                                    ((6.0, 9.0, 14.0), (1, 2, 3))], ids=str)
def test_one_and_two_cells_on_an_axis(B, box, nc):
    """r_search = 4: an edge of 6 has one cell and lies below 2 r_search (the same atom is within reach through two
    images: the single wrap picks the nearer), an edge of 9 has two cells (c - 1 and c + 1 are the same cell)."""
    rng = np.random.default_rng(int(sum(box) * 10))
    L = np.tile(np.array(box), (2, 1))
    assert tuple(R.cells(v, 4.0) for v in box) == nc
    x, cls = _system(rng, 2, 150, L, ignored=10)
    _check(B, x, L, cls, RADII, (11, 9, 13), 4.0, EDGES)


def test_many_cells_most_sparse_some_empty(B):
    rng = np.random.default_rng(40)
    L = np.full((1, 3), 40.0)
    x, cls = _system(rng, 1, 2000, L)
    x[0, :, :600] = x[0, :, :600] * 0.05 + 3.0      # a blob; and a slab without atoms:
    x[0, 2] = np.where(np.mod(x[0, 2], 40.0) > 30.0, x[0, 2] - 12.0, x[0, 2])
    assert R.cells(40.0, 2.5) == 15
    got, _ = _check(B, x, L, cls, RADII[:3] * 0.8, (40, 40, 40), 2.5, np.arange(21) * 0.0625)
    assert got["beyond"] > 1000 and (got["nearest"] < 0).sum() > 1000


def test_every_atom_ignored(B):
    rng = np.random.default_rng(5)
    L = np.full((2, 3), 9.0)
    x, _ = _system(rng, 2, 50, L)
    got, _ = _check(B, x, L, np.full(50, -1, dtype=np.int32), RADII, (7, 5, 6), 3.0, EDGES, probe=(0.0, 2.5))
    assert got["beyond"] == 2 * 210 and (got["n_free"] == 210).all() and (got["free_map"] == 2).all()
    assert np.isinf(got["s"]).all() and (got["nearest"] == -1).all() and not got["hist"].any()


def test_exact_ties_faces_and_the_search_radius_on_a_dyadic_grid(B):
    """L = 8, g = 8: the points sit at .5. r_search = 3.5 gives two cells of edge 4 per axis, faces at 0, 4 and 8. Every
    operation is exact, so the facts below are arithmetic, not luck."""
    L = np.full((1, 3), 8.0)
    x = np.array([[[3.5, 4.0, 8.0, -0.0, -1.0, 3.5 + 24.0],
                   [0.5, 4.5, 2.5, 6.5, 4.0, 6.5],
                   [0.5, 4.5, 6.5, 2.5, 0.0, 4.5 - 16.0]]])
    cls = np.array([0, 1, 2, 2, 1, 2], dtype=np.int32)
    radius = np.array([3.0, 0.25, 0.125])
    edges = np.arange(29) * 0.125                                  # up to 3.5
    assert R.cells(8.0, 3.5) == 2
    got, want = _check(B, x, L, cls, radius, (8, 8, 8), 3.5, edges, probe=(0.0, 0.125))
    s, near = got["s"][0], got["nearest"][0]
    # atom 0 at (3.5, .5, .5), R = 3: the points (0,0,0) and (6,0,0) are exactly on its surface: s == 0, bin 0, free at probe 0
    assert s[0, 0, 0] == 0.0 and near[0, 0, 0] == 0 and s[6, 0, 0] == 0.0
    assert got["free_map"][0, 0, 0] == 1 and want["hist"][0, 0] >= 2
    # atom 1 at (4, 4.5, 4.5) is exactly r_search = 3.5 from the point (0, 4, 4): not a candidate there
    assert near[0, 4, 4] != 1 and near[1, 4, 4] == 1 and s[1, 4, 4] == 2.5 - 0.25
    # x = L is x = 0, -0.0 is 0, -1 is 7, and 27.5 is 3.5 three boxes on
    assert near[0, 2, 6] == 2 and s[0, 2, 6] == 0.5 - 0.125 and near[7, 2, 6] == 2
    assert near[0, 6, 2] == 3 and near[7, 4, 0] == 4
    assert near[3, 6, 4] == 5 and s[3, 6, 4] == -0.125


def test_the_lower_index_lines_a_tie(B):
    """Two atoms of different classes at equal s = 0.5 from the point (0, 0, 0): 1 away with R = 0.5, 2 away with R = 1.5."""
    L = np.full((1, 3), 8.0)
    a, b = np.array([1.5, 0.5, 0.5]), np.array([0.5, 2.5, 0.5])
    radius, edges = np.array([0.5, 1.5]), np.arange(25) * 0.125
    for first, second, classes in ((a, b, [0, 1]), (b, a, [1, 0])):
        x = np.stack([first, second], axis=1)[None]
        got, _ = _check(B, x, L, np.array(classes, dtype=np.int32), radius, (8, 8, 8), 3.0, edges)
        assert got["s"][0, 0, 0, 0] == 0.5 and got["nearest"][0, 0, 0, 0] == 0
    # the lining of that point followed the index: the histograms of the two calls differ by that one point
    x = np.stack([a, b], axis=1)[None]
    h0 = B.free_volume(x, L, np.array([0, 1], dtype=np.int32), radius, (8, 8, 8), 3.0, edges)["hist"]
    x = np.stack([b, a], axis=1)[None]
    h1 = B.free_volume(x, L, np.array([1, 0], dtype=np.int32), radius, (8, 8, 8), 3.0, edges)["hist"]
    d = h0.astype(np.int64) - h1.astype(np.int64)
    assert d[0, 4] == 1 and d[1, 4] == -1 and np.abs(d).sum() == 2


def test_all_atoms_in_one_cell_several_staging_chunks(B):
    rng = np.random.default_rng(3000)
    L = np.full((1, 3), 12.0)
    x = (0.1 + 3.8 * rng.random((1, 3, 3000)))
    cls = rng.integers(0, 3, size=3000).astype(np.int32)
    assert R.cells(12.0, 3.0) == 3 and 3000 > 2 * R.CHUNK
    got, _ = _check(B, x, L, cls, RADII * 0.2, (12, 12, 12), 3.0, np.arange(25) * 0.125)
    assert got["beyond"] > 0


@pytest.mark.parametrize("n", [255, 257, 70001])
def test_atom_counts_beyond_a_workgroup(B, n):
    """The pre-pass sorts through counters in device memory and has no limit of its own; 70 001 atoms are more than a
    workgroup could sort in LDS (160 KiB), 255 / 257 stand on either side of its 256 lanes."""
    rng = np.random.default_rng(n)
    L = np.array([[12.0, 13.0, 14.0]])
    x, cls = _system(rng, 1, n, L, ignored=n // 10)
    radius = RADII * (0.6 if n < 1000 else 0.05)
    _check(B, x, L, cls, radius, (6, 5, 7), 3.0, EDGES)


def test_a_flat_grid_with_bricks_of_many_points(B):
    rng = np.random.default_rng(65537)
    L = np.array([[64.0, 3.0, 3.0]])
    x, cls = _system(rng, 1, 40, L)
    assert [R.cells(v, 2.0) for v in L[0]] == [31, 1, 1] and 65537 // 31 > 2 * R.BRICK
    _check(B, x, L, cls, RADII * 0.5, (65537, 1, 1), 2.0, np.arange(17) * 0.125, probe=(0.0, 1.0))


def test_frames_beyond_any_launch_dimension(B):
    """65 540 frames of 2 atoms on a 2 x 2 x 2 grid: 20 different frames (boxes included) over and over, so that the
    restatement is formed once per different frame."""
    rng = np.random.default_rng(65540)
    K, F = 20, 65540
    L = 5.0 + rng.random((K, 3))
    x, _ = _system(rng, K, 2, L)
    cls = np.array([0, 1], dtype=np.int32)
    radius, edges, probe = np.array([0.5, 1.0]), np.arange(9) * 0.25, (0.0, 0.5)
    one = R.free_volume(x, L, cls, radius, (2, 2, 2), 2.0, edges, probe)
    reps = -(-F // K)
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps, axis=0)[:F])  # noqa: E731
    xs, Ls = tile(x), tile(L)
    s, near = tile(one["s"]), tile(one["nearest"])
    want = R.counts(s.reshape(F, 8), near.reshape(F, 8), cls, 2, edges, probe, (2, 2, 2))
    want["s"], want["nearest"] = s, near
    _check(B, xs, Ls, cls, radius, (2, 2, 2), 2.0, edges, probe, want=want)


def test_several_batches_and_host_against_device_input(B):
    import torch

    from mdproptools_amd._lib import default_context

    rng = np.random.default_rng(7)
    F = 7
    L = np.array([10.0, 11.0, 12.0]) + rng.random((F, 3))
    x, cls = _system(rng, F, 120, L, ignored=5)
    args = (L, cls, RADII, (9, 10, 11), 3.0, EDGES, (0.0, 0.5))
    got, want = _check(B, x, *args)
    ctx = default_context()
    ctx.set_option("free_volume_batch", 3)          # 3 + 3 + 1 frames
    try:
        _check(B, x, *args, want=want)
        xd = torch.as_tensor(x, device="cuda")
        _check(B, xd, *args, want=want)
        s = torch.empty((F, 9, 10, 11), dtype=torch.float64, device="cuda")
        near = torch.empty((F, 9, 10, 11), dtype=torch.int32, device="cuda")
        dev = B.free_volume(xd, *args, out=(s, near))
        torch.cuda.synchronize()
        assert R.same_bits(s.cpu().numpy(), want["s"]) and np.array_equal(near.cpu().numpy(), want["nearest"])
        assert dev["free_map"] is None and np.array_equal(dev["hist"], want["hist"])
    finally:
        ctx.set_option("free_volume_batch", 0)
    dev = B.free_volume(torch.as_tensor(x, device="cuda"), *args, want_map=True, field=True)
    _same(dev, want, F, 990)


def test_with_and_without_each_optional_output(B):
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    rng = np.random.default_rng(9)
    L = np.full((2, 3), 10.0)
    x, cls = _system(rng, 2, 90, L)
    args = (x, L, cls, RADII, (8, 9, 10), 3.0, EDGES, (0.0, 0.75))
    want = R.free_volume(*args)
    for kw in (dict(), dict(want_map=True), dict(field=True), dict(counts=False), dict(counts=False, want_map=True, field=True)):
        got = B.free_volume(*args, **kw)
        assert np.array_equal(got["n_free"], want["n_free"])
        assert (got["hist"] is None and got["beyond"] is None) if kw.get("counts") is False else (
            np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["occupied"], want["occupied"])
            and got["beyond"] == want["beyond"])
        assert got["free_map"] is None if not kw.get("want_map") else np.array_equal(got["free_map"], want["free_map"])
        assert got["s"] is None if not kw.get("field") else R.same_bits(got["s"], want["s"])
    # each output alone through the C interface, and none at all
    ctx = default_context()
    g, pr, rad = np.array([8, 9, 10], dtype=np.int32), np.array([0.0, 0.75]), RADII.copy()
    outs = {"hist": np.zeros((3, 40), dtype=np.uint64), "occupied": np.zeros(3, dtype=np.uint64), "beyond": np.zeros(1, dtype=np.uint64),
            "n_free": np.zeros((2, 2), dtype=np.int64), "free_map": np.zeros((8, 9, 10), dtype=np.uint32),
            "s": np.zeros((2, 8, 9, 10)), "nearest": np.zeros((2, 8, 9, 10), dtype=np.int32)}
    types = {"hist": C.c_uint64, "occupied": C.c_uint64, "beyond": C.c_uint64, "n_free": C.c_int64, "free_map": C.c_uint32}

    def call(names, null=None):
        a = [None if k not in names else (C.c_void_p(outs[k].ctypes.data) if k in ("s", "nearest") else ptr(outs[k], types[k]))
             for k in outs]
        ins = [C.c_void_p(x.ctypes.data), ptr(L), ptr(cls, C.c_int32), ptr(rad), ptr(g, C.c_int32), ptr(EDGES), ptr(pr)]
        if null is not None:
            ins[null] = None
        return ctx.lib.mdhip_free_volume(ctx.h, 2, 90, ins[0], 0, ins[1], ins[2], 3, ins[3], ins[4], 3.0, 9.0, 40, ins[5], 2,
                                         ins[6], *a, 0)

    for k in outs:
        outs[k][...] = 0
        ctx.check(call([k]))
        assert np.array_equal(outs[k].ravel(), np.asarray(want[k]).ravel()), k
    with pytest.raises(MdhipError):
        ctx.check(call([]))
    for k in range(7):   # a NULL input array: xyz, box, atom_class, radius, grid, edges, probe
        with pytest.raises(MdhipError):
            ctx.check(call(["n_free"], null=k))
    assert np.array_equal(outs["n_free"], want["n_free"])   # nothing was written by the refused calls


def test_rows_beyond_the_lds_bins(B):
    """16 classes x 4096 bins do not fit the workgroup's LDS bins: the counts go straight to the device cells."""
    rng = np.random.default_rng(16)
    L = np.full((2, 3), 10.0)
    x, _ = _system(rng, 2, 160, L)
    cls = (np.arange(160) % 16).astype(np.int32)
    assert 16 * 4096 > R.LDS_CELLS
    _check(B, x, L, cls, np.linspace(0.2, 0.9, 16), (10, 9, 8), 3.0, np.arange(4097) * (2.0 / 4096))


def test_non_finite_coordinates_vanish(B):
    rng = np.random.default_rng(13)
    L = np.array([10.0, 11.0, 12.0]) + rng.random((2, 3))
    x, cls = _system(rng, 2, 100, L)
    bad = x.copy()
    bad[0, 0, 3], bad[0, 1, 40], bad[1, 2, 77], bad[1, 0, 78] = np.nan, np.inf, -np.inf, np.nan
    got, _ = _check(B, bad, L, cls, RADII, (9, 8, 10), 3.0, EDGES)
    # the same as leaving those atoms out of the frame they are bad in: frame by frame, with the class set to -1
    for f, gone in ((0, [3, 40]), (1, [77, 78])):
        c = cls.copy()
        c[gone] = -1
        ref = B.free_volume(x[f:f + 1], L[f:f + 1], c, RADII, (9, 8, 10), 3.0, EDGES, field=True)
        assert R.same_bits(ref["s"][0], got["s"][f]) and np.array_equal(ref["nearest"][0], got["nearest"][f])


def test_arguments_are_refused_before_anything_is_written(B):
    from mdproptools_amd._lib import MdhipError

    rng = np.random.default_rng(2)
    L = np.full((1, 3), 10.0)
    x, cls = _system(rng, 1, 30, L)
    good = dict(xyz=x, box=L, atom_class=cls, radius=RADII, grid=(4, 4, 4), r_search=3.0, edges=EDGES, probe=(0.0,))
    B.free_volume(**good)
    bad = [dict(radius=np.full(17, 1.0)), dict(radius=np.array([1.0, -0.5, 1.0])), dict(radius=np.array([1.0, np.nan, 1.0])),
           dict(edges=np.arange(4098) * 0.001), dict(edges=np.array([0.0])), dict(edges=np.array([0.125, 0.5])),
           dict(edges=np.array([0.0, 0.5, 0.5])), dict(probe=np.zeros(9)), dict(probe=()), dict(probe=(-0.125,)),
           dict(probe=(np.nan,)), dict(probe=(2.75,)), dict(grid=(0, 4, 4)), dict(grid=(1 << 14, 1 << 14, 1)),
           dict(r_search=0.0), dict(r_search=np.inf), dict(r_search=-1.0), dict(atom_class=np.where(cls == 2, 3, cls)),
           dict(atom_class=np.where(cls == 2, -2, cls)), dict(box=np.array([[10.0, 0.0, 10.0]])),
           dict(box=np.array([[10.0, np.inf, 10.0]]))]
    for change in bad:
        with pytest.raises((MdhipError, ValueError)):
            B.free_volume(**dict(good, **change))
        print("refused", {k: np.shape(v) for k, v in change.items()})


def test_calc_free_volume_end_to_end(B, tmp_path):
    """Dump files with boxes that change per frame and lower bounds that are not 0, against the tables formed from the
    restatement's counts."""
    import pandas as pd

    from mdproptools_amd.structural import free_volume as FV

    traj = DR.synthetic_trajectory(n_frames=5)
    pattern = DR.write_dumps(tmp_path, traj, file_order=[3, 0, 4, 1, 2])
    radii = {1: 1.5, 2: 1.25}
    got = FV.calc_free_volume(pattern, radii, DR.NUM_MOLS, DR.ATOMS_PER_MOL, grid_spacing=0.75, probe_radii=(0.0, 0.5),
                              bin_size=0.125, s_max=2.0, type_names={1: "A", 2: "B"}, map_file="occ.cube",
                              return_field=True, working_dir=str(tmp_path), save=True)
    L0 = traj["L"][3]                                   # the first frame in file order sets the grid
    g = tuple(int(np.ceil(v / 0.75 - 1e-9)) for v in L0)
    cls = (traj["types"] - 1).astype(np.int32)
    edges = np.arange(17) * 0.125
    want = R.free_volume(traj["x"], traj["L"], cls, [1.5, 1.25], g, 2.0 + 1.5, edges, (0.0, 0.5))
    vol = traj["L"].prod(axis=1)
    tabs = FV.tables(["A", "B"], [0.0, 0.5], edges, int(np.prod(g)), traj["steps"], vol, want["n_free"], want["hist"],
                     want["beyond"])
    assert sorted(k for k in got if isinstance(got[k], pd.DataFrame)) == sorted(FV.TABLES)
    for name in FV.TABLES:
        pd.testing.assert_frame_equal(got[name], tabs[name], check_exact=True)
        back = pd.read_csv(tmp_path / ("free_volume_%s.csv" % name), index_col=0)
        assert list(back.columns) == list(tabs[name].columns) and len(back) == len(tabs[name])
    assert R.same_bits(got["s"], want["s"]) and np.array_equal(got["nearest"], want["nearest"])
    assert np.array_equal(got["free_map"], want["free_map"] / 5.0)
    lines = (tmp_path / "occ.cube").read_text().splitlines()
    assert lines[0].startswith("free-volume occupancy") and [int(lines[k].split()[0]) for k in (3, 4, 5)] == list(g)
    # leaving type 2 out: its atoms are ignored, and no class B is left
    only = FV.calc_free_volume(pattern, {1: 1.5}, grid_spacing=0.75, bin_size=0.125, s_max=2.0, exclude_types=[2])
    c1 = np.where(cls == 0, 0, -1).astype(np.int32)
    w1 = R.free_volume(traj["x"], traj["L"], c1, [1.5], g, 3.5, edges)
    assert [c for c in only["distribution"].columns if c.startswith("p_")] == ["p_total", "p_type1"] and np.array_equal(only["frames"]["FFV_0"].to_numpy(), w1["n_free"][:, 0] / float(np.prod(g)))
    with pytest.raises(ValueError, match="atom type 2"):
        FV.calc_free_volume(pattern, {1: 1.5})
    nine = tmp_path / "nine"
    nine.mkdir()
    with pytest.raises(ValueError, match="return_field"):
        FV.calc_free_volume(DR.write_dumps(nine, DR.synthetic_trajectory(n_frames=9)), radii, grid_spacing=3.0, return_field=True)
