"""The packed pair sweep's periodic images: one wave-uniform image per (wave, tile, axis), the per-lane
fallback (the long box) and the exact queue (atoms outside the cell) — bit for bit against the C oracle per frame and
against the all-f64 sweep, at the smallest size the culled path takes (2048 atoms = 8 tiles, `rdf_cull` forced: the
plan's estimate would choose the dense sweep here)."""
import numpy as np
import pytest

from oracle import cref as C

pytestmark = pytest.mark.gpu

N = 2048
REL = np.array([[1, 1], [1, 2], [2, 3], [3, 3]])
TY = (1 + np.arange(N) % 3).astype(np.int32)
PACKED = ("<3,", "<4,")


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ctxs():
    from mdproptools_amd._lib import Context

    pk, f64 = Context(0), Context(0)
    for ctx, v in ((pk, 1), (f64, 0)):
        ctx.set_option("rdf_cull", 1)
        ctx.set_option("rdf_pk", v)
    yield pk, f64
    pk.close()
    f64.close()


def slab_frame(rng, L, axis, n=N):
    """Atoms in two slabs hugging opposite faces on `axis`: [0, 3) and [L - 3, L), uniform on the other two axes."""
    L = np.broadcast_to(np.asarray(L, dtype=float), (3,))
    x = rng.uniform(0, 1, (3, n)) * L[:, None]
    s = rng.uniform(0, 3, n)
    x[axis] = np.where(rng.integers(0, 2, n) == 1, L[axis] - 3.0 + s, s)
    return x


def check_rdf(B, ctxs, xyz, box, r_cut, nbins, ty=TY, rel=REL, kernels=PACKED):
    pk, f64 = ctxs
    a = B.rdf_loop(xyz, ty, box, rel, r_cut, 0.05, nbins, ctx=pk)
    name = pk.last_kernel_name()
    assert any(t in name for t in kernels), name
    b = B.rdf_loop(xyz, ty, box, rel, r_cut, 0.05, nbins, ctx=f64)
    assert not any(t in f64.last_kernel_name() for t in ("<3,", "<4,", "<5,", "<6,")), f64.last_kernel_name()
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]
    for f in range(xyz.shape[0]):
        cf, cp, _ = C.rdf_pairs(xyz[f], ty, rel, box[f], r_cut * r_cut, 0.05, nbins)
        np.testing.assert_array_equal(a[0][f], cf, err_msg="frame %d" % f)
        np.testing.assert_array_equal(a[1][f], cp, err_msg="frame %d" % f)
    return a


@pytest.mark.parametrize("r_cut,nbins", [(10.0, 200), (12.45, 249)])
def test_cutoff_near_half_the_box(B, ctxs, r_cut, nbins):
    """Cubic L = 25: r_cut = 10 and r_cut = 12.45, just under L/2, where the plain threshold L - r_cut is smallest."""
    rng = np.random.default_rng(4101)
    L = 25.0
    xyz = rng.uniform(0, L, (3, 3, N))
    check_rdf(B, ctxs, xyz, np.full((3, 3), L), r_cut, nbins)


@pytest.mark.parametrize("r_cut,nbins", [(10.0, 200), (12.45, 249)])
def test_slabs_on_every_axis(B, ctxs, r_cut, nbins):
    """Two slabs hugging opposite faces, one frame per axis: most waves straddle some tile's +-L/2 plane, and the
    groups of the far slab lie wholly at the other image of the wave."""
    rng = np.random.default_rng(4102)
    L = 25.0
    xyz = np.stack([slab_frame(rng, L, axis) for axis in range(3)])
    full = check_rdf(B, ctxs, xyz, np.full((3, 3), L), r_cut, nbins)[0]
    assert int(full.sum()) > 0


def test_orthorhombic_and_varying_boxes(B, ctxs):
    rng = np.random.default_rng(4103)
    L = np.array([25.0, 31.0, 40.0])
    xyz = np.stack([rng.uniform(0, 1, (3, N)) * L[:, None], slab_frame(rng, L, 1), slab_frame(rng, L, 2)])
    check_rdf(B, ctxs, xyz, np.tile(L, (3, 1)), 10.0, 200)
    # a box that differs from frame to frame
    box = np.array([[25.0, 31.0, 40.0], [26.5, 24.0, 33.0], [40.0, 25.5, 27.0], [24.0, 24.0, 24.0]])
    xyz = np.stack([slab_frame(rng, box[f], f % 3) if f % 2 else rng.uniform(0, 1, (3, N)) * box[f][:, None]
                    for f in range(4)])
    check_rdf(B, ctxs, xyz, box, 10.0, 200)


def test_atoms_outside_the_cell(B, ctxs):
    """A tenth of the atoms moved by exactly +L or -L on a random axis, on a uniform and on a slab frame: every tile is
    then about 3 L wide (`he >= 0.9 L`), no tile is covered and every pair goes through the exact queue. And a frame with
    a handful moved by 2 L, whose tiles go to the exact queue while the others stay packed."""
    rng = np.random.default_rng(4104)
    L = 25.0
    xyz = np.stack([rng.uniform(0, L, (3, N)), slab_frame(rng, L, 0), rng.uniform(0, L, (3, N))])
    for f in range(2):
        who = rng.choice(N, N // 10, replace=False)
        xyz[f, rng.integers(0, 3, who.size), who] += L * rng.choice([-1.0, 1.0], who.size)
    who = rng.choice(N, 6, replace=False)
    xyz[2, rng.integers(0, 3, who.size), who] += 2.0 * L * rng.choice([-1.0, 1.0], who.size)
    check_rdf(B, ctxs, xyz, np.full((3, 3), L), 10.0, 200)
    check_rdf(B, ctxs, xyz[:2], np.full((2, 3), L), 12.45, 249)


def long_box_frames(n_frames=2):
    """Uniform atoms in a (25, 25, 100) box at r_cut 10: the tiles are long on z, `s_cap` (79 here) lies below
    L_z/2 + h_wave + h_tile for the waves that straddle a tile's +-L_z/2 plane, and the 1.49 L clause does not catch them
    first — swept groups on the per-lane fallback (tests/test_wrap_share_cpu.py counts them in the model)."""
    rng = np.random.default_rng(4108)
    box = np.array([25.0, 25.0, 100.0])
    return rng.uniform(0, 1, (n_frames, 3, N)) * box[None, :, None], np.tile(box, (n_frames, 1))


def test_per_lane_fallback_on_a_long_box(B, ctxs):
    """The fallback axis of sj_item_pk with effect: covered tiles whose groups are swept at the per-lane image."""
    xyz, box = long_box_frames()
    check_rdf(B, ctxs, xyz, box, 10.0, 200)
    # the same with the long axis on x and on y (the fallback mask's other bits)
    for perm in ([2, 0, 1], [1, 2, 0]):
        check_rdf(B, ctxs, np.ascontiguousarray(xyz[:1, perm]), box[:1, perm], 10.0, 200)


def test_rdf_and_cn_from_one_sweep_on_the_slab_frames(B, ctxs):
    """rdf_cn_loop (the CN-checking instantiations) against cn_loop, the all-f64 sweep and the oracle."""
    pk, f64 = ctxs
    rng = np.random.default_rng(4105)
    L = 25.0
    xyz = np.stack([slab_frame(rng, L, axis) for axis in range(3)])
    box = np.full((3, 3), L)
    cuts = [3.0, 9.975, 6.2, 9.99]
    full, part, ov, cn = B.rdf_cn_loop(xyz, TY, box, REL, 10.0, 0.05, 200, cuts, ctx=pk)
    name = pk.last_kernel_name()
    assert any(t in name for t in PACKED) and name.endswith(", true>"), name  # the CN-checking instantiation
    f2, p2, o2, cn2 = B.rdf_cn_loop(xyz, TY, box, REL, 10.0, 0.05, 200, cuts, ctx=f64)
    np.testing.assert_array_equal(full, f2)
    np.testing.assert_array_equal(part, p2)
    np.testing.assert_array_equal(cn, cn2)
    assert ov == o2
    np.testing.assert_array_equal(cn, B.cn_loop(xyz, TY, box, REL, cuts, ctx=f64))
    for f in range(3):
        cf, cp, _ = C.rdf_pairs(xyz[f], TY, REL, box[f], 100.0, 0.05, 200)
        np.testing.assert_array_equal(full[f], cf)
        np.testing.assert_array_equal(part[f], cp)
        np.testing.assert_array_equal(cn[f], C.cn_pairs(xyz[f], TY, REL, box[f], [c * c for c in cuts]))


def test_atoms_x_sites(B, ctxs):
    pk, f64 = ctxs
    rng = np.random.default_rng(4106)
    L = 25.0
    xyz = np.stack([slab_frame(rng, L, 0), rng.uniform(0, L, (3, N))])
    sites = np.stack([slab_frame(rng, L, 0), slab_frame(rng, L, 2)])
    sites[:, :, :30] = xyz[:, :, :30]
    st = (1 + np.arange(N) % 2).astype(np.int32)
    rel = np.array([[1, 1], [2, 2], [3, 1], [3, 2]])
    box = np.full((2, 3), L)
    a = B.rdf_mol_loop(xyz, TY, sites, st, box, rel, 10.0, 0.05, 200, ctx=pk)
    assert any(t in pk.last_kernel_name() for t in PACKED), pk.last_kernel_name()
    b = B.rdf_mol_loop(xyz, TY, sites, st, box, rel, 10.0, 0.05, 200, ctx=f64)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1]
    for f in range(2):
        want = C.rdf_rect(xyz[f], TY, sites[f], st, rel, box[f], 100.0, 0.05, 200)
        np.testing.assert_array_equal(a[0][f], want[0])


def test_nine_types_with_class_rows(B):
    """Every unordered pair of nine types named: the class-row form of the packed sweep (`<5` / `<6`, ROWS)."""
    from mdproptools_amd._lib import Context

    rng = np.random.default_rng(4107)
    L = 25.0
    xyz = np.stack([slab_frame(rng, L, 1), rng.uniform(0, L, (3, N))])
    ty = rng.integers(1, 10, N).astype(np.int32)
    rel = np.array([[a, b] for a in range(1, 10) for b in range(a, 10)])
    pk, f64 = Context(0), Context(0)
    try:
        for ctx, opts in ((pk, {"rdf_big": 0}), (f64, {"rdf_pk": 0})):
            ctx.set_option("rdf_cull", 1)
            for k, v in opts.items():
                ctx.set_option(k, v)
        check_rdf(B, (pk, f64), xyz, np.full((2, 3), L), 10.0, 200, ty=ty, rel=rel, kernels=("<5,", "<6,"))
    finally:
        pk.close()
        f64.close()
