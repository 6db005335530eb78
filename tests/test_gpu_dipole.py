"""mdhip_mol_moments, mdhip_vector_pair_hist and the two drop-ins on top of them against tests/dipole_ref.py, which
restates include/mdhip.h operation by operation: every output is compared with == or bit for bit. The shapes are the
smallest at which the kernels can go wrong: either side of the 64-molecule and 64-frame tile, of the 64-lane tile of the
pair sweep with either group on the lanes, more than one workgroup, more than 65 535 jobs, more uniform entities than
one chunk of 2^20."""
import ctypes as C
import math

import numpy as np
import pytest

import dipole_ref as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


# ---- mol_moments -------------------------------------------------------------------------------------------------------


def _check_moments(B, x, box, a0, mols, length, site_terms, vec_terms, unit, want_deg=None):
    want = D.mol_moments(x, box, a0, mols, length, site_terms, vec_terms, unit)
    got = B.mol_moments(x, box, a0, mols, length, site_terms, vec_terms, unit, totals=True)
    for name in ("site", "vec", "total", "sq_total"):
        assert got[name].shape == want[name].shape, name
        bad = np.argwhere(~((got[name] == want[name]) | (np.isnan(got[name]) & np.isnan(want[name]))))
        print(name, got[name].shape, "mismatches", len(bad), bad[:5].tolist())
        assert D.same_bits(got[name], want[name]), name
    assert got["degenerate"].tolist() == want["degenerate"].tolist()
    if want_deg is not None:
        assert got["degenerate"].tolist() == list(want_deg)
    return got


def _molecules(rng, F, mols, per, L):
    """Wrapped coordinates [F,3,mols*per] of molecules about 2 wide placed anywhere in boxes L [F,3]."""
    centre = rng.random((F, 3, mols, 1)) * L[:, :, None, None]
    x = centre + rng.normal(0.0, 0.7, size=(F, 3, mols, per))
    return np.ascontiguousarray(np.mod(x, L[:, :, None, None]).reshape(F, 3, mols * per))


def _five_jobs(mols):
    """Types: `mols` x 3 atoms, none x 2 atoms, `mols` x 2 atoms, 5 x 1 atom. Jobs: both lists and unit vectors; a job
    without molecules; no site terms and raw vectors; a site and no vector; neither (a monatomic ion)."""
    first = np.concatenate(([0], np.cumsum([3 * mols, 0, 2 * mols, 5])))
    a0, n, length = [first[0], first[1], first[2], first[0], first[3]], [mols, 0, mols, mols, 5], [3, 2, 2, 3, 1]
    site_terms = [[(1, 0.25), (2, 0.125)], [(1, 1.0)], [], [(2, 1.0)], []]
    vec_terms = [[(1, 0.4), (2, 0.4)], [(1, 1.0)], [(1, -1.5)], [], []]
    return int(first[-1]), a0, n, length, site_terms, vec_terms, [1, 1, 0, 1, 0]


@pytest.mark.parametrize("mols", [1, 63, 64, 65])
@pytest.mark.parametrize("F", [1, 63, 65])
def test_moments_either_side_of_the_tile(B, mols, F):
    rng = np.random.default_rng(1000 * mols + F)
    L = 9.0 + rng.random((F, 3)) * 3.0                                    # a box of its own per frame and axis
    A, a0, n, length, site_terms, vec_terms, unit = _five_jobs(mols)
    x = np.concatenate([_molecules(rng, F, mols, 3, L), _molecules(rng, F, mols, 2, L), _molecules(rng, F, 5, 1, L)], axis=2)
    assert x.shape[2] == A
    got = _check_moments(B, x, L, a0, n, length, site_terms, vec_terms, unit, want_deg=[0] * 5)
    assert not got["vec"][:, :, -5:].any() and D.same_bits(got["site"][:, :, -5:], x[:, :, -5:])   # the ions: x[a] itself
    assert not got["total"][1].any() and not got["total"][3].any() and not got["total"][4].any()
    # molecules do cross faces: the single wrap is at work
    assert mols * F < 1000 or (np.abs(x[:, :, 1:3 * mols:3] - x[:, :, 0:3 * mols:3]) > L[:, :, None] / 2).any()


def test_moments_at_the_faces(B):
    """Differences at, just below and just above +-L/2 (strict: exactly half an edge stays), one diatomic per case."""
    L = np.array([[8.0, 10.0, 6.0]])
    up, down = np.nextafter(5.0, np.inf), np.nextafter(5.0, -np.inf)
    cases = [(1.0, 5.0), (1.0, up), (1.0, down), (5.0, 1.0), (up, 1.0), (down, 1.0)]
    x = np.zeros((1, 3, 12))
    for m, (first, second) in enumerate(cases):
        x[0, 0, 2 * m], x[0, 0, 2 * m + 1] = first, second
    got = _check_moments(B, x, L, [0], [6], [2], [[(1, 0.5)]], [[(1, 1.0)]], [0])
    assert got["vec"][0, 0].tolist() == [4.0, (up - 1.0) - 8.0, down - 1.0, -4.0, (1.0 - up) + 8.0, 1.0 - down]
    assert got["site"][0, 0, 0] == 3.0 and got["site"][0, 0, 1] == 1.0 + 0.5 * ((up - 1.0) - 8.0)


def test_moments_unwrapped_and_device_tensors(B):
    import torch

    rng = np.random.default_rng(12)
    A, a0, n, length, site_terms, vec_terms, unit = _five_jobs(70)
    x = rng.normal(0.0, 30.0, size=(67, 3, A))                            # unwrapped: no box
    host = _check_moments(B, x, None, a0, n, length, site_terms, vec_terms, unit)
    xd = torch.from_numpy(x).cuda()
    S = host["site"].shape[2]
    site, vec = (torch.full((67, 3, S), 77.0, dtype=torch.float64, device="cuda") for _ in range(2))
    dev = B.mol_moments(xd, None, a0, n, length, site_terms, vec_terms, unit, site_out=site, vec_out=vec, totals=True)
    assert dev["site"] is site and dev["vec"] is vec
    assert site.cpu().numpy().tobytes() == host["site"].tobytes() and vec.cpu().numpy().tobytes() == host["vec"].tobytes()
    assert dev["total"].tobytes() == host["total"].tobytes() and dev["sq_total"].tobytes() == host["sq_total"].tobytes()
    # the same bits from another call, and the totals alone (no site, no vector written)
    only = B.mol_moments(x, None, a0, n, length, site_terms, vec_terms, unit, want_site=False, want_vec=False, totals=True)
    assert only["site"] is None and only["vec"] is None
    assert only["total"].tobytes() == host["total"].tobytes() and only["sq_total"].tobytes() == host["sq_total"].tobytes()
    with pytest.raises(ValueError, match="go together"):
        B.mol_moments(xd, None, a0, n, length, site_terms, vec_terms, unit, site_out=site)


def test_moments_zero_vectors_and_nan(B):
    rng = np.random.default_rng(13)
    x = rng.normal(size=(5, 3, 40 * 4))                                   # 40 molecules of 4 atoms; atom 3 is never named
    x[2, :, 4 * 7 + 1] = x[2, :, 4 * 7]                                    # molecule 7, frame 2: atom 1 on atom 0 -> zero vector
    x[3, :, 4 * 9 + 2] = x[3, :, 4 * 9]
    x[:, :, 3::4] = np.nan                                                # the unnamed atom: does not leak
    x[4, 1, 4 * 20 + 1] = np.nan                                          # a named one does, into its molecule, frame and axis
    site_terms, vec_terms = [[(2, 0.5)], [(2, 0.5)]], [[(1, 2.0)], [(2, -1.0)]]
    got = _check_moments(B, x, None, [0, 0], [40, 40], [4, 4], site_terms, vec_terms, [1, 1], want_deg=[1, 1])
    assert not got["vec"][2, :, 7].any() and not got["vec"][3, :, 40 + 9].any()
    assert np.isnan(got["vec"][4, :, 20]).all() and np.isnan(got["vec"]).sum() == 3       # the unit vector: all three axes
    assert np.isnan(got["total"][0, :, 4]).all() and np.isnan(got["total"]).sum() == 3 and np.isnan(got["sq_total"]).sum() == 1
    raw = _check_moments(B, x, None, [0], [40], [4], [[]], [[(1, 2.0)]], [0], want_deg=[0])   # raw vectors: never degenerate
    assert np.isnan(raw["vec"]).sum() == 1 and np.isnan(raw["total"]).sum() == 1            # ... and one axis only


def test_moments_totals(B):
    """Small-integer components: every order gives the same sum, compared with ==. Random vectors: within
    (W + 3) * 2^-53 * sum |term| of the exact sum of the terms as written, W their number — valid for any order — and
    the same bits as the restatement's fixed order, and from call to call."""
    rng = np.random.default_rng(14)
    mols, F = 1000, 3
    x = rng.integers(-50, 50, size=(F, 3, 2 * mols)).astype(np.float64)
    got = _check_moments(B, x, None, [0], [mols], [2], [[]], [[(1, 3.0)]], [0])
    d = 3.0 * (x[:, :, 1::2] - x[:, :, 0::2])
    assert np.array_equal(got["total"][0], d.sum(axis=2).T) and np.array_equal(got["sq_total"][0], (d * d).sum(axis=(1, 2)))
    x = rng.normal(0.0, 5.0, size=(F, 3, 2 * mols))
    got = _check_moments(B, x, None, [0], [mols], [2], [[]], [[(1, 0.7)]], [0])
    v = got["vec"]
    sq = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    for f in range(F):
        for ax in range(3):
            err = abs(got["total"][0, ax, f] - math.fsum(v[f, ax]))
            assert err <= (mols + 3) * D.EPS * np.abs(v[f, ax]).sum()
        assert abs(got["sq_total"][0, f] - math.fsum(sq[f])) <= (mols + 3) * D.EPS * sq[f].sum()
    again = B.mol_moments(x, None, [0], [mols], [2], [[]], [[(1, 0.7)]], [0], totals=True)
    assert again["total"].tobytes() == got["total"].tobytes() and again["sq_total"].tobytes() == got["sq_total"].tobytes()


def test_moments_beyond_the_launch_limits(B):
    """70 001 frames of three molecules, and one frame of 65 535 x 64 + 1 diatomics: one molecule tile more than a launch
    dimension holds."""
    rng = np.random.default_rng(15)
    x = rng.normal(size=(70001, 3, 6))
    _check_moments(B, x, None, [0], [3], [2], [[(1, 0.5)]], [[(1, 1.0)]], [1], want_deg=[0])
    mols = 65535 * 64 + 1
    x = rng.random(size=(1, 3, 2 * mols)) + 0.5
    x[0, :, 2 * (mols - 1) + 1] = x[0, :, 2 * (mols - 1)]            # the last molecule, alone in the second launch
    got = _check_moments(B, x, None, [0], [mols], [2], [[(1, 0.5)]], [[(1, 1.0)]], [1], want_deg=[1])
    assert not got["vec"][0, :, -1].any() and got["vec"][0, :, -2].any()


def test_moments_invalid_arguments(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    x = np.zeros((4, 3, 12))
    good = dict(n_jobs=2, a0=[0, 6], mols=[2, 2], length=[3, 3], s_off=[0, 2, 2], s_atom=[1, 2], v_off=[0, 1, 3],
                v_atom=[2, 1, 2], unit=[0, 1], F=4, A=12)
    bad = [dict(n_jobs=0), dict(n_jobs=-1), dict(a0=[0, 7]), dict(mols=[2, 3]), dict(mols=[-1, 2]), dict(a0=[-1, 6]),
           dict(length=[3, 0]), dict(s_atom=[0, 2]), dict(s_atom=[1, 3]), dict(s_atom=[2, 1]), dict(s_atom=[1, 1]),
           dict(v_atom=[2, 2, 2]), dict(v_atom=[3, 1, 2]), dict(v_atom=[2, 0, 2]), dict(s_off=[1, 2, 2]), dict(s_off=[0, 2, 1]),
           dict(v_off=[0, 3, 3]), dict(v_off=[0, 1, 4]), dict(unit=[0, 2]), dict(unit=[-1, 1]), dict(F=0), dict(A=0), dict(A=11),
           dict(null="x"), dict(null="degenerate"), dict(null="a0"), dict(null="mols"), dict(null="length"),
           dict(null="s_off"), dict(null="v_off"), dict(null="s_atom"), dict(null="s_w"), dict(null="v_atom"),
           dict(null="v_w"), dict(null="unit")]
    for change in bad:
        c = dict(good, **{k: v for k, v in change.items() if k != "null"})
        arr = {"a0": np.array(c["a0"], dtype=np.int64), "mols": np.array(c["mols"], dtype=np.int64),
               "length": np.array(c["length"], dtype=np.int32), "s_off": np.array(c["s_off"], dtype=np.int64),
               "s_atom": np.array(c["s_atom"], dtype=np.int32), "s_w": np.ones(4), "v_off": np.array(c["v_off"], dtype=np.int64),
               "v_atom": np.array(c["v_atom"], dtype=np.int32), "v_w": np.ones(4), "unit": np.array(c["unit"], dtype=np.int32)}
        site, vec = np.full((4, 3, 4), 77.0), np.full((4, 3, 4), 77.0)
        total, sq_total = np.full((2, 3, 4), 77.0), np.full((2, 4), 77.0)
        deg = np.full(2, 77, dtype=np.uint64)
        ctype = {np.dtype(np.int64): C.c_int64, np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double}
        args = {k: ptr(v, ctype[v.dtype]) for k, v in arr.items()}
        args.update(x=vp(x), degenerate=ptr(deg, C.c_uint64))
        if "null" in change:
            args[change["null"]] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_mol_moments(
                ctx.h, c["F"], c["A"], args["x"], 0, None, c["n_jobs"], args["a0"], args["mols"], args["length"],
                args["s_off"], args["s_atom"], args["s_w"], args["v_off"], args["v_atom"], args["v_w"], args["unit"],
                vp(site), vp(vec), 0, ptr(total), ptr(sq_total), args["degenerate"]))
        assert err.value.code == -1, change
        assert all((a == 77).all() for a in (site, vec, total, sq_total, deg)), change
    # ... and the arguments these were derived from are fine
    got = B.mol_moments(x + np.arange(12.0), None, good["a0"], good["mols"], good["length"], [[(1, 1.0), (2, 1.0)], []],
                        [[(2, 1.0)], [(1, 1.0), (2, 1.0)]], good["unit"], totals=True)
    assert got["site"].shape == (4, 3, 4) and not got["degenerate"].any()


# ---- vector_pair_hist --------------------------------------------------------------------------------------------------


def _unit_vectors(rng, shape):
    v = rng.normal(size=shape)
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None, :]


def _check_pairs(B, site, vec, box, off, jobs, bin_size, nbins, summed=True):
    from mdproptools_amd._lib import bin_edges

    want = D.vector_pair_hist(site, vec, box, off, jobs, bin_size, nbins, bin_edges(bin_size, nbins))
    got = B.vector_pair_hist(site, vec, box, np.asarray(off, dtype=np.int64), jobs, bin_size, nbins)
    names = ("hist", "sums", "beyond", "unsummed", "pairs")
    for name, g, w in zip(names, got, want):
        bad = np.argwhere(np.asarray(g != w))
        print(name, np.shape(g), "mismatches", len(bad), bad[:5].tolist())
        assert g.tolist() == w.tolist(), name
    hist, sums, beyond, unsummed, pairs = got
    assert (hist.sum(axis=1) + beyond).tolist() == pairs.tolist()
    if summed:
        assert not unsummed.any()  # (a condition of the test: unit vectors, distinct sites)
    return got


SIZES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def liquid():
    """Five groups of 1, 63, 64, 65 and 130 entities, three frames with a box of their own, sites anywhere within several
    box lengths of the cell, random unit vectors."""
    rng = np.random.default_rng(31)
    F, E = 3, sum(SIZES)
    box = 9.0 + rng.random((F, 3)) * 2.0
    site = (rng.random((F, 3, E)) + rng.integers(-3, 4, size=(F, 3, E))) * box[:, :, None]
    return site, _unit_vectors(rng, (F, 3, E)), box, np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)


def test_pairs_every_group_size_on_either_side(B, liquid):
    """All 25 ordered pairs of groups in one call, a == b included: whichever group the kernel puts on the lanes, e is
    the vector of b against a -> b, as the restatement has it."""
    site, vec, box, off = liquid
    jobs = [(a, b) for a in range(5) for b in range(5)]
    hist, sums, beyond, _, pairs = _check_pairs(B, site, vec, box, off, jobs, 0.25, 16)
    assert hist.sum() > 20000 and beyond.sum() > 0
    # small against large both ways: the same pairs and cosines, another direction cosine
    s = {j: k for k, j in enumerate(jobs)}
    assert hist[s[(0, 4)]].tolist() == hist[s[(4, 0)]].tolist() and sums[s[(0, 4)], 0].tolist() == sums[s[(4, 0)], 0].tolist()
    assert sums[s[(0, 4)], 2].tolist() != sums[s[(4, 0)], 2].tolist()
    assert any(v < 0 for v in sums[:, 0].ravel().tolist())


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("nbins", [1, 2, 4096])
def test_pairs_bins_and_frames(B, liquid, nbins, frames):
    site, vec, box, off = liquid
    _check_pairs(B, site[:frames], vec[:frames], box[:frames], off, [(3, 3), (1, 4), (4, 2)], 4.0 / nbins, nbins)


def test_pairs_axis_vectors_ties_and_negative_sums(B):
    """Vectors +-e_x, +-e_y, +-e_z: c and c^2 are 0 or +-1 and their sums exact multiples of 2^32. d * inv = +-0.5
    exactly: nothing shifts. Twenty pairs with c = -1 in one bin: the sum is negative and its high word all ones."""
    from mdproptools_amd._lib import default_context, ptr

    rng = np.random.default_rng(32)
    E = 150
    box = np.array([[8.0, 8.0, 16.0]])
    site = rng.integers(0, 8 * 16, size=(1, 3, E)) / 16.0                  # dyadic: ties at d = 4 on x and y do occur
    assert len(np.unique(site[0].T, axis=0)) == E
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    vec = np.ascontiguousarray(axes[rng.integers(0, 6, E)].T)[None]
    dx = site[0, 0][:, None] - site[0, 0][None, :]
    assert (np.abs(dx) == 4.0).sum() > 50
    hist, sums, _, _, _ = _check_pairs(B, site, vec, box, [0, 70, E], [(0, 0), (0, 1), (1, 0)], 0.5, 8)
    assert all(v % D.ONE == 0 for v in sums[:, :2].ravel().tolist()) and any(v % D.ONE for v in sums[:, 2].ravel().tolist())
    # ten far-apart columns of two entities 1.25 apart, vectors up and down: 20 ordered pairs, all in bin 2 of 4, c = -1
    site = np.zeros((1, 3, 20))
    site[0, 0] = np.repeat(np.arange(10.0) * 30.0, 2)                      # ten far-apart columns of two
    site[0, 2] = np.tile([0.0, 1.25], 10)
    vec = np.zeros((1, 3, 20))
    vec[0, 2] = np.tile([1.0, -1.0], 10)
    box = np.full((1, 3), 1000.0)
    hist, sums, beyond, _, _ = _check_pairs(B, site, vec, box, [0, 20], [(0, 0)], 0.5, 4)
    assert hist[0].tolist() == [0, 0, 20, 0] and sums[0, 0, 2] == -20 * D.ONE and sums[0, 2, 2] == -20 * D.ONE
    # the words themselves, straight from the C entry point
    ctx = default_context()
    words = np.full((1, 3, 4, 2), 77, dtype=np.uint64)
    h, bey, uns, prs = np.zeros((1, 4), dtype=np.uint64), *(np.zeros(1, dtype=np.uint64) for _ in range(3))
    off, jobs = np.array([0, 20], dtype=np.int64), np.array([[0, 0]], dtype=np.int32)
    ctx.check(ctx.lib.mdhip_vector_pair_hist(
        ctx.h, 1, 20, C.c_void_p(site.ctypes.data), C.c_void_p(vec.ctypes.data), 0, ptr(box), 1, ptr(off, C.c_int64), 1,
        ptr(jobs, C.c_int32), 0.5, 4, None, ptr(h, C.c_uint64), ptr(words, C.c_uint64), ptr(bey, C.c_uint64),
        ptr(uns, C.c_uint64), ptr(prs, C.c_uint64)))
    assert tuple(words[0, 0, 2].tolist()) == D.split_words(-20 * D.ONE) and words[0, 0, 2, 1] == 2 ** 64 - 1
    assert tuple(words[0, 1, 2].tolist()) == (20 * D.ONE, 0) and not words[0, :, [0, 1, 3]].any()


def test_pairs_that_cannot_be_summed_or_binned(B):
    """Coincident sites, a NaN vector and a vector of length 3: inside hist, counted in unsummed exactly, in no sum. A NaN
    site and a box edge of 0: beyond."""
    rng = np.random.default_rng(33)
    E = 70
    site = rng.random((2, 3, E)) * 6.0
    vec = _unit_vectors(rng, (2, 3, E))
    site[0, :, 5] = site[0, :, 4]                                         # coincident in frame 0
    vec[1, 1, 10] = np.nan
    vec[0, :, 20] *= 3.0
    site[1, 2, 30] = np.nan
    box = np.full((2, 3), 6.0)
    hist, sums, beyond, unsummed, pairs = _check_pairs(B, site, vec, box, [0, E], [(0, 0)], 0.5, 6, summed=False)
    assert 2 < unsummed[0] < 2 + 2 * 2 * (E - 1) + 1 and beyond[0] >= 2 * (E - 1)
    box[0, 1] = 0.0
    hist, _, beyond, unsummed, pairs = _check_pairs(B, site, vec, box, [0, E], [(0, 0)], 0.5, 6, summed=False)
    assert beyond[0] >= E * (E - 1)                                        # every pair of frame 0


def test_pairs_more_jobs_than_a_launch_holds(B):
    """65 537 jobs over three small groups: the job list goes in two launches. The nine different jobs are computed once."""
    from mdproptools_amd._lib import bin_edges

    rng = np.random.default_rng(34)
    E = 12
    site, vec, box = rng.random((1, 3, E)) * 5.0, _unit_vectors(rng, (1, 3, E)), np.full((1, 3), 5.0)
    off = np.array([0, 3, 8, 12], dtype=np.int64)
    nine = [(a, b) for a in range(3) for b in range(3)]
    want = D.vector_pair_hist(site, vec, box, off, nine, 1.0, 2, bin_edges(1.0, 2))
    pick = rng.integers(0, 9, 65537)
    pick[-1] = 5
    got = B.vector_pair_hist(site, vec, box, off, [nine[k] for k in pick], 1.0, 2)
    for name, g, w in zip(("hist", "sums", "beyond", "unsummed", "pairs"), got, want):
        assert np.array_equal(g, w[pick]), name
    assert got[0].sum() > 0


def test_pairs_and_van_hove_on_one_walker(B):
    """vp_pair_kernel and vh_pair_kernel step through the same units (csrc/group_pairs.h): on sites that are multiples of
    1/8 in a cubic box of edge 16 every difference, wrap and square is exact, the single wrap and the nearest image are
    the same number, and hist, beyond and pairs of the vector sweep equal those of the distinct van Hove function at
    lag 0, stride 1 — for every ordered pair of groups of 5, 64, 65 and 130 entities, a with a included."""
    import vanhove_ref as R

    from mdproptools_amd._lib import bin_edges

    rng = np.random.default_rng(35)
    sizes = [5, 64, 65, 130]
    F, E = 3, sum(sizes)
    site = rng.integers(0, 16 * 8, size=(F, 3, E)) / 8.0
    vec, box = _unit_vectors(rng, (F, 3, E)), np.full((F, 3), 16.0)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    jobs = [(a, b) for a in range(4) for b in range(4)]
    lagged = [(a, b, 0, 1) for a, b in jobs]
    # the premise, on the CPU: the two restatements agree on these inputs
    want_vh = R.van_hove_distinct(site, box, off, lagged, 0.25, 32)
    want_vp = D.vector_pair_hist(site, vec, box, off, jobs, 0.25, 32, bin_edges(0.25, 32))
    for w_vh, w_vp in zip(want_vh, (want_vp[0], want_vp[2], want_vp[4])):
        assert np.array_equal(w_vh, w_vp)
    assert want_vh[0].sum() > 10000 and want_vh[1].sum() > 10000
    hist, _, beyond, _, pairs = B.vector_pair_hist(site, vec, box, off, jobs, 0.25, 32)
    got_vh = B.van_hove_distinct(site, box, off, lagged, 0.25, 32)
    for name, g_vp, g_vh, w in zip(("hist", "beyond", "pairs"), (hist, beyond, pairs), got_vh, want_vh):
        assert g_vp.tolist() == g_vh.tolist(), name
        assert g_vp.tolist() == w.tolist(), name


def _long_group(rng):
    """One frame in a box of edge 64: group a of 64 entities, then 2^20 + 65 more, the last 65 of them within 2 of
    entity 0 -> (sites [1,3,E], box, group_off of (a, b), group_off of (a, b1, b2) with b split at 2^20 - 7)."""
    n_b = (1 << 20) + 65
    E = 64 + n_b
    site = rng.random((1, 3, E)) * 64.0
    site[0, :, -65:] = np.mod(site[0, :, :1] + rng.uniform(-1.0, 1.0, size=(3, 65)), 64.0)
    whole = np.array([0, 64, E], dtype=np.int64)
    return site, np.full((1, 3), 64.0), whole, np.array([0, 64, 64 + (1 << 20) - 7, E], dtype=np.int64)


def test_pairs_past_one_chunk_of_uniform_entities(B):
    """2^20 + 65 entities on the uniform side, the lanes holding a (job (a, b)) and holding b (job (b, a)): two chunks
    per tile. Every output equals the sum over the two parts of the long group, each of which is one chunk."""
    rng = np.random.default_rng(36)
    site, box, whole, split = _long_group(rng)
    vec = _unit_vectors(rng, site.shape)
    got = B.vector_pair_hist(site, vec, box, whole, [(0, 1), (1, 0)], 0.25, 16)
    part = B.vector_pair_hist(site, vec, box, split, [(0, 1), (0, 2), (1, 0), (2, 0)], 0.25, 16)
    for name, g, p in zip(("hist", "sums", "beyond", "unsummed", "pairs"), got, part):
        assert (p[0] + p[1]).tolist() == g[0].tolist(), name
        assert (p[2] + p[3]).tolist() == g[1].tolist(), name
    hist, sums, beyond, _, pairs = got
    assert pairs.tolist() == [64 * ((1 << 20) + 65)] * 2 and (hist.sum(axis=1) + beyond).tolist() == pairs.tolist()
    # the last 65 entities are all within reach of entity 0, and they are counted
    assert part[0][1].sum() >= 65 and part[0][0].sum() > 1000 and hist[0].sum() == part[0][0].sum() + part[0][1].sum()
    # the same pairs and cosines either way round, another direction cosine
    assert hist[0].tolist() == hist[1].tolist() and sums[0, 0].tolist() == sums[1, 0].tolist()
    assert sums[0, 2].tolist() != sums[1, 2].tolist()


def test_pairs_invalid_arguments(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    site, vec = np.zeros((2, 3, 10)), np.zeros((2, 3, 10))
    good = dict(F=2, E=10, box=np.full((2, 3), 5.0), G=2, off=[0, 4, 10], J=2, jobs=[[0, 1], [1, 1]], bin_size=0.5, nbins=4,
                edges=None)
    bad = [dict(F=-1), dict(E=-1), dict(E=9), dict(G=-1), dict(J=-1), dict(box=None), dict(off=[0, 5, 4]), dict(off=[-1, 4, 10]),
           dict(off=[0, 4, 11]), dict(jobs=[[0, 2], [1, 1]]), dict(jobs=[[0, 1], [-1, 1]]), dict(bin_size=0.0),
           dict(bin_size=-1.0), dict(bin_size=float("inf")), dict(bin_size=float("nan")), dict(nbins=0), dict(nbins=4097),
           dict(edges=[0.5, 1.0, 2.0, 3.0, 4.0]), dict(edges=[0.0, 1.0, 0.5, 3.0, 4.0]), dict(null="site"), dict(null="vec"),
           dict(null="off"), dict(null="jobs"), dict(null="hist"), dict(null="sums"), dict(null="beyond"),
           dict(null="unsummed"), dict(null="pairs")]
    for change in bad:
        c = dict(good, **{k: v for k, v in change.items() if k != "null"})
        off, jobs = np.array(c["off"], dtype=np.int64), np.array(c["jobs"], dtype=np.int32)
        edges = None if c["edges"] is None else np.array(c["edges"], dtype=np.float64)
        out = {"hist": np.full((2, 4), 77, dtype=np.uint64), "sums": np.full((2, 3, 4, 2), 77, dtype=np.uint64),
               "beyond": np.full(2, 77, dtype=np.uint64), "unsummed": np.full(2, 77, dtype=np.uint64),
               "pairs": np.full(2, 77, dtype=np.uint64)}
        args = {k: ptr(v, C.c_uint64) for k, v in out.items()}
        args.update(site=C.c_void_p(site.ctypes.data), vec=C.c_void_p(vec.ctypes.data), off=ptr(off, C.c_int64),
                    jobs=ptr(jobs, C.c_int32))
        if "null" in change:
            args[change["null"]] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_vector_pair_hist(
                ctx.h, c["F"], c["E"], args["site"], args["vec"], 0, None if c["box"] is None else ptr(c["box"]), c["G"],
                args["off"], c["J"], args["jobs"], c["bin_size"], c["nbins"], None if edges is None else ptr(edges),
                args["hist"], args["sums"], args["beyond"], args["unsummed"], args["pairs"]))
        assert err.value.code == -1, change
        assert all((a == 77).all() for a in out.values()), change
    # ... and the arguments these were derived from are fine: no entity within reach of itself, every pair at distance 0
    hist, sums, beyond, unsummed, pairs = B.vector_pair_hist(site, vec, good["box"], good["off"], good["jobs"], 0.5, 4)
    assert pairs.tolist() == [48, 60] and hist[:, 0].tolist() == [48, 60] and unsummed.tolist() == [48, 60]


# ---- the drop-ins ------------------------------------------------------------------------------------------------------

WATER, ION = (1, "dipole", 1), (2, None, "first")
PAIRS = [(WATER, WATER), (ION, WATER), ((1, (2, 3), "com"), ION)]
MASS = [16.0, 1.0, 23.0]


@pytest.fixture(scope="module")
def water(tmp_path_factory):
    d = tmp_path_factory.mktemp("dipole")
    traj = D.water_like()
    return {"dir": d, "pattern": D.write_dumps(d, traj), "traj": traj}


def _expected_frames(traj, r_cut, bin_size):
    """The restatement applied to the frames the dumps hold: three species, three pairs."""
    from mdproptools_amd._lib import bin_edges

    nbins = int(r_cut / bin_size)
    com = [(1, 1.0 / 18.0), (2, 1.0 / 18.0)]
    got = D.mol_moments(traj["x"], traj["L"], [0, 120, 0], [40, 6, 40], [3, 1, 3], [[], [], com],
                        [[(1, 0.4), (2, 0.4)], [], [(1, -1.0), (2, 1.0)]], [1, 1, 1])
    assert not got["degenerate"].any()
    off = np.array([0, 40, 46, 86], dtype=np.int64)
    jobs = [(0, 0), (1, 0), (2, 1)]
    hist, sums, beyond, unsummed, pairs = D.vector_pair_hist(got["site"], got["vec"], traj["L"], off, jobs, bin_size, nbins,
                                                            bin_edges(bin_size, nbins))
    assert not unsummed.any() and hist.sum() > 1000
    F = len(traj["steps"])
    volume = math.fsum((traj["L"][:, 0] * traj["L"][:, 1] * traj["L"][:, 2]).tolist()) / F
    sizes = np.diff(off)
    return [D.pair_columns(hist[j], sums[j], F, int(sizes[a]), int(sizes[b]), a == b, volume, bin_size)
            for j, (a, b) in enumerate(jobs)]


@pytest.mark.parametrize("stream", [True, False])
def test_orientational_correlation_end_to_end(B, water, stream, monkeypatch):
    """Dipole-dipole with O sites, ion-dipole with a vectorless ion, and an H-H vector at the centre of mass against the
    ion: every column is the restatement's bit for bit (the host formulas are the same expressions on the same
    integers), streamed in batches of four frames and loaded at once."""
    from mdproptools_amd.structural import orientational_correlation as M

    monkeypatch.setattr(M, "STREAM", stream)
    monkeypatch.setattr(M, "BATCH_BYTES", 4 * 126 * 24)
    frames = M.calc_orientational_correlation(5.0, 0.25, PAIRS, water["pattern"], D.NUM_MOLS, D.ATOMS_PER_MOL, mass=MASS,
                                              save=True, working_dir=str(water["dir"]))
    want = _expected_frames(water["traj"], 5.0, 0.25)
    assert len(frames) == 3
    for df, cols in zip(frames, want):
        assert list(df.columns) == list(cols) and len(df) == 20
        for name in cols:
            assert D.same_bits(df[name].to_numpy(), cols[name]), name
    assert np.nanmax(np.abs(frames[1]["<cos_r>"].to_numpy())) > 0 and not frames[1]["<cos>"].to_numpy()[frames[1]["g(r)"] > 0].any()
    import pandas as pd

    summary = pd.read_csv(str(water["dir"]) + "/orientational_correlation_pairs.csv")
    assert summary["pairs"].tolist() == [6 * 40 * 39, 6 * 6 * 40, 6 * 40 * 6] and summary["frames"].tolist() == [6, 6, 6]
    # unwrapped coordinates of the same frames: the sites differ by whole box edges and every coordinate is a multiple
    # of 1 / 1024, so the nearest images, and with them the pair counts, are the same
    unwrapped = M.calc_orientational_correlation(5.0, 0.25, PAIRS[:1], water["pattern"], D.NUM_MOLS, D.ATOMS_PER_MOL,
                                                 coords="unwrapped")
    assert np.array_equal(unwrapped[0]["g(r)"], frames[0]["g(r)"])


def test_orientational_correlation_refuses(B, water, tmp_path):
    from mdproptools_amd.structural.orientational_correlation import calc_orientational_correlation

    traj = dict(water["traj"])
    x = traj["x"].copy()
    x[1, :, 3 * 4] = x[1, :, 3 * 9]                                        # the O of molecule 5 on that of molecule 10, frame 1
    x[1, :, 3 * 4 + 1:3 * 4 + 3] += (x[1, :, 3 * 9] - traj["x"][1, :, 3 * 4])[:, None]
    traj["x"] = np.mod(x - traj["lo"][:, :, None], traj["L"][:, :, None]) + traj["lo"][:, :, None]
    traj["xu"], traj["img"] = traj["x"], np.zeros_like(traj["img"])
    pattern = D.write_dumps(tmp_path, traj, frames=range(3))
    with pytest.raises(ValueError, match=r"1:dipole@1 -- 1:dipole@1 \(2\)"):
        calc_orientational_correlation(5.0, 0.25, PAIRS[:2], pattern, D.NUM_MOLS, D.ATOMS_PER_MOL)
    x = water["traj"]["x"].copy()
    x[2, :, 3 * 7 + 2] = x[2, :, 3 * 7 + 1]                                # the two H of molecule 8 coincide in frame 2
    traj["x"] = x
    for f in tmp_path.glob("traj.*.dump"):
        f.unlink()
    pattern = D.write_dumps(tmp_path, traj, frames=range(3))
    with pytest.raises(ValueError, match=r"1:2-3@com \(1\)"):
        calc_orientational_correlation(5.0, 0.25, PAIRS, pattern, D.NUM_MOLS, D.ATOMS_PER_MOL, mass=MASS)


@pytest.mark.parametrize("integer", [True, False])
def test_dielectric_constant_end_to_end(B, tmp_path, integer, monkeypatch):
    """Against the restatement on the frames the dumps hold. The totals come from the kernel in the restatement's fixed
    order, and the host formulas are the same expressions: eps_r, its running value, <mu^2> and g_K are compared with ==
    — in the integer-valued configuration (whole-number coordinates, charges -2, 1, 1) every sum is exact whatever its
    order, in the other one the equality rests on that order. Phi goes through mdhip_xcorr's transform: within 1e-9 of
    the restatement's exactly summed lags (measured: printed below; its error is that of an FP64 FFT of 24 points)."""
    from mdproptools_amd.common import constants
    from mdproptools_amd.structural import dielectric as M

    traj = D.water_like(n_frames=24, integer=integer)
    pattern = D.write_dumps(tmp_path, traj)
    monkeypatch.setattr(M, "BATCH_BYTES", 7 * 126 * 24)
    res = M.calc_dielectric_constant(pattern, D.NUM_MOLS, D.ATOMS_PER_MOL, 298.0, dt=2, max_lag=8, save=True,
                                     working_dir=str(tmp_path))
    assert res["skipped"] == [2]                                          # the ions carry a net charge
    q = traj["q"][:3]
    got = D.mol_moments(traj["x"], traj["L"], [0], [40], [3], [[]], [[(1, q[1]), (2, q[2])]], [0])
    volume = traj["L"][:, 0] * traj["L"][:, 1] * traj["L"][:, 2]
    dip, dist = constants.DIPOLE_CONVERSION["real"], constants.DISTANCE_CONVERSION["real"]
    want = D.dielectric(got["total"], got["sq_total"], volume, [40], 298.0, dip, dist)
    if integer:
        assert np.array_equal(got["total"], np.rint(got["total"])) and np.abs(got["total"]).max() > 10
    print("eps_r", res["eps_r"], want["eps_r"])
    assert res["eps_r"] == want["eps_r"] and res["eps_r"] > 1.0
    conv = res["convergence"]
    assert D.same_bits(conv["eps_r"].to_numpy(), want["running"]) and conv["frames"].tolist() == list(range(1, 25))
    assert np.array_equal(conv["Time (ps)"].to_numpy(), (200 * np.arange(24)).astype(np.float64) * 2e-3)
    to_debye = dip / constants.DIPOLE_CONVERSION["electron"]
    types = res["types"]
    assert types["mol_type"].tolist() == [1] and types["N"].tolist() == [40]
    assert types["<mu^2> (D^2)"][0] == want["mu2"][0] * to_debye ** 2 and types["g_K"][0] == want["g_K"][0]
    v = got["vec"]
    norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).sum(axis=1)
    assert types["<|mu|> (D)"][0] == np.mean(norm) / 40 * to_debye
    phi = D.acf(want["M"], 8)
    err = np.abs(res["acf"]["Phi"].to_numpy() - phi).max()
    print("Phi: largest deviation", err)
    assert err <= 1e-9 and res["acf"]["Phi"][0] == 1.0
    # only the ions asked for: nothing to sum
    with pytest.raises(ValueError, match="net charge"):
        M.calc_dielectric_constant(pattern, D.NUM_MOLS, D.ATOMS_PER_MOL, 298.0, mol_types=[2])
