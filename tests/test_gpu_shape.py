"""
mdhip_mol_shape (csrc/mol_shape.hip) and structural/molecular_shape.py on the GPU, against the numpy restatement
(tests/shape_ref.py).

The header states every operation, so the histograms and counts are compared with `==` and the per-molecule values and
the totals bit for bit (reorientation_ref.same_bits). Shapes are the smallest at which the kernel can go wrong: either
side of a run's molecule limit (256) and atom limit (1024), molecules one atom longer than the stage (the walk form),
bond differences at the half edge, a chain several boxes long, frames beyond gridDim.y, non-finite input.
"""
import ctypes as C

import numpy as np
import pytest

import dihedral_ref as DR
import shape_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("hist_rg", "hist_ee", "hist_k", "beyond", "degenerate")


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(B, x, box, a0, mols, length, weights, ends=None, unwrap=1, per_mol=True, **bins):
    """Every output of one call against the restatement; -> (library's dict, restatement's dict)."""
    want = R.mol_shape(x, box, a0, mols, length, weights, ends=ends, unwrap=unwrap, **bins)
    got = B.mol_shape(x, box, a0, mols, length, weights, ends=ends, unwrap=unwrap, per_mol=per_mol, **bins)
    for key in KEYS:
        print(key, "mismatches", int((got[key] != want[key]).sum()))
    for key in KEYS:
        assert got[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), key
    bad = np.argwhere(~((got["totals"] == want["totals"]) | (np.isnan(got["totals"]) & np.isnan(want["totals"]))))
    print("totals mismatches", len(bad), bad[:5].tolist())
    assert R.same_bits(got["totals"], want["totals"])
    if per_mol:
        pm = np.asarray(got["per_mol"])
        bad = np.argwhere(~((pm == want["per_mol"]) | (np.isnan(pm) & np.isnan(want["per_mol"]))))
        print("per_mol mismatches", len(bad), bad[:5].tolist())
        assert R.same_bits(pm, want["per_mol"])
    else:
        assert got["per_mol"] is None
    n = np.asarray(mols, dtype=np.uint64) * np.uint64(np.shape(x)[0])
    assert np.array_equal(got["hist_rg"].sum(axis=1) + got["beyond"][:, 0], n)
    assert np.array_equal(got["hist_ee"].sum(axis=1) + got["beyond"][:, 1], n)
    assert np.array_equal(got["hist_k"].sum(axis=1) + got["degenerate"] + want["uncounted"], n)
    return got, want


def _molecules(rng, F, mols, per, L):
    """Wrapped coordinates [F,3,mols*per] of chains with bonds about 1 long placed anywhere in boxes L [F,3]."""
    centre = rng.random((F, 3, mols, 1)) * L[:, :, None, None]
    x = centre + np.cumsum(rng.normal(0.0, 0.6, size=(F, 3, mols, per)), axis=3)
    return np.ascontiguousarray(np.mod(x, L[:, :, None, None]).reshape(F, 3, mols * per))


@pytest.mark.parametrize("mols,per", [(255, 3), (256, 3), (257, 3), (64, 16), (65, 16), (1, 5)])
@pytest.mark.parametrize("F", [1, 2, 65])
def test_either_side_of_the_stage(B, mols, per, F):
    rng = np.random.default_rng(1000 * mols + 10 * per + F)
    L = 9.0 + rng.random((F, 3))                                    # the box varies per frame and axis
    x = _molecules(rng, F, mols, per, L)
    w = rng.uniform(1.0, 32.0, size=per)
    for unwrap in (1, 0):
        got, _ = _check(B, x, L, [0], [mols], [per], [w], unwrap=unwrap, per_mol=bool(unwrap), bin_size=0.05, n_bins=120)
        assert got["hist_rg"].sum() > 0 and not got["degenerate"].any()
    _check(B, x, None, [0], [mols], [per], [w], unwrap=1, per_mol=F != 2, bin_size=0.05, n_bins=120)
    if mols == 257 and F == 65:   # some bond difference must have been wrapped
        d = x[:, :, 1::3] - x[:, :, 0::3]
        assert (np.abs(d) > L[:, :, None] / 2).any()


def test_a_job_without_molecules_between_two_others_and_one_atom_molecules(B):
    rng = np.random.default_rng(6501)
    F = 5
    L = 9.0 + rng.random((F, 3))
    x = np.concatenate([_molecules(rng, F, 65, 4, L), _molecules(rng, F, 3, 7, L), _molecules(rng, F, 300, 1, L)], axis=2)
    a0, mols, length = [0, 260, 260, 281], [65, 0, 3, 300], [4, 4, 7, 1]
    w = [rng.uniform(1, 9, size=n) for n in length]
    got, _ = _check(B, x, L, a0, mols, length, w, ends=[(0, 3), (1, 2), (6, 0), (0, 0)], bin_size=0.1, n_bins=64)
    assert got["hist_rg"].sum(axis=1).tolist()[1] == 0 and got["degenerate"].tolist() == [0, 0, 0, 300 * F]
    assert not got["totals"][1].any() and not got["totals"][3].any()          # a one-atom molecule: zeros, counted
    assert got["hist_rg"][3, 0] == 300 * F and not got["hist_k"][3].any() and not np.asarray(got["per_mol"])[:, :, 68:].any()


def test_the_walk_form_alone_and_beside_a_short_type(B):
    """Two molecules of one atom more than the largest stage: one lane per (molecule, frame) in global memory; the
    restatement knows nothing of forms, so agreeing with it in both calls is agreeing with the staged form."""
    rng = np.random.default_rng(1025)
    F, n = 3, R.CAP + 1
    L = 30.0 + rng.random((F, 3))
    long_x = _molecules(rng, F, 2, n, L)
    short_x = _molecules(rng, F, 70, 6, L)
    w_long, w_short = rng.uniform(1.0, 20.0, size=n), rng.uniform(1.0, 20.0, size=6)
    for unwrap in (1, 0):
        alone, _ = _check(B, long_x, L, [0], [2], [n], [w_long], unwrap=unwrap, bin_size=0.25, n_bins=400)
        both, _ = _check(B, np.concatenate([short_x, long_x], axis=2), L, [0, 420], [70, 2], [6, n], [w_short, w_long],
                         unwrap=unwrap, bin_size=0.25, n_bins=400)
        assert np.array_equal(alone["hist_rg"][0], both["hist_rg"][1]) and R.same_bits(alone["totals"][0], both["totals"][1])
    # the same molecules cut down to the largest stage take the staged form
    _check(B, np.ascontiguousarray(long_x[:, :, : 2 * R.CAP]), L, [0], [2], [R.CAP], [w_long[:-1]], bin_size=0.25, n_bins=400)


def test_a_chain_across_the_box(B):
    """A straight 40-atom chain of spacing 1 in a box of edge 8, along each axis, and one with the steps (1, 1/2, 0): chain
    mode gives the rod exactly; mode 0 folds every atom next to the first one (along an axis the folded atoms still lie
    on a line; the oblique chain, whose x and y fold at different atoms, loses that too)."""
    xu = np.zeros((1, 3, 160))
    for ax in range(3):
        xu[0, ax, 40 * ax:40 * (ax + 1)] = np.arange(40) + 0.5
    xu[0, 0, 120:], xu[0, 1, 120:] = np.arange(40) + 0.5, np.arange(40) / 2 + 0.25
    x = np.mod(xu, 8.0)
    L = np.full((1, 3), 8.0)
    w = [np.ones(40)]
    got, _ = _check(B, x, L, [0], [4], [40], w, unwrap=1, bin_size=0.25, n_bins=200)
    pm = np.asarray(got["per_mol"])[0]
    rod = (40 * 40 - 1) / 12
    assert pm[0].tolist() == [rod] * 3 + [1.25 * rod] and pm[1].tolist() == [39.0 ** 2] * 3 + [1.25 * 39.0 ** 2]
    assert pm[2].tolist() == [1.0] * 4 and pm[3].tolist() == pm[0].tolist() and not pm[4:].any() and got["hist_k"][0, -1] == 4
    first, _ = _check(B, x, L, [0], [4], [40], w, unwrap=0, bin_size=0.25, n_bins=200)
    pm0 = np.asarray(first["per_mol"])[0]
    assert (pm0[0] < 16.0).all() and pm0[2, 3] < 0.9 and pm0[4, 3] > 0.1


def test_bond_differences_at_the_half_edge(B):
    """A bond difference just above, exactly at and just below +-L/2 on every axis, for each of the three bonds of a
    4-atom chain (the construction of test_gpu_dihedrals.py): the wrap is strict, in both modes."""
    F = 5
    L = np.array([[8.0, 10.0, 12.0]] * F) + np.arange(F)[:, None] * 0.5
    half = L / 2
    base = np.array([[1.0, 0.25, 0.0], [0.5, 1.0, 0.25], [0.25, -0.5, 1.0]])
    cases = []
    for bond in range(3):
        for ax in range(3):
            for sign in (1.0, -1.0):
                for pick in (lambda h: h, lambda h: np.nextafter(h, np.inf), lambda h: np.nextafter(h, 0.0)):
                    v = sign * pick(half[:, ax])
                    pts = np.concatenate([np.zeros((F, 1, 3)), np.cumsum(np.tile(base[None], (F, 1, 1)), axis=1)], axis=1)
                    col = np.zeros((F, 4))
                    col[:, bond + 1] = v
                    for k in range(bond - 1, -1, -1):
                        col[:, k] = col[:, k + 1] - 1.0
                    for k in range(bond + 2, 4):
                        col[:, k] = col[:, k - 1] - sign
                    pts[:, :, ax] = col
                    assert np.array_equal(col[:, bond + 1] - col[:, bond], v)
                    cases.append(pts)
    pts = np.stack(cases, axis=1)                                      # [F,M,4,3]
    M = pts.shape[1]
    x = np.ascontiguousarray(pts.transpose(0, 3, 1, 2).reshape(F, 3, 4 * M))
    w = [np.array([1.0, 2.0, 3.0, 4.0])]
    chain, _ = _check(B, x, L, [0], [M], [4], w, unwrap=1, bin_size=0.1, n_bins=100)
    first, _ = _check(B, x, L, [0], [M], [4], w, unwrap=0, bin_size=0.1, n_bins=100)
    open_, _ = _check(B, x, None, [0], [M], [4], w, unwrap=1, bin_size=0.1, n_bins=100)
    assert not R.same_bits(chain["per_mol"], open_["per_mol"]) and not R.same_bits(chain["per_mol"], first["per_mol"])


def test_the_exact_shapes_on_the_device(B):
    rod = [(k, 0, 0) for k in range(4)]
    diag = [(k, k, 0) for k in range(4)]
    square = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    cube = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    x = np.ascontiguousarray(np.array(rod + diag + square + cube, dtype=np.float64).T[None])
    got, _ = _check(B, x, None, [0, 12, 12], [3, 1, 0], [4, 8, 8], [np.ones(4), np.ones(8), np.ones(8)], bin_size=0.25,
                    n_bins=16, n_kbins=4)
    pm = np.asarray(got["per_mol"])[0]                                 # rows Rg2 Ree2 k2 l1 l2 l3
    assert pm[:, 0].tolist() == [1.25, 9.0, 1.0, 1.25, 0.0, 0.0]
    assert pm[:, 1].tolist() == [2.5, 18.0, 1.0, 2.5, 0.0, 0.0]
    assert pm[:, 2].tolist() == [0.5, 1.0, 0.25, 0.25, 0.25, 0.0]
    assert pm[:, 3].tolist() == [0.75, 3.0, 0.0, 0.25, 0.25, 0.25]
    assert got["hist_k"].tolist() == [[0, 1, 0, 2], [1, 0, 0, 0], [0, 0, 0, 0]]   # 0.25 opens bin 1, 1.0 is in the last bin
    assert np.flatnonzero(got["hist_rg"][0]).tolist() == sorted({int(np.sqrt(v) / 0.25) for v in (1.25, 2.5, 0.5)})
    assert got["hist_ee"][0, 12] == 1 and got["hist_ee"][0, 4] == 1 and got["beyond"].tolist() == [[0, 1], [0, 0], [0, 0]]
    # (the tree adds partial 2 to partial 0 before partial 1)
    assert got["totals"][0, :, 0].tolist() == [4.25, (np.sqrt(1.25) + np.sqrt(0.5)) + np.sqrt(2.5), 28.0, 4.0, 0.25, 0.0, 2.25,
                                               0.0625, 1.25 ** 2 + 2.5 ** 2 + 0.25]


def test_weights(B):
    rng = np.random.default_rng(4)
    F, mols = 4, 90
    L = np.full((F, 3), 12.0)
    x = _molecules(rng, F, mols, 6, L)
    heavy = np.array([1.008, 12.011, 15.999, 12.011, 32.06, 1.008])
    got, _ = _check(B, x, L, [0, 0, 0], [mols] * 3, [6] * 3, [heavy, np.ones(6), [0.0, 1, 1, 1, 1, 1]],
                    ends=[(0, 5), (5, 0), (1, 5)], bin_size=0.05, n_bins=160)
    assert not R.same_bits(got["totals"][0], got["totals"][1])
    assert R.same_bits(got["totals"][0, 2], got["totals"][1, 2])       # Ree2 knows no weights and no direction
    # a massless first atom: the shape of the other five, whatever the first one does
    y = x.copy()
    y[:, :, 0::6] = np.mod(y[:, :, 0::6] + 0.125, 12.0)
    moved, _ = _check(B, y, L, [0], [mols], [6], [[0.0, 1, 1, 1, 1, 1]], ends=[(1, 5)], unwrap=1, bin_size=0.05, n_bins=160)
    assert np.abs(moved["totals"][0, 0] - got["totals"][2, 0]).max() < 1e-9 * got["totals"][2, 0].max()


def test_non_finite_input(B):
    rng = np.random.default_rng(8)
    F, mols = 6, 300
    L = np.full((F, 3), 11.0)
    x = np.concatenate([_molecules(rng, F, mols, 5, L), _molecules(rng, F, 40, 3, L)], axis=2)
    a0, m, length = [0, 5 * mols], [mols, 40], [5, 3]
    w = [rng.uniform(1, 9, size=5), rng.uniform(1, 9, size=3)]
    base, _ = _check(B, x, L, a0, m, length, w, bin_size=0.05, n_bins=100)
    for value, frame, mol, atom, axis in ((np.nan, 2, 7, 3, 1), (np.inf, 4, 299, 0, 0), (1e300, 0, 256, 4, 2), (-np.inf, 5, 0, 2, 0)):
        y = x.copy()
        y[frame, axis, 5 * mol + atom] = value
        got, want = _check(B, y, L, a0, m, length, w, bin_size=0.05, n_bins=100)
        pm, pm0 = np.asarray(got["per_mol"]), np.asarray(base["per_mol"])
        other = np.ones(pm.shape, dtype=bool)
        other[frame, :, mol] = False
        assert R.same_bits(pm[other], pm0[other])                       # every other molecule and frame: no bit changed
        assert not np.isfinite(pm[frame, 0, mol])
        finite = np.isfinite(got["totals"])
        assert finite[1].all() and R.same_bits(got["totals"][1], base["totals"][1])
        assert not finite[0, 0, frame] and finite[0][:, np.arange(F) != frame].all()
        assert got["beyond"][0, 0] == base["beyond"][0, 0] + 1 and want["uncounted"].tolist() == [1, 0]
        assert (base["hist_rg"].astype(np.int64) - got["hist_rg"].astype(np.int64)).sum() == 1 and (base["hist_rg"] >= got["hist_rg"]).all()
        assert (base["hist_k"].astype(np.int64) - got["hist_k"].astype(np.int64)).sum() == 1 and (base["hist_k"] >= got["hist_k"]).all()
        assert np.array_equal(got["hist_rg"][1], base["hist_rg"][1]) and np.array_equal(got["hist_k"][1], base["hist_k"][1])
    y = x.copy()
    y[1, :, 5 * 3 + 1] = np.nan                                            # ... and with a box that is NaN in one frame
    Ln = L.copy()
    Ln[3, 1] = np.nan
    _check(B, y, Ln, a0, m, length, w, bin_size=0.05, n_bins=100)


@pytest.mark.parametrize("F", [65536, 2 * 65535 + 1])
def test_frames_past_the_launch_limit(B, F):
    """gridDim.y holds 65 535 frames: a workgroup strides over the rest. One 2-atom molecule on k/1024 coordinates: every
    value is exact, so frame f's Rg2 = (d/2)^2 with d the distance it was given."""
    k = np.arange(F, dtype=np.float64)
    x = np.zeros((F, 3, 2))
    x[:, 0, 0], x[:, 1, 0], x[:, 2, 0] = 1.0 + (k % 7) / 1024.0, 2.0, 3.0
    x[:, 0, 1] = x[:, 0, 0] + 1.0 + (k % 1021) / 1024.0
    x[:, 1, 1], x[:, 2, 1] = 2.0 + (k % 3) / 1024.0, 3.0
    got, _ = _check(B, x, None, [0], [1], [2], [np.ones(2)], bin_size=0.01, n_bins=150)
    d2 = (1.0 + (k % 1021) / 1024.0) ** 2 + ((k % 3) / 1024.0) ** 2
    pm = np.asarray(got["per_mol"])
    assert np.array_equal(pm[:, 1, 0], d2) and np.array_equal(pm[:, 0, 0], d2 / 4) and np.array_equal(got["totals"][0, 2], d2)
    assert got["hist_k"][0, -1] == F and got["hist_rg"].sum() == F


def test_invalid_arguments_leave_the_outputs_untouched(B):
    """Straight to the C entry point: MDHIP_EINVAL before anything is written."""
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    x = np.random.default_rng(0).normal(size=(4, 3, 12))
    good = dict(n_jobs=2, a0=[0, 4], mols=[1, 2], length=[4, 4], F=4, A=12, w_off=[0, 4, 8], w=[1.0] * 8, ends=[[0, 3], [3, 0]],
                unwrap=1, bin_size=0.1, nbins=8, n_kbins=4, edges=None)
    bad = [dict(n_jobs=0), dict(n_jobs=-1), dict(nbins=0), dict(nbins=4097), dict(n_kbins=0), dict(n_kbins=1025), dict(unwrap=2),
           dict(unwrap=-1), dict(bin_size=0.0), dict(bin_size=float("nan")), dict(bin_size=float("inf")), dict(ends=[[0, 4], [3, 0]]),
           dict(ends=[[0, 3], [-1, 0]]), dict(a0=[0, 5]), dict(mols=[1, 3]), dict(mols=[-1, 2]), dict(a0=[-1, 4]), dict(length=[4, 0]),
           dict(A=11), dict(F=0), dict(A=0), dict(w_off=[1, 5, 9]), dict(w_off=[0, 3, 8]), dict(w_off=[0, 4, 7]),
           dict(w=[1.0] * 4 + [0.0] * 4), dict(w=[1.0] * 4 + [2.0, -1.0, -1.0, 0.0]), dict(w=[1.0] * 7 + [float("inf")]),
           dict(w=[float("nan")] + [1.0] * 7), dict(edges=[0.1] + list(np.arange(1, 9) * 0.01)),
           dict(edges=[0.0, 0.02, 0.01] + list(np.arange(3, 9) * 0.01)),
           dict(null=("hist_rg", "hist_ee", "hist_k", "beyond", "degenerate", "totals", "per_mol")), dict(null=("x",)),
           dict(null=("a0",)), dict(null=("mols",)), dict(null=("length",)), dict(null=("w_off",)), dict(null=("w",)),
           dict(null=("ends",))]
    for change in bad:
        c = dict(good, **{k: v for k, v in change.items() if k != "null"})
        arrays = {"a0": np.array(c["a0"], dtype=np.int64), "mols": np.array(c["mols"], dtype=np.int64),
                  "length": np.array(c["length"], dtype=np.int32), "w_off": np.array(c["w_off"], dtype=np.int64),
                  "w": np.array(c["w"], dtype=np.float64), "ends": np.array(c["ends"], dtype=np.int32)}
        edges = None if c["edges"] is None else np.array(c["edges"], dtype=np.float64)
        outs = {"hist_rg": np.full((2, 4097), 77, dtype=np.uint64), "hist_ee": np.full((2, 4097), 77, dtype=np.uint64),
                "hist_k": np.full((2, 1025), 77, dtype=np.uint64), "beyond": np.full((2, 2), 77, dtype=np.uint64),
                "degenerate": np.full(2, 77, dtype=np.uint64), "totals": np.full((2, 9, 4), 77.0), "per_mol": np.full((4, 6, 3), 77.0)}
        args = {"x": vp(x), "a0": ptr(arrays["a0"], C.c_int64), "mols": ptr(arrays["mols"], C.c_int64),
                "length": ptr(arrays["length"], C.c_int32), "w_off": ptr(arrays["w_off"], C.c_int64), "w": ptr(arrays["w"]),
                "ends": ptr(arrays["ends"], C.c_int32)}
        args.update({k: ptr(v, C.c_uint64) for k, v in outs.items() if v.dtype == np.uint64})
        args.update(totals=ptr(outs["totals"]), per_mol=vp(outs["per_mol"]))
        for name in change.get("null", ()):
            args[name] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_mol_shape(
                ctx.h, c["F"], c["A"], args["x"], 0, None, c["n_jobs"], args["a0"], args["mols"], args["length"], args["w_off"],
                args["w"], args["ends"], c["unwrap"], c["bin_size"], c["nbins"], None if edges is None else ptr(edges),
                c["n_kbins"], args["hist_rg"], args["hist_ee"], args["hist_k"], args["beyond"], args["degenerate"],
                args["totals"], args["per_mol"], 0))
        assert err.value.code == -1, change
        assert all((v == 77).all() for v in outs.values()), change
    # ... and the arguments these were derived from are fine, with single outputs as well
    w = [np.ones(4), np.ones(4)]
    got, _ = _check(B, x, None, good["a0"], good["mols"], good["length"], w, ends=good["ends"], bin_size=0.1, n_bins=8, n_kbins=4)
    assert got["hist_k"].sum() == 12
    from mdproptools_amd._lib import ptr as p

    a0, mols, length = (np.array(good[k], dtype=t) for k, t in (("a0", np.int64), ("mols", np.int64), ("length", np.int32)))
    w_off, wt, ends = np.array(good["w_off"], dtype=np.int64), np.ones(8), np.array(good["ends"], dtype=np.int32)
    only = np.zeros((2, 4), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_mol_shape(ctx.h, 4, 12, vp(x), 0, None, 2, p(a0, C.c_int64), p(mols, C.c_int64), p(length, C.c_int32),
                                      p(w_off, C.c_int64), p(wt), p(ends, C.c_int32), 1, 0.1, 8, None, 4, None, None,
                                      p(only, C.c_uint64), None, None, None, None, 0))
    assert np.array_equal(only, got["hist_k"])


def test_device_tensors_in_and_out(B):
    import torch

    rng = np.random.default_rng(21)
    F, mols = 7, 130
    L = 10.0 + rng.random((F, 3))
    x = _molecules(rng, F, mols, 9, L)
    w = [rng.uniform(1, 20, size=9)]
    got, _ = _check(B, x, L, [0], [mols], [9], w, bin_size=0.05, n_bins=200)
    dev = torch.device("cuda", B.default_context().device)
    out = torch.full((F, 6, mols), 7.0, dtype=torch.float64, device=dev)
    again = B.mol_shape(torch.as_tensor(x, device=dev), L, [0], [mols], [9], w, bin_size=0.05, n_bins=200, out=out, totals=False)
    assert again["per_mol"] is out and out.cpu().numpy().tobytes() == np.asarray(got["per_mol"]).tobytes()
    assert again["totals"] is None and all(np.array_equal(again[k], got[k]) for k in KEYS)


# ---- end to end ------------------------------------------------------------------------------------------------------------

FILE_ORDER = [7, 3] + [f for f in range(40) if f not in (3, 7)]       # the timestep column is out of order
MASS = [12.011, 15.999]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("shape")
    traj = DR.synthetic_trajectory()
    return {"dir": d, "pattern": DR.write_dumps(d, traj, file_order=FILE_ORDER), "traj": traj}


@pytest.mark.parametrize("stream", [True, False])
@pytest.mark.parametrize("coords", ["wrapped", "unwrapped"])
def test_end_to_end(B, dumps, stream, coords):
    from mdproptools_amd.structural import molecular_shape as M

    traj = dumps["traj"]
    # molecules are cut by faces: the wrapped coordinates of some bond differ by more than half an edge
    assert (np.abs(traj["x"][:, :, 1:280:4] - traj["x"][:, :, 0:280:4]) > traj["L"][:, :, None] / 2).any()
    a0, mols, length = [0, 280], DR.NUM_MOLS, DR.ATOMS_PER_MOL
    w = [np.full(4, MASS[0]), np.full(6, MASS[1])]
    ends = [(0, 3), (1, 4)]
    wrapped = coords == "wrapped"
    want = R.mol_shape(traj["x"] if wrapped else traj["xu"], traj["L"] if wrapped else None, a0, mols, length, w, ends=ends,
                       unwrap=1, bin_size=0.1, n_bins=60, n_kbins=20)
    tables = M.tables(["chain4", "chain6"], mols, traj["steps"], want["hist_rg"], want["hist_ee"], want["hist_k"],
                      want["beyond"], want["degenerate"], want["totals"], 0.1)
    got = M.calc_molecular_shape(dumps["pattern"], DR.NUM_MOLS, DR.ATOMS_PER_MOL, MASS, mol_names=["chain4", "chain6"],
                                 bin_size=0.1, r_max=6.0, ends=[(1, 4), (2, 5)], kappa_bins=20, coords=coords,
                                 per_molecule=True, save=stream, working_dir=str(dumps["dir"]), stream=stream,
                                 batch_bytes=7 * 334 * 24)                # seven frames per streamed batch: six batches
    for name in M.TABLES:
        assert list(got[name].columns) == list(tables[name].columns), name
        for col in tables[name].columns:
            a, b = got[name][col].to_numpy(), tables[name][col].to_numpy()
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (name, col)
    assert [v.shape for v in got["per_molecule"]] == [(40, 6, 70), (40, 6, 9)]
    assert R.same_bits(np.concatenate(got["per_molecule"], axis=2), want["per_mol"])
    if stream:
        import pandas as pd

        back = pd.read_csv(str(dumps["dir"] / "shape_summary.csv"), index_col=0)
        assert back["molecule"].tolist() == ["chain4", "chain6"] and np.allclose(back["<Rg>"], got["summary"]["<Rg>"], rtol=1e-12)
    # one type, mode "first": without a box the two modes differ by rounding alone
    one = M.calc_molecular_shape(dumps["pattern"], DR.NUM_MOLS, DR.ATOMS_PER_MOL, MASS, mol_types=[2], unwrap="first",
                                 coords=coords, r_max=6.0, bin_size=0.1, stream=stream)
    assert list(one["summary"]["molecule"]) == ["mol2"] and "per_molecule" not in one and len(one["frames"]) == 40
    if not wrapped:
        assert abs(one["summary"]["<Rg>"][0] - got["summary"]["<Rg>"][1]) < 1e-9
