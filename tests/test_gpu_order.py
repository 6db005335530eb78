"""
backend.bond_order / calc_order_parameters and their kernels (csrc/bond_order.hip) on the GPU against the numpy
restatement (tests/order_ref.py): count, centres and flags with ==, the values to 1e-12 absolute with NaN in the same
places. The bound: |dq_l| <= sqrt(4 pi / (2l + 1)) * ||dq_lm|| <= sqrt(4 pi) * e_Y, with e_Y ~ 1e-14 the absolute
error of one Y_lm for l <= 12 (direction cosines of two ulps through the recurrence). The cases: lattices with closed
forms, randomised systems built to hit every edge (rsq == r_cut**2 exactly, d == +-L/2 exactly, neighbours across each
boundary, an atom on a centre, three neighbours under `tetrahedral`, neighbours on the poles, a per-frame box), and the
structural ones (centre counts around the tile width, candidate counts around the chunk, rows around `cap`, the limits,
device input, more than 65 535 frames, non-finite coordinates, repeated calls).
"""
import numpy as np
import pytest

import order_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-12
SEEN = {"dev": 0.0}  # the largest deviation from the restatement over the module (printed by every check)


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _same(got, want, what):
    """Values to TOL with NaN in the same places; records the largest deviation."""
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    dev = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    SEEN["dev"] = max(SEEN["dev"], dev)
    print("%s: largest deviation %.3e (module so far %.3e)" % (what, dev, SEEN["dev"]))
    assert dev <= TOL, (what, dev)


def _check(B, xyz, box, types, centre_type, neighbour_types, r_cut, xin=None, **kw):
    """backend.bond_order against the restatement; returns (the GPU's dict, the restatement's)."""
    cap = kw.pop("cap", 64)
    got = B.bond_order(xin if xin is not None else xyz, box, types, centre_type, neighbour_types, r_cut * r_cut, cap=cap,
                       **kw)
    want = R.bond_order(xyz, box, types, centre_type, neighbour_types, r_cut * r_cut, **kw)
    assert got["count"].dtype == np.int32 and got["flags"].dtype == np.int32
    assert np.array_equal(got["centres"], want["centres"])
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["flags"], want["flags"])
    for key in ("q", "qbar", "tet"):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            _same(got[key], want[key], key)
    return got, want


def _bytes(out):
    return b"".join(out[k].tobytes() for k in ("q", "qbar", "tet", "flags", "count") if out[k] is not None)


# ---- lattices ----

Q_SC = (np.sqrt(7.0 / 12.0), np.sqrt(2.0) / 4.0)
LATTICES = {"sc": (lambda: R.simple_cubic(4, 2.0), 2.5, 6, Q_SC),
            "fcc": (lambda: R.fcc(3, 2.0), 1.5, 12, (0.190940654, 0.574524260)),
            "bcc": (lambda: R.bcc(3, 2.0), 1.85, 8, (0.509175077, 0.628539361)),
            "diamond": (lambda: R.diamond(2, 4.0), 2.2, 4, (0.509175077, 0.628539361))}


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_lattice_backend_and_dropin(B, name, tmp_path):
    from mdproptools_amd.structural.order_parameters import calc_order_parameters

    make, r_cut, n_nb, (q4, q6) = LATTICES[name]
    xyz, box = make()
    n = xyz.shape[2]
    types = np.ones(n, dtype=np.int64)
    tetra = name == "diamond"
    got, want = _check(B, xyz, box, types, 1, [1], r_cut, degrees=(4, 6), tetrahedral=tetra)
    assert np.all(got["count"] == n_nb) and not got["flags"].any()
    assert np.abs(got["q"][..., 0] - q4).max() < 1e-9 and np.abs(got["q"][..., 1] - q6).max() < 1e-9
    if tetra:
        assert np.abs(got["tet"] - 1.0).max() < 1e-14
    pattern = R.write_dumps(xyz, box, types, str(tmp_path), stem="ord")
    out = tmp_path / "order.csv"
    dist, summary, values = calc_order_parameters(r_cut, 1, [1], pattern, tetrahedral=tetra, path_or_buff=str(out),
                                                  per_centre=True)
    names = ["q4", "q6"] + (["q_tet", "s_k"] if tetra else [])
    cols = ["value"] + [p + k for k in names for p in ("p_", "count_")]
    assert list(dist.columns) == cols and out.read_text().splitlines()[0] == ",".join(cols)
    assert np.array_equal(values["centres"], np.arange(n))
    _same(values["q4"], want["q"][..., 0], "drop-in q4")
    _same(values["q6"], want["q"][..., 1], "drop-in q6")
    assert list(summary["n_values"]) == [n] * len(names) and not summary["n_short"].any()
    lo, n_bins = (-3.0, 400) if tetra else (0.0, 100)
    assert len(dist) == n_bins and int(dist["count_q4"].to_numpy()[int(np.floor((q4 - lo) / 0.01))]) == n


def test_fcc_selection_and_average(B):
    xyz, box = R.fcc(3, 2.0)
    types = np.ones(108, dtype=np.int64)
    first, _ = _check(B, xyz, box, types, 1, [1], 1.5, degrees=(4, 6), averaged=True)
    assert np.abs(first["qbar"] - first["q"]).max() < TOL  # every site is the same: the average changes nothing
    # past the second shell (18 neighbours), the 12 nearest are the first shell, in the same atom order: the same bytes
    wide, _ = _check(B, xyz, box, types, 1, [1], 2.1, degrees=(4, 6), n_nearest=12, averaged=True)
    assert np.all(wide["count"] == 18) and not wide["flags"].any()
    assert wide["q"].tobytes() == first["q"].tobytes() and wide["qbar"].tobytes() == first["qbar"].tobytes()
    # 8 of 12 equidistant neighbours: the ties go by atom index
    eight, want = _check(B, xyz, box, types, 1, [1], 1.5, degrees=(4, 6), n_nearest=8, tetrahedral=True)
    assert np.all(eight["count"] == 12) and not eight["flags"].any()
    assert np.abs(eight["q"][..., 0] - 0.190940654).min() > 1e-3  # (not the whole shell)


# ---- randomised systems with the edge cases ----

def _edge_system(seed, n, n_frames=2):
    """Types 1 (centres), 2, 3 in turn; frame 0 carries the edges (r_cut 3.5, box 24 x 9 x 6); the box varies. The
    random atoms keep to x <= 16.5: what is placed around x = 20.25 has no other neighbours."""
    rng = np.random.default_rng(seed)
    box = np.array([[24.0, 9.0, 6.0], [24.5, 9.25, 6.5], [23.75, 9.5, 6.25]])[:n_frames]
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * np.array([16.5, 8.9, 5.9])[None, :, None], 3)
    types = np.arange(n) % 3 + 1
    c = lambda i: 3 * i        # noqa: E731  (the i-th centre)
    a = lambda i: 3 * i + 1    # noqa: E731  (the i-th atom of type 2)
    f = xyz[0]
    f[:, c(0)], f[:, a(0)] = [5.0, 5.0, 2.0], [8.5, 5.0, 2.0]          # exactly r_cut: left out
    f[:, c(1)], f[:, a(1)] = [4.0, 4.0, 1.0], [4.0, 4.5, 4.0]          # d_z == +L/2
    f[:, c(2)], f[:, a(2)] = [9.0, 4.0, 5.0], [9.5, 4.0, 2.0]          # d_z == -L/2
    f[:, c(3)] = [0.2, 0.3, 0.1]                                       # neighbours across each boundary
    f[:, a(3)], f[:, a(4)], f[:, a(5)] = [23.5, 0.3, 0.1], [0.2, 8.6, 0.1], [0.2, 0.3, 5.4]
    f[:, c(4)] = [6.0, 6.0, 3.0]                                       # neighbours exactly on the poles
    f[:, a(6)], f[:, a(7)] = [6.0, 6.0, 4.5], [6.0, 6.0, 1.5]
    f[:, a(11)] = f[:, c(5)]                                           # an atom on a centre: degenerate
    f[:, c(6)] = [20.25, 4.0, 3.0]                                     # three neighbours: short under tetrahedral
    f[:, a(12)], f[:, a(13)], f[:, a(14)] = [21.25, 4.0, 3.0], [20.25, 5.0, 3.0], [20.25, 4.0, 2.0]
    return xyz, box, types


@pytest.mark.parametrize("seed,n", [(1, 201), (2, 402), (3, 600)])
def test_random_systems_with_edges(B, seed, n):
    xyz, box, types = _edge_system(seed, n)
    got, want = _check(B, xyz, box, types, 1, [2], 3.5, degrees=(4, 6), tetrahedral=True)
    fl = want["flags"][0]
    assert fl[5] == R.Q_DEGENERATE | R.TET_DEGENERATE          # the atom on a centre
    assert want["count"][0, 6] == 3 and fl[6] == R.TET_SHORT    # three neighbours: q_l has a value, q_tet has none
    assert not np.isnan(got["q"][0, 6]).any() and np.isnan(got["tet"][0, 6]).all()
    d = xyz[0][:, 1] - xyz[0][:, 0]
    assert float((d ** 2).sum()) == 3.5 ** 2                    # the atom at exactly r_cut ...
    closer = xyz[:1].copy()
    closer[0, 0, 1] = 8.499
    near = R.bond_order(closer, box[:1], types, 1, [2], 3.5 * 3.5, degrees=())
    assert near["count"][0, 0] == want["count"][0, 0] + 1       # ... is out
    _check(B, xyz, box, types, 1, [2, 3], 3.5, degrees=(6,), n_nearest=6, tetrahedral=True)


# ---- structural cases ----

@pytest.mark.parametrize("n_centres", [1, 15, 16, 17, 33])
def test_centre_counts_around_the_tile(B, n_centres):
    rng = np.random.default_rng(n_centres)
    n = n_centres + 150
    xyz = np.round(rng.uniform(0, 1, (2, 3, n)) * np.array([9.0, 8.0, 7.0])[None, :, None], 3)
    types = np.where(np.arange(n) < n_centres, 1, 2)
    _check(B, xyz, np.tile([9.0, 8.0, 7.0], (2, 1)), types, 1, [2], 3.0, degrees=(4, 6), tetrahedral=True)


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
    got, _ = _check(B, xyz, np.full((1, 3), L), types, 1, [2], 3.5, degrees=(4, 6))
    assert 1 <= got["count"].max() <= 6 and not np.isnan(got["q"]).all()


def _ball(rng, centre, k, r):
    """k points within r of `centre`, 3 decimals."""
    p = rng.normal(size=(3, k))
    p = p / np.linalg.norm(p, axis=0) * (r * rng.uniform(0.2, 0.95, k))
    return np.round(np.asarray(centre)[:, None] + p, 3)


def test_rows_around_cap_and_the_rerun(B):
    """Centres with 0 .. 9 neighbours and cap = 8 (run again with cap = 9), 9 and 64: the same bytes."""
    rng = np.random.default_rng(8)
    sizes = [0, 1, 3, 4, 5, 7, 8, 9]
    spots = [[10.0 + 20.0 * i, 50.0, 50.0] for i in range(len(sizes))]
    cols = [np.array(spots).T] + [_ball(rng, s, k, 3.0) for s, k in zip(spots, sizes)]
    xyz = np.concatenate(cols, axis=1)[None]
    types = np.where(np.arange(xyz.shape[2]) < len(sizes), 1, 2)
    box = np.full((1, 3), 200.0)
    outs = []
    for cap in (8, 9, 64):
        got, want = _check(B, xyz, box, types, 1, [2], 3.5, degrees=(4, 6), tetrahedral=True, cap=cap)
        assert list(want["count"][0]) == sizes
        assert list(want["flags"][0]) == [R.Q_SHORT | R.TET_SHORT, R.TET_SHORT, R.TET_SHORT, 0, 0, 0, 0, 0]
        outs.append(_bytes(got))
    assert outs[0] == outs[1] == outs[2]
    sel = [_bytes(_check(B, xyz, box, types, 1, [2], 3.5, degrees=(4,), n_nearest=5, cap=cap)[0]) for cap in (8, 64)]
    assert sel[0] == sel[1]


def test_512_neighbours_pass_and_520_raise(B):
    rng = np.random.default_rng(513)
    xyz = np.concatenate([np.full((3, 1), 20.0), _ball(rng, [20.0] * 3, 520, 3.0)], axis=1)[None]
    types = np.where(np.arange(521) < 1, 1, 2)
    with pytest.raises(ValueError, match="frame 0, centre atom 0 has 520 neighbours"):
        B.bond_order(xyz, np.full((1, 3), 40.0), types, 1, [2], 3.5 ** 2)
    xyz, types = xyz[:, :, :513], types[:513]
    got, _ = _check(B, xyz, np.full((1, 3), 40.0), types, 1, [2], 3.5, degrees=(4, 6), tetrahedral=True)
    assert got["count"].max() == 512
    _check(B, xyz, np.full((1, 3), 40.0), types, 1, [2], 3.5, degrees=(6,), n_nearest=300)


def test_centres_among_their_neighbours_and_exclusion(B):
    rng = np.random.default_rng(88)
    n = 240
    xyz = np.round(rng.uniform(0, 1, (3, 3, n)) * np.array([10.0, 9.0, 6.0])[None, :, None], 3)
    xyz[1][:, 6] = xyz[1][:, 0]  # two centres on each other
    box = np.array([[10.0, 9.0, 6.0], [10.0, 9.5, 6.0], [10.5, 9.0, 6.25]])
    types = np.arange(n) % 2 + 1
    mol_of = np.arange(n) // 4
    for mol in (None, mol_of):
        got, want = _check(B, xyz, box, types, 1, [1], 3.0, degrees=(4, 6), averaged=True, tetrahedral=True, mol_of=mol)
        assert (want["flags"] & R.Q_DEGENERATE).any() and (want["flags"] == R.QBAR_SHORT).any()
        _check(B, xyz, box, types, 1, [1, 2], 3.0, degrees=(6,), n_nearest=12, mol_of=mol)
    _check(B, xyz, box, types, 1, [1], 3.0, degrees=(6,), n_nearest=10, averaged=True, mol_of=mol_of)


def test_four_degrees_at_once(B):
    xyz, box, types = _edge_system(5, 150)
    got, _ = _check(B, xyz, box, types, 1, [2, 3], 3.0, degrees=(1, 4, 6, 12), averaged=False, tetrahedral=True)
    one, _ = _check(B, xyz, box, types, 1, [2, 3], 3.0, degrees=(12,))
    assert got["q"][..., 3].tobytes() == one["q"][..., 0].tobytes()  # a degree does not depend on its company


def test_library_limits(B):
    import ctypes as C

    from mdproptools_amd._lib import MdhipError, default_context, ptr

    xyz, box = R.simple_cubic(2, 2.0)
    types = np.ones(8, dtype=np.int64)
    for bad in ((0,), (13,), (4, 6, 4)):
        with pytest.raises(MdhipError, match="l must be in|twice"):
            B.bond_order(xyz, box, types, 1, [1], 6.25, degrees=bad)
    with pytest.raises(MdhipError, match="n_degrees must be"):
        B.bond_order(xyz, box, types, 1, [1], 6.25, degrees=(1, 2, 3, 4, 5))
    with pytest.raises(MdhipError, match="nothing to compute"):
        B.bond_order(xyz, box, types, 1, [1], 6.25, degrees=())
    for cap in (0, 513):
        with pytest.raises(MdhipError, match="cap must be in"):
            B.bond_order(xyz, box, types, 1, [1], 6.25, cap=cap)
    with pytest.raises(MdhipError, match="candidates to be the centres"):
        B.bond_order(xyz, box, np.arange(8) % 2 + 1, 1, [2], 6.25, averaged=True)
    ctx = default_context()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    cen = i32(np.arange(8))
    x, bx = np.ascontiguousarray(xyz), np.ascontiguousarray(box)
    q, flags, count = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)

    def raw(xp, qp, fp, l=4, cap=64):
        deg = i32([l])
        return ctx.lib.mdhip_bond_order(ctx.h, 1, 8, xp, 0, ptr(bx), 8, ptr(cen, C.c_int32), 8, ptr(cen, C.c_int32), None,
                                        6.25, 1, ptr(deg, C.c_int32), 0, 0, 0, cap, qp, None, None, fp,
                                        ptr(count, C.c_int32))

    for args in ((None, ptr(q), ptr(flags, C.c_int32)), (C.c_void_p(x.ctypes.data), None, ptr(flags, C.c_int32)),
                 (C.c_void_p(x.ctypes.data), ptr(q), None)):
        rc = raw(*args)
        assert rc == -1
        with pytest.raises(MdhipError, match="NULL array"):
            ctx.check(rc)
    for kw, text in (({"l": 0}, "l must be in"), ({"l": 13}, "l must be in"), ({"cap": 0}, "cap must be in"),
                     ({"cap": 513}, "cap must be in")):
        rc = raw(C.c_void_p(x.ctypes.data), ptr(q), ptr(flags, C.c_int32), **kw)
        assert rc == -1
        with pytest.raises(MdhipError, match=text):
            ctx.check(rc)
    assert raw(C.c_void_p(x.ctypes.data), ptr(q), ptr(flags, C.c_int32)) == 0
    assert np.abs(q - Q_SC[0]).max() < 1e-12 and not flags.any()
    assert np.all(count == 3)  # (a cell of 2: +a and -a are one atom, three directions)
    # at the limits: cap 512, n_nearest 512 (more than any row holds: short)
    got, _ = _check(B, xyz, box, types, 1, [1], 2.5, degrees=(12,), cap=512)
    assert np.all(got["count"] == 3)
    got, _ = _check(B, xyz, box, types, 1, [1], 2.5, degrees=(4,), n_nearest=512)
    assert np.all(got["flags"] == R.Q_SHORT)


def test_device_input_and_repeated_calls(B):
    import torch

    xyz, box, types = _edge_system(4, 300, n_frames=3)
    kw = dict(degrees=(4, 6), tetrahedral=True)
    dev, _ = _check(B, xyz, box, types, 1, [2, 3], 3.5, cap=4, xin=torch.as_tensor(xyz, device="cuda"), **kw)  # re-run
    first = B.bond_order(xyz, box, types, 1, [2, 3], 3.5 * 3.5, **kw)
    second = B.bond_order(xyz, box, types, 1, [2, 3], 3.5 * 3.5, **kw)  # (the workspaces are zeroed again)
    assert _bytes(first) == _bytes(second) == _bytes(dev)
    same = np.where(np.arange(300) % 3 == 2, 2, 1)
    a = B.bond_order(xyz, box, same, 1, [1], 9.0, degrees=(6,), averaged=True, n_nearest=8)
    b = B.bond_order(torch.as_tensor(xyz, device="cuda"), box, same, 1, [1], 9.0, degrees=(6,), averaged=True,
                     n_nearest=8, cap=16)
    assert _bytes(a) == _bytes(b)


def test_more_than_65535_frames(B):
    """One centre with exactly four neighbours in every frame; the restatement's tetra() takes the frames at once."""
    rng = np.random.default_rng(9)
    F = 70001
    xyz = np.full((F, 3, 5), 2.5)
    xyz[:, :, 1:] += np.round(rng.uniform(-1.2, 1.2, (F, 3, 4)), 3)
    types = np.array([1, 2, 2, 2, 2])
    box = np.full((F, 3), 5.0)
    got = B.bond_order(xyz, box, types, 1, [2], 2.4 * 2.4, degrees=(), tetrahedral=True)
    assert np.all(got["count"] == 4) and got["q"].shape == (F, 1, 0)
    d = np.moveaxis(xyz[:, :, 1:] - xyz[:, :, :1], 1, 2)  # [F, 4, 3]; no wrap: |d| < L/2
    on_centre = ~d.any(axis=(1, 2))
    assert not on_centre.any() and not got["flags"].any()
    q_tet, s_k = R.tetra(d)
    _same(got["tet"], np.stack([q_tet, s_k], axis=1)[:, None, :], "70001 frames")
    few = R.bond_order(xyz[:20], box[:20], types, 1, [2], 2.4 * 2.4, degrees=(), tetrahedral=True)
    assert np.array_equal(few["tet"][:, 0, 0], q_tet[:20])  # (tetra() is what the restatement itself evaluates)
    assert np.abs(q_tet).max() <= 3.0 and q_tet.std() > 0.1


@pytest.mark.parametrize("case", ["neighbour_nan", "neighbour_pinf", "neighbour_ninf", "centre_nan"])
def test_non_finite_input(B, case):
    """A clean system of 60 atoms with one poisoned coordinate: the sweep's comparison leaves that atom out (a centre
    at NaN has no neighbours: short), nothing else changes, and the call returns."""
    rng = np.random.default_rng(60)
    xyz = np.round(rng.uniform(0, 1, (2, 3, 60)) * np.array([7.0, 6.0, 5.0])[None, :, None], 3)
    box = np.tile([7.0, 6.0, 5.0], (2, 1))
    types = np.arange(60) % 2 + 1
    clean = R.bond_order(xyz, box, types, 1, [2], 9.0, tetrahedral=True)
    atom, value = {"neighbour_nan": (7, np.nan), "neighbour_pinf": (7, np.inf), "neighbour_ninf": (7, -np.inf),
                   "centre_nan": (8, np.nan)}[case]
    xyz[0, 1, atom] = value
    got, want = _check(B, xyz, box, types, 1, [2], 3.0, degrees=(4, 6), tetrahedral=True)
    assert np.array_equal(want["count"][1], clean["count"][1])
    if case == "centre_nan":
        assert want["count"][0, 4] == 0 and want["flags"][0, 4] == R.Q_SHORT | R.TET_SHORT
        assert np.array_equal(np.delete(want["count"][0], 4), np.delete(clean["count"][0], 4))
    else:
        assert want["count"][0].sum() < clean["count"][0].sum()
    _check(B, xyz, box, np.ones(60, dtype=np.int64), 1, [1], 3.0, degrees=(6,), averaged=True, n_nearest=4)
