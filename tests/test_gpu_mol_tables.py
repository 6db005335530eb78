"""
The device tables of the per-molecule job calls and of mdhip_free_volume (csrc/call_tables.h behind mdhip_axis_vectors,
mdhip_mol_moments, mdhip_dihedral_angles, mdhip_mol_shape and mdhip_free_volume) on the GPU, at the smallest shapes at
which an offset into a call's table can go wrong: an odd number of 4-byte entries in front of 8-byte ones, empty and
absent segments, the counters that stand last in a table. Every result is compared with the family's numpy restatement
as the family's own tests compare it: bit for bit (same_bits) or with ==. Every case checks the degenerate counters,
and `beyond` where the call has one.

RUNS lists the calls (label, function of the backend -> dict of arrays): the tests go through it, and so can a
comparison of two builds of the library.
"""
import ctypes as C

import numpy as np
import pytest

import dihedral_ref as DH
import dipole_ref as D
import free_volume_ref as FV
import reorientation_ref as R
import shape_ref as SH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _chains(rng, F, mols, per, L):
    """Wrapped coordinates [F,3,mols*per] of chains with bonds about 1 long placed anywhere in boxes L [F,3]."""
    centre = rng.random((F, 3, mols, 1)) * L[:, :, None, None]
    x = centre + np.cumsum(rng.normal(0.0, 0.6, size=(F, 3, mols, per)), axis=3)
    return np.ascontiguousarray(np.mod(x, L[:, :, None, None]).reshape(F, 3, mols * per))


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


# ---- the jobs of the tile calls: 5, 0 and 2 molecules of 4 atoms, three frames --------------------------------------------

A0, MOLS, LEN = [0, 20, 20], [5, 0, 2], [4, 4, 4]
TERMS = [[(1, -1.0)], [(1, 0.5), (2, 0.25), (3, -1.0)], [(3, 1.0)]]        # 1 + 3 + 1: five 4-byte atoms, then the counters


def _tile_input():
    rng = np.random.default_rng(20261021)
    L = 9.0 + rng.random((3, 3))
    x = _chains(rng, 3, 7, 4, L)
    x[2, :, 4 * 3 + 1] = x[2, :, 4 * 3]          # job 0, molecule 3, frame 2: atom 1 on atom 0
    x[1, :, 20 + 3] = x[1, :, 20]                # job 2, molecule 0, frame 1: atom 3 on atom 0 (the LAST counter)
    return x, L


def run_axis(B):
    x, L = _tile_input()
    U, deg = B.axis_vectors(x, L, A0, MOLS, LEN, TERMS)
    return {"U": U, "degenerate": deg}


def test_axis_vectors_odd_term_table(B):
    x, L = _tile_input()
    want, want_deg = R.axis_vectors(x, L, A0, MOLS, LEN, TERMS)
    got = run_axis(B)
    assert got["U"].shape == want.shape == (7, 3, 3) and R.same_bits(got["U"], want)
    assert got["degenerate"].tolist() == want_deg.tolist() == [1, 0, 1]


# moments: a fourth job with neither site nor vector terms; `null_site`: no job has a site term and the site arrays are NULL
MM_A0, MM_MOLS, MM_LEN, MM_UNIT = A0 + [0], MOLS + [5], LEN + [4], [1, 1, 1, 1]
MM_SITE = [[(1, 0.25)], [(1, 1.0), (2, 0.5), (3, 0.25)], [(2, 1.0)], []]
MM_VEC = TERMS + [[]]


def _moments(B, null_site, want_site, want_vec, totals):
    from mdproptools_amd._lib import default_context, ptr

    x, L = _tile_input()
    if not null_site:  # 5 + 5 terms
        return B.mol_moments(x, L, MM_A0, MM_MOLS, MM_LEN, MM_SITE, MM_VEC, MM_UNIT, want_site=want_site, want_vec=want_vec,
                             totals=totals)
    # 0 + 5 terms, straight to the entry point: site_atom and site_w are NULL
    ctx = default_context()
    J, F, S = 4, 3, sum(MM_MOLS)
    a0, mols, length = np.array(MM_A0, dtype=np.int64), np.array(MM_MOLS, dtype=np.int64), np.array(MM_LEN, dtype=np.int32)
    s_off, unit = np.zeros(J + 1, dtype=np.int64), np.array(MM_UNIT, dtype=np.int32)
    v_off = np.array([0, 1, 4, 5, 5], dtype=np.int64)
    v_atom = np.array([k for t in MM_VEC for k, _ in t], dtype=np.int32)
    v_w = np.array([w for t in MM_VEC for _, w in t])
    site, vec = (np.full((F, 3, S), 77.0) if want else None for want in (want_site, want_vec))
    total, sq_total = (np.full((J, 3, F), 77.0), np.full((J, F), 77.0)) if totals else (None, None)
    deg = np.full(J, 77, dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_mol_moments(
        ctx.h, F, x.shape[2], _vp(x), 0, ptr(L), J, ptr(a0, C.c_int64), ptr(mols, C.c_int64), ptr(length, C.c_int32),
        ptr(s_off, C.c_int64), None, None, ptr(v_off, C.c_int64), ptr(v_atom, C.c_int32), ptr(v_w), ptr(unit, C.c_int32),
        _vp(site), _vp(vec), 0, None if total is None else ptr(total), None if sq_total is None else ptr(sq_total),
        ptr(deg, C.c_uint64)))
    return {"site": site, "vec": vec, "degenerate": deg, "total": total, "sq_total": sq_total}


MM_CASES = [(null_site, want_site, want_vec, totals) for null_site in (False, True)
            for want_site, want_vec, totals in ((True, True, True), (True, True, False), (False, True, True),
                                                (True, False, True), (False, False, True), (True, False, False))]


@pytest.mark.parametrize("null_site,want_site,want_vec,totals", MM_CASES)
def test_moments_tables_and_output_slots(B, null_site, want_site, want_vec, totals):
    x, L = _tile_input()
    want = D.mol_moments(x, L, MM_A0, MM_MOLS, MM_LEN, [[]] * 4 if null_site else MM_SITE, MM_VEC, MM_UNIT)
    got = _moments(B, null_site, want_site, want_vec, totals)
    for name, asked in (("site", want_site), ("vec", want_vec), ("total", totals), ("sq_total", totals)):
        if asked:
            assert got[name].shape == want[name].shape and D.same_bits(got[name], want[name]), name
        else:
            assert got[name] is None, name
    assert got["degenerate"].tolist() == want["degenerate"].tolist() == [1, 0, 1, 0]


# dihedrals: the same jobs and a fourth over the molecules of the first, which joins its class: 3 classes, 4 jobs
DH_A0, DH_MOLS, DH_LEN = A0 + [0], MOLS + [5], LEN + [4]
DH_QUADS, DH_ROWS = [(0, 1, 2, 3), (0, 1, 2, 3), (3, 0, 1, 2), (3, 2, 0, 1)], [0, 1, 1, 0]


def _dihedrals(B, n_bins, want_series):
    x, L = _tile_input()
    hist, U, deg = B.dihedral_angles(x, L, DH_A0, DH_MOLS, DH_LEN, DH_QUADS, job_row=DH_ROWS if n_bins else None, n_bins=n_bins,
                                     want_series=want_series)
    return {"hist": hist, "U": U, "degenerate": deg}


@pytest.mark.parametrize("n_bins,want_series", [(10, False), (None, True), (10, True)], ids=["hist", "series", "both"])
def test_dihedrals_with_and_without_the_edge_table(B, n_bins, want_series):
    x, L = _tile_input()
    w_hist, w_U, w_deg = DH.dihedral_angles(x, L, DH_A0, DH_MOLS, DH_LEN, DH_QUADS, job_row=DH_ROWS, n_bins=10)
    got = _dihedrals(B, n_bins, want_series)
    if n_bins:
        assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], w_hist)
        assert int(got["hist"].sum()) + int(w_deg.sum()) == 12 * 3
    else:
        assert got["hist"] is None
    if want_series:
        assert got["U"].shape == w_U.shape == (12, 3, 3) and R.same_bits(got["U"], w_U)
    else:
        assert got["U"] is None
    # molecule 3 of the first type at frame 2 (jobs 0 and 3) and molecule 0 of job 2 at frame 1 have two atoms in one place
    assert got["degenerate"].tolist() == w_deg.tolist() == [1, 0, 1, 1]


# ---- shape ------------------------------------------------------------------------------------------------------------

SH_BINS = dict(bin_size=0.05, n_bins=16, n_kbins=7)      # Rg and Ree up to 0.8: most values have no bin


def _shape_input(which):
    """-> x, box, a0, mols, length, weights: the staged jobs (5, 0 and 2 molecules of 4 atoms), a walk job (2 molecules of
    1025 atoms), or both in one call; two frames for the walk job, else three."""
    rng = np.random.default_rng(1025)
    F = 3 if which == "staged" else 2
    L = 30.0 + rng.random((F, 3))
    parts, a0, mols, length = [], [], [], []
    if which != "walk":
        short = _chains(rng, F, 7, 4, L)
        short[1, :, 20:24] = short[1, :, 20:21]      # every atom of molecule 0 of the third job in one place: Rg == 0
        parts.append(short)
        a0, mols, length = list(A0), list(MOLS), list(LEN)
    if which != "staged":
        a0.append(sum(p.shape[2] for p in parts)), mols.append(2), length.append(SH.CAP + 1)
        parts.append(_chains(rng, F, 2, SH.CAP + 1, L))
    weights = [rng.uniform(1.0, 20.0, size=n) for n in length]
    return np.ascontiguousarray(np.concatenate(parts, axis=2)), L, a0, mols, length, weights


def _shape(B, which, want_totals=True, want_per_mol=True, want_hist=True):
    """All outputs through the backend; else straight to the entry point with the others NULL."""
    from mdproptools_amd._lib import default_context, ptr

    x, L, a0, mols, length, weights = _shape_input(which)
    if want_totals and want_per_mol and want_hist:
        return B.mol_shape(x, L, a0, mols, length, weights, per_mol=True, **SH_BINS)
    ctx = default_context()
    J, F, S, nb, nk = len(mols), x.shape[0], sum(mols), SH_BINS["n_bins"], SH_BINS["n_kbins"]
    a0_, mols_, len_ = np.array(a0, dtype=np.int64), np.array(mols, dtype=np.int64), np.array(length, dtype=np.int32)
    w_off = np.concatenate(([0], np.cumsum(length))).astype(np.int64)
    w = np.concatenate(weights)
    ends = np.array([(0, n - 1) for n in length], dtype=np.int32)
    u64 = lambda *shape: np.full(shape, 77, dtype=np.uint64) if want_hist else None  # noqa: E731
    out = {"hist_rg": u64(J, nb), "hist_ee": u64(J, nb), "hist_k": u64(J, nk), "beyond": u64(J, 2), "degenerate": u64(J),
           "totals": np.full((J, 9, F), 77.0) if want_totals else None, "per_mol": np.full((F, 6, S), 77.0) if want_per_mol else None}
    p64 = lambda a: None if a is None else ptr(a, C.c_uint64)  # noqa: E731
    ctx.check(ctx.lib.mdhip_mol_shape(
        ctx.h, F, x.shape[2], _vp(x), 0, ptr(L), J, ptr(a0_, C.c_int64), ptr(mols_, C.c_int64), ptr(len_, C.c_int32),
        ptr(w_off, C.c_int64), ptr(w), ptr(ends, C.c_int32), 1, SH_BINS["bin_size"], nb, None, nk, p64(out["hist_rg"]),
        p64(out["hist_ee"]), p64(out["hist_k"]), p64(out["beyond"]), p64(out["degenerate"]),
        None if out["totals"] is None else ptr(out["totals"]), _vp(out["per_mol"]), 0))
    return out


@pytest.fixture(scope="module")
def shape_want():
    return {which: SH.mol_shape(*_shape_input(which), unwrap=1, **SH_BINS) for which in ("staged", "walk", "both")}


def _check_shape(got, want, want_totals=True, want_per_mol=True, want_hist=True):
    for key in ("hist_rg", "hist_ee", "hist_k", "beyond", "degenerate"):
        if want_hist:
            assert got[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), key
        else:
            assert got[key] is None
    for key, asked in (("totals", want_totals), ("per_mol", want_per_mol)):
        if asked:
            assert got[key].shape == want[key].shape and SH.same_bits(np.asarray(got[key]), want[key]), key
        else:
            assert got[key] is None


@pytest.mark.parametrize("which", ["staged", "walk", "both"])
def test_shape_run_tables(B, shape_want, which):
    got, want = _shape(B, which), shape_want[which]
    _check_shape(got, want)
    n = np.asarray(_shape_input(which)[3], dtype=np.uint64) * np.uint64(want["totals"].shape[2])
    assert got["beyond"].sum() > 0 and np.array_equal(got["hist_rg"].sum(axis=1) + got["beyond"][:, 0], n)
    assert got["degenerate"].tolist() == {"staged": [0, 0, 1], "walk": [0], "both": [0, 0, 1, 0]}[which]


@pytest.mark.parametrize("alone", ["totals", "per_mol", "hist"])
def test_shape_one_output_alone(B, shape_want, alone):
    asked = dict(want_totals=alone == "totals", want_per_mol=alone == "per_mol", want_hist=alone == "hist")
    got = _shape(B, "both", **asked)
    _check_shape(got, shape_want["both"], **asked)
    if alone == "hist":
        assert got["beyond"].sum() > 0 and got["degenerate"].tolist() == [0, 0, 1, 0]


# ---- free volume ------------------------------------------------------------------------------------------------------

FV_EDGES = np.arange(41) * 0.0625      # 40 bins up to 2.5
FV_RADII = np.array([0.5, 1.0, 1.5])


def _free_volume_input(n_classes):
    rng = np.random.default_rng(7)
    L = 9.0 + rng.random((2, 3))
    x = np.ascontiguousarray((rng.random((2, 3, 7)) * 3.0 - 1.0) * L[:, :, None])      # seven atoms: 28 bytes of classes
    cls = (np.arange(7) % n_classes).astype(np.int32)
    return x, L, cls, FV_RADII[:n_classes]


def _free_volume(B, n_classes, n_probes):
    x, L, cls, radii = _free_volume_input(n_classes)
    return B.free_volume(x, L, cls, radii, (4, 4, 4), 3.0, FV_EDGES, (0.0, 0.5)[:n_probes], want_map=True, field=True)


@pytest.mark.parametrize("n_probes", [1, 2])
@pytest.mark.parametrize("n_classes", [1, 3])
def test_free_volume_odd_class_table(B, n_classes, n_probes):
    x, L, cls, radii = _free_volume_input(n_classes)
    want = FV.free_volume(x, L, cls, radii, (4, 4, 4), 3.0, FV_EDGES, (0.0, 0.5)[:n_probes])
    got = _free_volume(B, n_classes, n_probes)
    assert FV.same_bits(got["s"], want["s"])
    assert got["nearest"].dtype == np.int32 and np.array_equal(got["nearest"], want["nearest"])
    for key, dtype in (("hist", np.uint64), ("occupied", np.uint64), ("n_free", np.int64), ("free_map", np.uint32)):
        assert got[key].dtype == dtype and np.array_equal(got[key], want[key]), key
    assert got["n_free"].shape == (2, n_probes) and got["hist"].shape == (n_classes, 40)
    assert got["beyond"] == want["beyond"] and got["beyond"] > 0
    assert int(got["hist"].sum()) + int(got["occupied"].sum()) + got["beyond"] == 2 * 64


RUNS = ([("axis vectors", run_axis)]
        + [("moments null_site=%d site=%d vec=%d totals=%d" % c, lambda B, c=c: _moments(B, *c)) for c in MM_CASES]
        + [("dihedrals n_bins=%s series=%d" % c, lambda B, c=c: _dihedrals(B, *c)) for c in ((10, False), (None, True), (10, True))]
        + [("shape " + w, lambda B, w=w: _shape(B, w)) for w in ("staged", "walk", "both")]
        + [("shape both, %s alone" % a, lambda B, a=a: _shape(B, "both", a == "totals", a == "per_mol", a == "hist"))
           for a in ("totals", "per_mol", "hist")]
        + [("free volume classes=%d probes=%d" % c, lambda B, c=c: _free_volume(B, *c)) for c in ((1, 1), (1, 2), (3, 1), (3, 2))])
