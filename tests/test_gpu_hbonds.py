"""
backend.hbond_counts / backend.hbond_lifetime, the two public functions of structural/hydrogen_bonds.py and their
kernels (csrc/hbonds.hip, csrc/presence_table.h) on the GPU: every integer compared with == against the numpy
restatement (tests/hbonds_ref.py) — a randomised system built to hit every geometric edge, the structural cases
(donor counts around the tile width, acceptor counts around the chunk, mixed CSR rows, no histogram, device input,
more than 65 535 frames, repeated calls), scripted bond patterns for the lifetime (word boundaries, the forced
re-sweep, the frame limit), non-finite coordinates and the drop-in functions on dumps.
"""
import numpy as np
import pytest

import hbonds_ref as R

pytestmark = pytest.mark.gpu

R_DA, R_HA = 3.5, 2.6
COS150 = float(np.cos(np.radians(150.0)))


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check_counts(B, xyz, box, top, cos_cut=COS150, r_ha=None, mol_of=None, bin_size=1.0, xin=None, r_da=R_DA):
    """backend.hbond_counts against the restatement; returns the restatement's results."""
    edges = None if bin_size is None else B.angle_cos_edges(bin_size)
    r_ha_sq = 0.0 if r_ha is None else r_ha ** 2
    args = (top["donors"], top["don_class"], top["h_off"], top["h_atoms"], top["acceptors"], top["acc_class"],
            r_da ** 2, cos_cut)
    got = B.hbond_counts(xin if xin is not None else xyz, box, *args, r_ha_sq=r_ha_sq, cos_edges=edges, mol_of=mol_of,
                         n_dc=top["n_dc"], n_ac=top["n_ac"])
    want = R.hbond_counts(xyz, box, *args, r_ha_sq=r_ha_sq, edges=edges, mol_of=mol_of, n_dc=top["n_dc"],
                          n_ac=top["n_ac"])
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint64
    assert got[3].dtype == np.uint64
    for g, w, name in zip(got[:4], want[:4], ("n_bonds", "n_donated", "n_accepted", "angle_hist")):
        assert g.shape == w.shape, name
        assert np.array_equal(g.astype(np.int64), w), name
    assert got[4] == want[4]
    return want


# ---- one randomised system with the geometric edges ----

def _top(donors, don_class, hydrogens, acceptors, acc_class, n_dc=None, n_ac=None):
    """hydrogens: one list of atoms per donor."""
    h_off = np.concatenate([[0], np.cumsum([len(h) for h in hydrogens])]).astype(np.int32)
    h_atoms = np.array([a for h in hydrogens for a in h], dtype=np.int32)
    don_class, acc_class = np.asarray(don_class, dtype=np.int32), np.asarray(acc_class, dtype=np.int32)
    return {"donors": np.asarray(donors, dtype=np.int32), "don_class": don_class, "h_off": h_off, "h_atoms": h_atoms,
            "acceptors": np.asarray(acceptors, dtype=np.int32), "acc_class": acc_class,
            "n_dc": int(don_class.max()) + 1 if n_dc is None else n_dc,
            "n_ac": int(acc_class.max()) + 1 if n_ac is None else n_ac}


def _edge_system(seed=1, n_mol=60, n_frames=3):
    """Molecules of six atoms: O (donor class 0 AND acceptor class 0) with two hydrogens, N (donor class 1) with one,
    X (acceptor class 1). Hydrogens sit 0.95 from their donor and are wrapped into the box on their own. Frame 0
    carries the edges (r_da 3.5, box 12 x 9 x 6); the box varies from frame to frame."""
    rng = np.random.default_rng(seed)
    box = np.array([[12.0, 9.0, 6.0], [12.5, 9.25, 6.5], [11.75, 9.5, 6.25]])[:n_frames]
    n = 6 * n_mol
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * np.array([11.5, 8.9, 5.9])[None, :, None], 3)
    O, N, X = (lambda m: 6 * m), (lambda m: 6 * m + 3), (lambda m: 6 * m + 5)  # noqa: E731
    for m in range(n_mol):
        for d, hs in ((O(m), (1, 2)), (N(m), (1,))):
            for k in hs:
                u = rng.normal(size=(n_frames, 3))
                u *= 0.95 / np.linalg.norm(u, axis=1)[:, None]
                xyz[:, :, d + k] = np.round(np.mod(xyz[:, :, d] + u, box), 3)
    f = xyz[0]
    f[:, O(0)], f[:, O(0) + 1], f[:, X(1)] = [5.0, 5.0, 2.0], [6.0, 5.0, 2.0], [8.5, 5.0, 2.0]     # exactly r_da: out
    f[:, O(2)], f[:, O(2) + 1], f[:, X(3)] = [4.0, 4.0, 1.0], [4.0, 4.25, 0.25], [4.0, 4.5, 4.0]   # d_z == -L/2
    f[:, N(2)], f[:, N(2) + 1], f[:, X(4)] = [9.0, 4.0, 5.0], [9.25, 4.0, 5.75], [9.5, 4.0, 2.0]   # d_z == +L/2
    # a bond across each face, H and A wrapped differently (H on the far side of the face, A further in)
    f[:, O(5)], f[:, O(5) + 1], f[:, X(6)] = [0.3, 4.0, 3.0], [11.35, 4.0, 3.0], [9.5, 4.0, 3.0]
    f[:, O(7)], f[:, O(7) + 1], f[:, X(8)] = [7.0, 0.2, 3.0], [7.0, 8.25, 3.0], [7.0, 6.4, 3.0]
    f[:, O(9)], f[:, O(9) + 1], f[:, X(10)] = [7.0, 4.0, 0.4], [7.0, 4.0, 5.45], [7.0, 4.0, 3.6]
    f[:, N(11)], f[:, N(11) + 1], f[:, X(12)] = [11.8, 2.0, 1.0], [0.75, 2.0, 1.0], [2.6, 2.0, 1.0]  # ... and the other way
    # collinear (cos == -1) and perpendicular (cos == 0 exactly) neighbours
    f[:, N(13)], f[:, N(13) + 1], f[:, X(14)] = [2.0, 7.0, 3.0], [3.0, 7.0, 3.0], [4.5, 7.0, 3.0]
    f[:, O(15)], f[:, O(15) + 1], f[:, X(16)] = [6.0, 6.0, 3.0], [6.0, 7.0, 3.0], [8.0, 7.0, 3.0]
    f[:, O(17) + 1] = f[:, O(17)]                       # H on D: NaN
    f[:, X(18)] = f[:, O(17)] + [1.5, 0.0, 0.0]
    f[:, N(19) + 1] = f[:, X(20)] = f[:, N(19)] + [1.0, 0.5, 0.0]  # H on A: NaN
    don = [a for m in range(n_mol) for a in (O(m), N(m))]
    hyd = [h for m in range(n_mol) for h in ([O(m) + 1, O(m) + 2], [N(m) + 1])]
    acc = [a for m in range(n_mol) for a in (O(m), X(m))]
    top = _top(don, [0, 1] * n_mol, hyd, acc, [0, 1] * n_mol)
    return xyz, box, top, (np.arange(n) // 6).astype(np.int32)


@pytest.mark.parametrize("cos_cut", [COS150, 0.0, -1.0])
@pytest.mark.parametrize("r_ha", [None, R_HA])
@pytest.mark.parametrize("exclude", [False, True])
def test_edge_system(B, cos_cut, r_ha, exclude):
    xyz, box, top, mol_of = _edge_system()
    nb, nd, na, hist, degen = _check_counts(B, xyz, box, top, cos_cut=cos_cut, r_ha=r_ha,
                                            mol_of=mol_of if exclude else None)
    assert degen >= 2                                    # H on D and H on A
    if cos_cut > -1.0:
        assert (nb.sum(axis=0) > 0).all()                # bonds in each of the 2 x 2 class pairs
    else:
        assert nb[0].sum() >= 5                          # the planted straight bonds
    assert hist[:, :, 179].sum() > 0 and hist[:, :, 90].sum() > 0  # cos == -1 and cos == 0
    if not exclude:
        assert hist.sum() > _check_counts(B, xyz, box, top, cos_cut=cos_cut, r_ha=r_ha, mol_of=mol_of)[3].sum()


def test_edge_system_is_what_it_says():
    """The restatement on the planted atoms of frame 0: each edge does what the definition says."""
    xyz, box, top, mol_of = _edge_system()
    x, L = xyz[0], box[0]
    O, N, X = (lambda m: 6 * m), (lambda m: 6 * m + 3), (lambda m: 6 * m + 5)  # noqa: E731

    def one(d, h, a, cos_cut=COS150, r_ha_sq=0.0, frame=x):
        b = R.bonded(frame[None], L[None], [d], [0, 1], [h], [a], R_DA ** 2, r_ha_sq, cos_cut)
        return bool(b[0, 0, 0])

    assert float(R.rsq(x[:, O(0)], x[:, X(1)], L)) == R_DA ** 2 and not one(O(0), O(0) + 1, X(1))
    closer = x.copy()
    closer[0, X(1)] = 8.499
    assert one(O(0), O(0) + 1, X(1), frame=closer)      # ... and in when it is a hair closer
    assert x[2, O(2)] - x[2, X(3)] == -0.5 * L[2] and x[2, N(2)] - x[2, X(4)] == 0.5 * L[2]
    for d, a in ((O(5), X(6)), (O(7), X(8)), (O(9), X(10)), (N(11), X(12))):
        assert one(d, d + 1, a) and one(d, d + 1, a, r_ha_sq=R_HA ** 2)  # across a face: straight bonds
    c = R.cosine(x[:, N(13)], x[:, N(13) + 1], x[:, X(14)], L)
    assert c == -1.0 and one(N(13), N(13) + 1, X(14), cos_cut=-1.0)  # cos == cos_cut: in
    c = R.cosine(x[:, O(15)], x[:, O(15) + 1], x[:, X(16)], L)
    assert c == 0.0 and one(O(15), O(15) + 1, X(16), cos_cut=0.0) and not one(O(15), O(15) + 1, X(16))
    assert np.isnan(R.cosine(x[:, O(17)], x[:, O(17) + 1], x[:, X(18)], L))
    assert np.isnan(R.cosine(x[:, N(19)], x[:, N(19) + 1], x[:, X(20)], L))


# ---- structural cases ----

def _simple(rng, n_don, n_acc, n_frames, L, h_per_donor=1):
    """Donors with hydrogens 0.95 away, then the acceptors; one class each."""
    n_h = n_don * h_per_donor
    n = n_don + n_h + n_acc
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * np.asarray(L)[None, :, None], 3)
    hyd = []
    for d in range(n_don):
        hs = [n_don + d * h_per_donor + k for k in range(h_per_donor)]
        for h in hs:
            u = rng.normal(size=(n_frames, 3))
            u *= 0.95 / np.linalg.norm(u, axis=1)[:, None]
            xyz[:, :, h] = np.round(np.mod(xyz[:, :, d] + u, np.asarray(L)[None]), 3)
        hyd.append(hs)
    top = _top(np.arange(n_don), np.zeros(n_don), hyd, n_don + n_h + np.arange(n_acc), np.zeros(n_acc))
    return xyz, np.tile(np.asarray(L, dtype=np.float64), (n_frames, 1)), top


@pytest.mark.parametrize("n_don", [1, 15, 16, 17, 33])
def test_donor_counts_around_the_tile(B, n_don):
    xyz, box, top = _simple(np.random.default_rng(n_don), n_don, 150, 2, [9.0, 8.0, 7.0])
    want = _check_counts(B, xyz, box, top, cos_cut=float(np.cos(np.radians(110.0))), bin_size=2.0)
    assert want[3].sum() > 0


@pytest.mark.parametrize("n_acc", [4095, 4096, 4097])
def test_acceptor_counts_around_the_chunk(B, n_acc):
    """A dilute box: only the acceptors placed in line behind a hydrogen are bonded — the last ones of the list among
    them."""
    rng = np.random.default_rng(n_acc)
    xyz, box, top = _simple(rng, 3, n_acc, 1, [200.0, 200.0, 200.0])
    first = 6  # the first acceptor atom
    e = rng.normal(size=(3, 3))
    e /= np.linalg.norm(e, axis=1)[:, None]
    for d in range(3):
        xyz[0][:, d] = [50.0 + 40.0 * d, 100.0, 100.0]
        xyz[0][:, 3 + d] = np.round(xyz[0][:, d] + 0.95 * e[d], 3)
    for k, pos in enumerate([0, 1, n_acc - 1, n_acc - 2, 2000, 4094]):
        d = k % 3
        xyz[0][:, first + pos] = np.round(xyz[0][:, d] + e[d] * (2.7 + 0.1 * k), 3)
    nb, nd, na, _, _ = _check_counts(B, xyz, box, top)
    assert nb.sum() >= 4 and na[-1] == 1 and na[-2] == 1


def test_mixed_csr_rows(B):
    """Donors with 0, 1 and 3 hydrogens, in turn."""
    rng = np.random.default_rng(5)
    n_don, n_acc, L = 21, 120, np.array([9.0, 8.0, 7.0])
    per = [(0, 1, 3)[d % 3] for d in range(n_don)]
    n_h = sum(per)
    xyz = np.round(rng.uniform(0, 1, (2, 3, n_don + n_h + n_acc)) * L[None, :, None], 3)
    hyd, at = [], n_don
    for d in range(n_don):
        hyd.append(list(range(at, at + per[d])))
        for h in hyd[-1]:
            xyz[:, :, h] = np.round(np.mod(xyz[:, :, d] + rng.normal(size=(2, 3)) * 0.55, L[None]), 3)
        at += per[d]
    top = _top(np.arange(n_don), np.arange(n_don) % 2, hyd, n_don + n_h + np.arange(n_acc), np.zeros(n_acc))
    want = _check_counts(B, xyz, np.tile(L, (2, 1)), top, cos_cut=float(np.cos(np.radians(100.0))))
    assert want[1][0::3].sum() == 0 and want[1].sum() > 0
    only_bare = _top([0, 3], [0, 0], [[], []], top["acceptors"], top["acc_class"])
    assert _check_counts(B, xyz, np.tile(L, (2, 1)), only_bare)[3].sum() == 0  # n_h == 0


def test_no_histogram(B):
    xyz, box, top = _simple(np.random.default_rng(8), 20, 100, 2, [9.0, 8.0, 7.0])
    want = _check_counts(B, xyz, box, top, cos_cut=float(np.cos(np.radians(110.0))), bin_size=None)
    assert want[3].shape == (1, 1, 0) and want[0].sum() > 0


def test_device_input_and_calling_twice(B):
    import torch

    xyz, box, top = _simple(np.random.default_rng(9), 40, 200, 3, [10.0, 9.0, 8.0], h_per_donor=2)
    cut = float(np.cos(np.radians(110.0)))
    args = (top["donors"], top["don_class"], top["h_off"], top["h_atoms"], top["acceptors"], top["acc_class"],
            R_DA ** 2, cut)
    dev = torch.as_tensor(xyz, device="cuda")
    _check_counts(B, xyz, box, top, cos_cut=cut, xin=dev)
    edges = B.angle_cos_edges(1.0)
    a = B.hbond_counts(dev, box, *args, cos_edges=edges)
    b = B.hbond_counts(dev, box, *args, cos_edges=edges)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    la = B.hbond_lifetime(dev, box, *(args[:1] + args[2:4] + args[4:5]), R_DA ** 2, cut)
    lb = B.hbond_lifetime(xyz, box, *(args[:1] + args[2:4] + args[4:5]), R_DA ** 2, cut)
    want = R.hbond_lifetime(xyz, box, *(args[:1] + args[2:4] + args[4:5]), R_DA ** 2, cut)
    for u, v, w in zip(la, lb, want):
        assert np.array_equal(u, v) and np.array_equal(np.asarray(u).astype(np.int64), w)


def test_more_frames_than_a_launch_dimension(B):
    """70 001 frames of a six-atom system: the frames are flattened into the block index."""
    rng = np.random.default_rng(11)
    F, L = 70001, np.array([6.0, 5.5, 5.0])
    xyz = np.round(rng.uniform(0, 1, (F, 3, 6)) * L[None, :, None], 3)
    for d, h in ((0, 1), (2, 3)):
        xyz[:, :, h] = np.round(np.mod(xyz[:, :, d] + rng.normal(size=(F, 3)) * 0.55, L[None]), 3)
    top = _top([0, 2], [0, 1], [[1], [3]], [0, 4, 5], [0, 1, 1])
    want = _check_counts(B, xyz, np.tile(L, (F, 1)), top, cos_cut=float(np.cos(np.radians(120.0))), bin_size=5.0)
    assert want[0][-1000:].sum() > 0 and want[0][:1000].sum() > 0


# ---- lifetime ----

def _scripted(patterns, angle_out_every=3):
    """One (donor, hydrogen, acceptor) triple per pattern, 10 apart on a line in a large box; in frame t the acceptor
    of pair p sits in line behind the hydrogen (bonded) when patterns[p][t], else beyond r_da or — every third pair —
    within r_da at a right angle."""
    h = np.asarray(patterns, dtype=bool)
    P, F = h.shape
    L = np.array([10.0 * P + 10.0, 30.0, 30.0])
    xyz = np.zeros((F, 3, 3 * P))
    for p in range(P):
        d = np.array([5.0 + 10.0 * p, 15.0, 15.0])
        xyz[:, :, 3 * p] = d
        xyz[:, :, 3 * p + 1] = d + [0.95, 0.0, 0.0]
        out = d + ([0.95, 2.0, 0.0] if p % angle_out_every == 2 else [5.0, 0.0, 0.0])
        xyz[:, :, 3 * p + 2] = np.where(h[p][:, None], (d + [2.8, 0.0, 0.0])[None], out[None])
    top = _top(3 * np.arange(P), np.zeros(P), [[3 * p + 1] for p in range(P)], 3 * np.arange(P) + 2, np.zeros(P))
    return xyz, np.tile(L, (F, 1)), top


def _patterns(F, rng):
    rows = [np.ones(F, dtype=bool), (np.arange(F) % 4) < 2, rng.random(F) < 0.5, rng.random(F) < 0.9,
            np.zeros(F, dtype=bool)]
    for lo, hi in ((60, 70), (0, 64), (63, 65), (1, 128), (64, 129), (126, 129)):  # runs across the word boundaries
        r = np.zeros(F, dtype=bool)
        r[lo:hi] = True
        rows.append(r)
    rows.append(~rows[1])
    return np.array(rows)


def _lifetime_args(top):
    return top["donors"], top["h_off"], top["h_atoms"], top["acceptors"], R_DA ** 2, COS150


@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
def test_lifetime_scripted_patterns(B, F):
    pat = _patterns(F, np.random.default_rng(F))
    xyz, box, top = _scripted(pat)
    want_int, want_cont = R.lifetime_sums(pat, F - 1)
    assert want_int[0] == pat.sum() and want_cont[0] == pat.sum()
    for max_lag in sorted({0, F - 1}):
        c_int, c_cont, n_pairs, n_rec = B.hbond_lifetime(xyz, box, *_lifetime_args(top), max_lag=max_lag)
        assert c_int.dtype == np.uint64 and c_cont.dtype == np.uint64
        assert np.array_equal(c_int.astype(np.int64), want_int[:max_lag + 1])
        assert np.array_equal(c_cont.astype(np.int64), want_cont[:max_lag + 1])
        assert n_pairs == int(pat.any(axis=1).sum()) and n_rec == int(pat.sum())
        ref = R.hbond_lifetime(xyz, box, *_lifetime_args(top), max_lag=max_lag)
        assert np.array_equal(ref[0], want_int[:max_lag + 1]) and np.array_equal(ref[1], want_cont[:max_lag + 1])
        assert ref[2:] == (n_pairs, n_rec)
    k = np.arange(F)
    always = np.ones((1, F), dtype=bool)
    c_int, c_cont, _, _ = B.hbond_lifetime(*_scripted(always)[:2], *_lifetime_args(_scripted(always)[2]))
    assert np.array_equal(c_int.astype(np.int64), F - k) and np.array_equal(c_cont.astype(np.int64), F - k)


def test_lifetime_forced_resweep(B):
    """table_slots = 4 with 40 pairs: the first sweep's table fills, the call sweeps again and gives the same."""
    from mdproptools_amd._lib import default_context

    rng = np.random.default_rng(3)
    pat = rng.random((40, 70)) < 0.6
    xyz, box, top = _scripted(pat)
    want = R.lifetime_sums(pat, 69)
    plain = B.hbond_lifetime(xyz, box, *_lifetime_args(top))
    n_plain = default_context().last_kernel_ms()[1]
    forced = B.hbond_lifetime(xyz, box, *_lifetime_args(top), table_slots=4)
    n_forced = default_context().last_kernel_ms()[1]
    assert n_forced == n_plain + 1                       # one more sweep
    for res in (plain, forced):
        assert np.array_equal(res[0].astype(np.int64), want[0]) and np.array_equal(res[1].astype(np.int64), want[1])
        assert res[2] == 40 and res[3] == int(pat.sum())


def test_lifetime_frame_limit(B):
    """65 536 frames are refused with MDHIP_EINVAL and a text, before anything is launched."""
    from mdproptools_amd._lib import MdhipError

    F = 65536
    xyz = np.zeros((F, 3, 3))
    box = np.full((F, 3), 30.0)
    with pytest.raises(ValueError, match="at most 65535 frames") as err:
        B.hbond_lifetime(xyz, box, [0], [0, 1], [1], [2], R_DA ** 2, COS150, max_lag=10)
    assert isinstance(err.value.__cause__, MdhipError) and err.value.__cause__.code == -1
    # the frame limit itself is accepted
    c_int, c_cont, n_pairs, n_rec = B.hbond_lifetime(xyz[:65535], box[:65535], [0], [0, 1], [1], [2], R_DA ** 2, COS150,
                                                     max_lag=3)
    assert (n_pairs, n_rec) == (0, 0) and not c_int.any() and not c_cont.any()


# ---- non-finite input ----

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("r_ha", [None, R_HA])
def test_nonfinite_coordinates(B, bad, r_ha):
    """A non-finite coordinate on a donor, a hydrogen and an acceptor of frame 1: the counts are the restatement's, and
    the other frames are as without it."""
    xyz, box, top, mol_of = _edge_system(seed=4)
    clean = _check_counts(B, xyz, box, top, r_ha=r_ha, mol_of=mol_of)
    dirty = xyz.copy()
    dirty[1, 0, 6 * 3] = bad          # a donor (and acceptor) O
    dirty[1, 1, 6 * 7 + 1] = bad      # a hydrogen
    dirty[1, 2, 6 * 9 + 5] = bad      # an acceptor
    got = _check_counts(B, dirty, box, top, r_ha=r_ha, mol_of=mol_of)
    assert np.array_equal(got[0][[0, 2]], clean[0][[0, 2]])
    assert got[0][1].sum() <= clean[0][1].sum()
    life = B.hbond_lifetime(dirty, box, top["donors"], top["h_off"], top["h_atoms"], top["acceptors"], R_DA ** 2,
                            COS150, r_ha_sq=0.0 if r_ha is None else r_ha ** 2, mol_of=mol_of)
    want = R.hbond_lifetime(dirty, box, top["donors"], top["h_off"], top["h_atoms"], top["acceptors"], R_DA ** 2,
                            COS150, r_ha_sq=0.0 if r_ha is None else r_ha ** 2, mol_of=mol_of)
    assert np.array_equal(life[0].astype(np.int64), want[0]) and np.array_equal(life[1].astype(np.int64), want[1])
    assert life[2:] == want[2:] and life[3] == got[0].sum()


# ---- the public functions on dumps ----

def _water_like(seed, n_mol, n_frames, L):
    """n_mol three-atom molecules O H H (ids in molecule order) that drift a little from frame to frame."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    o = rng.uniform(0, 1, (3, n_mol)) * L[:, None]
    xyz = np.zeros((n_frames, 3, 3 * n_mol))
    u = rng.normal(size=(2, 3, n_mol))
    for f in range(n_frames):
        o = np.mod(o + rng.normal(size=o.shape) * 0.05, L[:, None])
        u = u + rng.normal(size=u.shape) * 0.15
        xyz[f][:, 0::3] = o
        for k in (0, 1):
            xyz[f][:, 1 + k::3] = np.mod(o + 0.95 * u[k] / np.linalg.norm(u[k], axis=0), L[:, None])
    return np.round(xyz, 4), np.tile(L, (n_frames, 1))


def test_dropin_functions_on_dumps(B, tmp_path):
    from mdproptools_amd.structural.hydrogen_bonds import calc_hbond_lifetime, calc_hydrogen_bonds

    n_mol, F = 90, 12
    xyz, box = _water_like(2, n_mol, F, [14.0, 13.0, 12.0])
    pattern = R.write_dumps(xyz, box, str(tmp_path), step=50)
    o = 3 * np.arange(n_mol)
    top = _top(o, np.zeros(n_mol), [[a + 1, a + 2] for a in o], o, np.zeros(n_mol))
    mol_of = np.arange(3 * n_mol) // 3
    cut = float(np.cos(np.radians(140.0)))
    edges = R.cos_edges(2.0)
    args = (top["donors"], top["don_class"], top["h_off"], top["h_atoms"], top["acceptors"], top["acc_class"])
    nb, nd, na, hist, degen = R.hbond_counts(xyz, box, *args, R_DA ** 2, cut, r_ha_sq=R_HA ** 2, edges=edges,
                                             mol_of=mol_of)
    assert nb.sum() > 20

    out = tmp_path / "hb.csv"
    per_frame, summary, angles = calc_hydrogen_bonds([(1, 2), (1, 3)], [1], pattern, [n_mol], [3], r_da=R_DA,
                                                     angle_cut=140.0, r_ha=R_HA, bin_size=2.0, path_or_buff=str(out))
    assert list(per_frame.columns) == ["Timestep", "hb_1-1"]
    assert np.array_equal(per_frame["Timestep"].to_numpy(), 50 * np.arange(F))
    assert np.array_equal(per_frame["hb_1-1"].to_numpy(), nb[:, 0, 0])
    assert out.read_text().splitlines()[0] == "Timestep,hb_1-1"
    assert np.array_equal(angles["count_1-1"].to_numpy(), hist[0, 0])
    total = int(nb.sum())
    assert summary["n_bonds"].iloc[0] == total and summary["n_degenerate"].iloc[0] == degen
    np.testing.assert_allclose(summary["bonds_per_donor_frame"].iloc[0], total / (n_mol * F), rtol=1e-13)
    np.testing.assert_allclose(summary["bonds_per_acceptor_frame"].iloc[0], total / (n_mol * F), rtol=1e-13)
    cen = (np.arange(len(edges)) + 0.5) * 2.0
    np.testing.assert_allclose(angles["adf_1-1"].to_numpy(), hist[0, 0] / (hist[0, 0].sum() * 2.0), rtol=1e-13)
    np.testing.assert_allclose(summary["mean_angle"].iloc[0], (hist[0, 0] * cen).sum() / hist[0, 0].sum(), rtol=1e-13)
    assert np.array_equal(summary.attrs["n_donated"].astype(np.int64), nd)
    assert np.array_equal(summary.attrs["n_accepted"].astype(np.int64), na)

    c_int, c_cont, n_pairs, n_rec = R.hbond_lifetime(xyz, box, top["donors"], top["h_off"], top["h_atoms"],
                                                     top["acceptors"], R_DA ** 2, cut, r_ha_sq=R_HA ** 2, mol_of=mol_of)
    out = tmp_path / "life.csv"
    table, info = calc_hbond_lifetime([(1, 2), (1, 3)], [1], pattern, [n_mol], [3], dt=2, r_da=R_DA, angle_cut=140.0,
                                      r_ha=R_HA, path_or_buff=str(out))
    assert list(table.columns) == ["Time (ps)", "C_int", "C_cont"]
    k = np.arange(F)
    delta = 50 * 2 * 1e-3
    np.testing.assert_allclose(table["Time (ps)"].to_numpy(), k * delta, rtol=1e-13)
    want_int = (c_int / (F - k)) / (c_int[0] / F)
    want_cont = (c_cont / (F - k)) / (c_cont[0] / F)
    np.testing.assert_allclose(table["C_int"].to_numpy(), want_int, rtol=1e-13)
    np.testing.assert_allclose(table["C_cont"].to_numpy(), want_cont, rtol=1e-13)
    assert info["n_pairs"] == n_pairs and info["n_frames"] == F
    np.testing.assert_allclose(info["bonds_per_frame"], n_rec / F, rtol=1e-13)
    np.testing.assert_allclose(info["tau_int"], R.trapezoid(want_int, delta), rtol=1e-13)
    np.testing.assert_allclose(info["tau_cont"], R.trapezoid(want_cont, delta), rtol=1e-13)
    assert out.read_text().splitlines()[0] == "Time (ps),C_int,C_cont"
    assert table["C_int"].iloc[0] == 1.0 and table["C_cont"].iloc[0] == 1.0
