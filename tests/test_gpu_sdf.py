"""
backend.sdf_hist / calc_spatial_distribution and their kernels (csrc/sdf.hip) on the GPU: every integer compared with
== against the numpy restatement (tests/sdf_ref.py, itself pinned by tests/test_sdf_cpu.py) — the lattice with a
closed form, the rotated clusters (handedness and axis order), the randomised systems built to hit every edge, the
structural cases (molecule counts around the tile, candidate counts around the chunk, more hits of one centre in one
chunk than a wave's queue holds, every lane hitting at once, G of 1, 2 and odd, the library's limits, device input,
repeated calls, more than 65 535 frames), non-finite input, and a cross-check against the hydration search that does
not pass through the restatement.
"""
import numpy as np
import pytest

import sdf_ref as R
from test_sdf_cpu import CHOSEN, _cells, handed_cluster

pytestmark = pytest.mark.gpu

QUEUE_DEPTH = 64 * (8 + 1)  # records of a wave's queue (csrc/sdf.hip: SDF_QUEUE)


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(B, xyz, box, o, p, q, cand, cls, S, r_cut, bin_size, mol_of=None, xin=None):
    """backend.sdf_hist against the restatement; returns the restatement's result."""
    got = B.sdf_hist(xin if xin is not None else xyz, box, o, p, q, cand, cls, S, r_cut, bin_size, mol_of=mol_of)
    want = R.sdf_hist(xyz, box, o, p, q, cand, cls, S, r_cut, bin_size, mol_of=mol_of)
    hist, degen, n_hits, bad = got
    assert hist.dtype == np.uint64 and degen.dtype == np.uint64 and n_hits.dtype == np.int32 and isinstance(bad, int)
    assert hist.shape == want[0].shape
    assert np.array_equal(n_hits, want[2])
    assert np.array_equal(degen.astype(np.int64), want[1])
    assert np.array_equal(hist.astype(np.int64), want[0])
    assert bad == want[3]
    return want


# ---- the closed forms ----

def test_lattice_backend_and_dropin(B, tmp_path):
    from mdproptools_amd.structural.spatial_distribution import calc_spatial_distribution

    xyz, box, num_mols, num_atoms = R.lattice()
    mol_of = np.concatenate([[0, 0, 0], 1 + np.arange(61)])
    h, _, _, _ = _check(B, xyz, box, [0], [1], [2], np.arange(3, 64), np.zeros(61, dtype=int), 1, 2.5, 1.0, mol_of=mol_of)
    assert _cells(h[0]) == {(0, 2, 2): 1, (2, 0, 2): 1, (2, 2, 4): 1, (2, 2, 0): 1}
    cls = np.concatenate([[1, 2, 3], np.zeros(61, dtype=int)])
    h, _, nh, _ = _check(B, xyz, box, [0], [1], [2], np.arange(64), cls, 4, 2.5, 1.0)
    assert _cells(h[2]) == {(4, 2, 2): 1} and _cells(h[3]) == {(2, 4, 2): 1} and nh.tolist() == [[6]]
    pattern = R.write_dumps(xyz, box, str(tmp_path))
    out = tmp_path / "sdf.npz"
    sdf, counts, axes, summary = calc_spatial_distribution(2.5, 1.0, (1, 1, 2, 3), [4], pattern, num_mols, num_atoms,
                                                           path_or_buff=str(out), cube=True)
    assert _cells(counts[0]) == {(0, 2, 2): 1, (2, 0, 2): 1, (2, 2, 4): 1, (2, 2, 0): 1}
    assert sdf[0, 0, 2, 2] == 512.0 / 61 and summary.iloc[0].tolist() == [4, 4, 0, 512.0 / 61, 4.0]
    assert np.array_equal(np.load(str(out))["counts"], counts) and (tmp_path / "sdf_4.cube").exists()
    _, counts, _, _ = calc_spatial_distribution(2.5, 1.0, (1, 1, 2, 3), [4, 2, 3], pattern, num_mols, num_atoms,
                                                exclude_same_molecule=False, save_mode=False)
    assert _cells(counts[1]) == {(4, 2, 2): 1} and _cells(counts[2]) == {(2, 4, 2): 1}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_handedness_backend_and_dropin(B, seed, tmp_path):
    from mdproptools_amd.structural.spatial_distribution import calc_spatial_distribution

    xyz, box = handed_cluster(seed)
    h, _, _, _ = _check(B, xyz, box, [0], [1], [2], np.arange(3, 7), np.zeros(4, dtype=int), 1, 3.5, 1.0)
    assert _cells(h[0]) == {cell: 1 for cell in CHOSEN}
    pattern = R.write_dumps(xyz, box, str(tmp_path))
    _, counts, _, _ = calc_spatial_distribution(3.5, 1.0, (1, 1, 2, 3), [4], pattern, [1, 4], [3, 1], save_mode=False)
    assert _cells(counts[0]) == {cell: 1 for cell in CHOSEN}


# ---- randomised systems with the edge cases (tests/test_sdf_cpu.py pins what they hold) ----

@pytest.mark.parametrize("seed,n,n_frames", [(1, 240, 2), (2, 402, 3), (3, 600, 2)])
@pytest.mark.parametrize("exclude", [False, True])
def test_random_systems_with_edges(B, seed, n, n_frames, exclude):
    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(seed, n, n_frames)
    if not exclude:  # the molecules' own atoms are candidates too: the origin atom is skipped, p and q are binned
        cand = np.arange(n, dtype=np.int32)
        cls = (cand % 3).astype(np.int32)
    h, d, nh, bad = _check(B, xyz, box, o, p, q, cand, cls, 3, R.EDGE_R_CUT, R.EDGE_BIN,
                           mol_of=mol_of if exclude else None)
    assert bad >= 2 and d.sum() >= 4 and h.sum() + d.sum() == nh.sum() and (h.sum(axis=(1, 2, 3)) > 0).all()
    # the degenerate rows' hits are in n_degenerate and nowhere else: without those two molecules nothing else changes
    keep = np.array([m for m in range(len(o)) if m not in (6, 7)])
    h2, d2, nh2, _ = R.sdf_hist(xyz[:1], box[:1], o[keep], p[keep], q[keep], cand, cls, 3, R.EDGE_R_CUT, R.EDGE_BIN,
                                mol_of=mol_of if exclude else None)
    h1, d1, nh1, _ = B.sdf_hist(xyz[:1], box[:1], o, p, q, cand, cls, 3, R.EDGE_R_CUT, R.EDGE_BIN,
                                mol_of=mol_of if exclude else None)
    assert np.array_equal(h1.astype(np.int64), h2) and int(d1.sum()) - int(d2.sum()) == int(nh1[0, 6] + nh1[0, 7])


# ---- structural cases ----

@pytest.mark.parametrize("n_mols", [1, 15, 16, 17, 33])
def test_molecule_counts_around_the_tile(B, n_mols):
    rng = np.random.default_rng(n_mols)
    n = 3 * n_mols + 150
    xyz = np.round(rng.uniform(0, 1, (2, 3, n)) * np.array([9.0, 8.0, 7.0])[None, :, None], 3)
    o = 3 * np.arange(n_mols)
    cand = np.arange(3 * n_mols, n)
    _check(B, xyz, np.tile([9.0, 8.0, 7.0], (2, 1)), o, o + 1, o + 2, cand, cand % 2, 2, 3.0, 0.5)


@pytest.mark.parametrize("n_cand", [4095, 4096, 4097])
def test_candidate_counts_around_the_chunk(B, n_cand):
    """A dilute box: only the candidates placed next to the three molecules are in a shell — the last ones of the
    candidate list among them."""
    rng = np.random.default_rng(n_cand)
    L = 200.0
    xyz = np.round(rng.uniform(0, 1, (1, 3, 9 + n_cand)) * L, 3)
    for m in range(3):
        xyz[0][:, 3 * m] = [50.0 + 30.0 * m, 100.0, 150.0]
        xyz[0][:, 3 * m + 1] = xyz[0][:, 3 * m] + [0.9, 0.1, 0.0]
        xyz[0][:, 3 * m + 2] = xyz[0][:, 3 * m] + [0.2, 1.0, 0.1]
    for k, at in enumerate([9, 10, 8 + n_cand, 7 + n_cand, 2000]):
        xyz[0][:, at] = xyz[0][:, 3 * (k % 3)] + np.round(rng.uniform(-1.5, 1.5, 3), 3)
    o = np.array([0, 3, 6])
    cand = np.arange(9, 9 + n_cand)
    h, _, nh, _ = _check(B, xyz, np.full((1, 3), L), o, o + 1, o + 2, cand, cand % 2, 2, 3.5, 0.5)
    assert h.sum() >= 5 and nh.min() >= 1


def _ball(rng, centre, k, r):
    """k points within r of `centre`, 3 decimals."""
    pts = rng.normal(size=(3, k))
    pts = pts / np.linalg.norm(pts, axis=0) * (r * rng.uniform(0.2, 0.95, k))
    return np.round(np.asarray(centre)[:, None] + pts, 3)


@pytest.mark.parametrize("n_in", [QUEUE_DEPTH - 1, QUEUE_DEPTH, QUEUE_DEPTH + 1, 4 * QUEUE_DEPTH + 65])
def test_more_hits_in_a_chunk_than_the_queue_holds(B, n_in):
    """One molecule with n_in candidates in its shell, all in one chunk and next to each other in the list (a wave sees
    64 hits per step): the queue is drained and filled again; a second, far molecule has none."""
    rng = np.random.default_rng(n_in)
    mols = np.array([[20.0, 20.0, 20.0], [20.9, 20.1, 20.0], [20.2, 21.0, 20.1],
                     [60.0, 60.0, 60.0], [60.9, 60.0, 60.0], [60.0, 60.9, 60.0]]).T
    far = np.round(rng.uniform(30.0, 50.0, (3, 300)), 3)
    xyz = np.concatenate([mols, far[:, :100], _ball(rng, [20.0] * 3, n_in, 3.0), far[:, 100:]], axis=1)[None]
    cand = np.arange(6, xyz.shape[2])
    assert len(cand) <= 4096
    h, _, nh, _ = _check(B, xyz, np.full((1, 3), 80.0), [0, 3], [1, 4], [2, 5], cand, cand % 3, 3, 3.5, 0.25)
    assert nh.tolist() == [[n_in, 0]] and h.sum() == n_in


def test_every_lane_hits_at_once(B):
    """33 molecules and 700 candidates in one small ball, in two frames: every (centre, candidate) test of every wave
    is a hit, 8 x 64 records per step."""
    rng = np.random.default_rng(64)
    n_mols, n_cand = 33, 700
    xyz = np.stack([_ball(rng, [10.0] * 3, 3 * n_mols + n_cand, 1.0) for _ in range(2)])
    o = 3 * np.arange(n_mols)
    cand = np.arange(3 * n_mols, 3 * n_mols + n_cand)
    h, d, nh, bad = _check(B, xyz, np.full((2, 3), 20.0), o, o + 1, o + 2, cand, cand % 8, 8, 2.5, 0.3125)
    assert (nh == n_cand).all() and bad == 0 and h.sum() == 2 * n_mols * n_cand


@pytest.mark.parametrize("bin_size,G", [(7.0, 1), (3.5, 2), (1.0, 7), (1.4, 5)])
def test_small_and_odd_grids(B, bin_size, G):
    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(5, 300)
    h, _, _, _ = _check(B, xyz, box, o, p, q, cand, cls, 3, 3.5, bin_size, mol_of=mol_of)
    assert h.shape == (3, G, G, G)


def test_library_limits(B):
    from mdproptools_amd._lib import MdhipError

    xyz, box, _, _ = R.lattice()
    cand, zero = np.arange(3, 64), np.zeros(61, dtype=int)
    args = (xyz, box, [0], [1], [2], cand)
    with pytest.raises(MdhipError, match="n_species must be in \\[1, 8\\]"):
        B.sdf_hist(*args, zero, 9, 2.5, 1.0)
    with pytest.raises(MdhipError, match="n_species must be in \\[1, 8\\]"):
        B.sdf_hist(*args, zero, 0, 2.5, 1.0)
    with pytest.raises(MdhipError, match="n_grid must be in \\[1, 256\\]"):
        B.sdf_hist(*args, zero, 1, 2.5, 5.0 / 257)
    with pytest.raises(MdhipError, match="n_species \\* n_grid\\*\\*3 must be at most 33554432"):
        B.sdf_hist(*args, zero, 8, 81.0, 1.0)  # G = 162: 8 * 162**3 = 34 012 224
    with pytest.raises(MdhipError, match="candidate 60: class 3 out of range"):
        B.sdf_hist(*args, np.where(cand == 63, 3, 0), 3, 2.5, 1.0)
    with pytest.raises(MdhipError, match="candidate 0: atom index 64 out of range"):
        B.sdf_hist(xyz, box, [0], [1], [2], [64], [0], 1, 2.5, 1.0)
    with pytest.raises(MdhipError, match="xy-plane atom 0: atom index -1 out of range"):
        B.sdf_hist(xyz, box, [0], [1], [-1], cand, zero, 1, 2.5, 1.0)
    with pytest.raises(ValueError, match="positive and finite"):
        B.sdf_hist(*args, zero, 1, 2.5, 0.0)
    # at the limits: 8 species; G = 256 with 2 species is 2**25 cells exactly
    _check(B, xyz, box, [0], [1], [2], cand, cand % 8, 8, 2.5, 1.0)
    assert B.sdf_grid(2.5, 5.0 / 256) == 256
    hist, degen, nh, bad = B.sdf_hist(*args, cand % 2, 2, 2.5, 5.0 / 256)
    assert hist.shape == (2, 256, 256, 256) and int(hist.sum()) == 4 and nh.tolist() == [[4]]
    got = {tuple(int(v) for v in ix) for ix in np.argwhere(hist)}
    want = R.sdf_hist(xyz, box, [0], [1], [2], cand, cand % 2, 2, 2.5, 5.0 / 256)[0]
    assert got == {tuple(int(v) for v in ix) for ix in np.argwhere(want)}
    # no molecules, no candidates, no frames
    h, d, nh, bad = B.sdf_hist(xyz, box, [], [], [], cand, zero, 1, 2.5, 1.0)
    assert h.sum() == 0 and nh.shape == (1, 0) and bad == 0
    h, d, nh, bad = B.sdf_hist(xyz, box, [0], [0], [2], [], [], 1, 2.5, 1.0)
    assert h.sum() == 0 and nh.tolist() == [[0]] and bad == 1  # (the degenerate rows are counted all the same)
    h, d, nh, bad = B.sdf_hist(xyz[:0], box[:0], [0], [1], [2], cand, zero, 1, 2.5, 1.0)
    assert h.shape == (1, 5, 5, 5) and h.sum() == 0 and nh.shape == (0, 1)


def test_device_input_and_repeated_calls(B):
    import torch

    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(4, 300, n_frames=3)
    _check(B, xyz, box, o, p, q, cand, cls, 3, 3.5, 0.875, mol_of=mol_of, xin=torch.as_tensor(xyz, device="cuda"))
    first = B.sdf_hist(xyz, box, o, p, q, cand, cls, 3, 3.5, 0.875, mol_of=mol_of)
    second = B.sdf_hist(xyz, box, o, p, q, cand, cls, 3, 3.5, 0.875, mol_of=mol_of)  # (the workspaces are zeroed again)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


def test_more_than_65535_frames(B):
    rng = np.random.default_rng(9)
    F = 70001
    xyz = np.round(rng.uniform(0, 5, (F, 3, 5)), 3)
    h, _, nh, _ = _check(B, xyz, np.full((F, 3), 5.0), [0], [1], [2], np.arange(5), [0, 1, 1, 0, 1], 2, 2.4, 0.6)
    assert h.sum() > F and nh.max() == 4


# ---- the frame pre-pass alone ----

@pytest.mark.parametrize("value", [None, float("nan"), float("inf"), -float("inf")])
def test_body_frames(B, value):
    """Every component of every frame is the restatement's double; degenerate rows are flagged and counted."""
    import torch

    xyz, box, o, p, q, _, _, _ = R.edge_system(7, 300, n_frames=3)
    n_mols = 33  # (three tiles; most molecules are three unrelated atoms)
    o = np.concatenate([o, 3 * np.arange(len(o), n_mols)]).astype(np.int32)
    p, q = o + 1, o + 2
    p[20] = o[20]  # p is o itself
    if value is not None:
        xyz[1, 0, o[8]] = xyz[0, 2, p[9]] = xyz[2, 1, q[3]] = value
        box = box.copy()
        box[2, 0] = value
    we, wv = R.body_frames(xyz, box, o, p, q)
    for xin in (xyz, torch.as_tensor(xyz, device="cuda")):
        e, valid, bad = B.body_frames(xin, box, o, p, q)
        assert e.shape == (3, n_mols, 3, 3) and valid.dtype == bool
        assert np.array_equal(valid, wv) and bad == int((~wv).sum())
        assert np.array_equal(e[wv], we[wv])
    assert not wv[0, 6] and not wv[0, 7] and not wv[:, 20].any() and wv[0, :6].all()
    rh = np.einsum("fmi,fmi->fm", np.cross(e[..., 0, :], e[..., 1, :]), e[..., 2, :])[wv]
    assert np.allclose(rh, 1.0, atol=1e-12)  # right-handed
    if value is not None:
        assert not wv[1, 8] and not wv[0, 9] and not wv[2, 3]
    e, valid, bad = B.body_frames(xyz[:, :, :5], box, [], [], [])
    assert e.shape == (3, 0, 3, 3) and bad == 0
    from mdproptools_amd._lib import MdhipError

    with pytest.raises(MdhipError, match="x-axis atom 1: atom index 300 out of range"):
        B.body_frames(xyz, box, [0, 3], [1, 300], [2, 5])


def test_body_frames_of_more_than_65535_frames(B):
    rng = np.random.default_rng(11)
    F = 70001
    xyz = np.round(rng.uniform(0, 5, (F, 3, 4)), 3)
    box = np.full((F, 3), 5.0)
    e, valid, bad = B.body_frames(xyz, box, [0, 1], [1, 2], [2, 3])
    we, wv = R.body_frames(xyz, box, [0, 1], [1, 2], [2, 3])
    assert np.array_equal(valid, wv) and np.array_equal(e[wv], we[wv]) and bad == int((~wv).sum())


# ---- non-finite input ----

@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_input(B, value):
    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(2, 240, n_frames=3)
    rc, bs = R.EDGE_R_CUT, R.EDGE_BIN
    clean = B.sdf_hist(xyz, box, o, p, q, cand, cls, 3, rc, bs)
    bad = xyz.copy()
    bad[1, 0, cand[5]] = value   # a candidate
    bad[1, 1, o[8]] = value      # o of molecule 8
    bad[0, 2, p[9]] = value      # p of molecule 9
    bad[2, 0, q[3]] = value      # q of molecule 3
    _, _, nh, rows = _check(B, bad, box, o, p, q, cand, cls, 3, rc, bs)
    assert nh[1, 8] == 0 and rows == clean[3] + 3
    touched = np.zeros(nh.shape, dtype=bool)
    touched[1, :] = True         # (the candidate may have been a hit of any row of its frame)
    assert np.array_equal(nh[~touched], clean[2][~touched])  # the degenerate rows keep their hits
    # ... and in a box edge of one frame: the restatement decides, the other frames do not change
    bbox = box.copy()
    bbox[1, 2] = value
    _, _, nh, _ = _check(B, xyz, bbox, o, p, q, cand, cls, 3, rc, bs, mol_of=mol_of)
    assert np.array_equal(nh[[0, 2]], B.sdf_hist(xyz, box, o, p, q, cand, cls, 3, rc, bs, mol_of=mol_of)[2][[0, 2]])


# ---- a cross-check that does not pass through the restatement ----

def test_hits_agree_with_the_hydration_search(B):
    """For every species: hist[s].sum() + n_degenerate[s] is the number of (origin atom, atom of s) pairs within r_cut,
    which the counts mode of the hydration search finds for the same centres (exclusion off; no species holds an
    origin atom; two trailing atoms so that every `water` has its two followers)."""
    xyz, box, o, p, q, cand, cls, _ = R.edge_system(6, 500, n_frames=3)
    cand, cls = cand[:-2], cls[:-2]
    hist, degen, nh, _ = B.sdf_hist(xyz, box, o, p, q, cand, cls, 3, 3.5, 0.875)
    total = np.zeros(nh.shape, dtype=np.int64)
    for s in range(3):
        n_water, _, _ = B.hydration_counts(xyz, box, o, cand[cls == s], B.cutoff_sq(3.5), 0.0, 0.5, 4)
        assert int(hist[s].sum()) + int(degen[s]) == int(n_water.sum()) > 0
        total += n_water
    assert np.array_equal(nh, total)
