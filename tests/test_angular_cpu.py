"""
calc_angular_distribution without a GPU: the numpy restatement (tests/angular_ref.py) on lattices whose angle counts
are known in closed form, its asymmetric counting against the ordered-pair definition, its table binning against the
arccos rule it replaces, and the public function's signature, ValueErrors, normalisation and summary with
backend.angle_hist replaced by the restatement.
"""
import inspect

import numpy as np
import pytest

import angular_ref as R


def _lattice_hist(xyz, box, r_cut, bin_size):
    n = xyz.shape[2]
    edges = R.cos_edges(bin_size)
    hist, degen, count, centres = R.angle_hist(xyz, box, np.ones(n, dtype=np.int64), [(1, 1, 1)], [[r_cut ** 2] * 2],
                                               edges)
    assert len(centres) == n and degen[0] == 0
    return hist[0], count


def test_simple_cubic_counts():
    xyz, box = R.simple_cubic(4, 2.0)
    hist, count = _lattice_hist(xyz, box, 2.5, 7.0)
    assert len(hist) == 26 and np.all(count == 6)
    assert {int(7 * m): int(h) for m, h in enumerate(hist) if h} == {84: 768, 175: 192}


def test_fcc_counts():
    xyz, box = R.fcc(3, 2.0)
    assert xyz.shape[2] == 108
    hist, count = _lattice_hist(xyz, box, 1.5, 7.0)
    assert len(hist) == 26 and np.all(count == 12)
    assert {int(7 * m): int(h) for m, h in enumerate(hist) if h} == {56: 2592, 84: 1296, 119: 2592, 175: 648}


def test_simple_cubic_edges_at_one_degree():
    """cos == 0 exactly is <= E[90]: bin 90; the straight angles are in the last bin, 179."""
    xyz, box = R.simple_cubic(4, 2.0)
    hist, _ = _lattice_hist(xyz, box, 2.5, 1.0)
    assert len(hist) == 180
    assert {m: int(h) for m, h in enumerate(hist) if h} == {90: 768, 179: 192}


def test_asymmetric_counting_is_the_ordered_pair_definition():
    """A hand-made row: centre 0 (type 1); type-2 atoms at 1.0 (+x), 1.5 (+y), 2.5 (-x); a type-3 atom at 2.0 (+z)."""
    xyz = np.array([[5.0, 6.0, 5.0, 2.5, 5.0], [5.0, 5.0, 6.5, 5.0, 5.0], [5.0, 5.0, 5.0, 5.0, 7.0]])
    box = np.array([20.0, 20.0, 20.0])
    types = np.array([1, 2, 2, 2, 3])
    edges = R.cos_edges(10.0)
    trip = [(2, 1, 2), (2, 1, 2), (2, 1, 3), (3, 1, 2)]
    rc2 = np.array([[3.0, 3.0], [2.0, 3.0], [3.0, 3.0], [3.0, 3.0]]) ** 2
    hist, degen, count, centres = R.angle_hist(xyz[None], box[None], types, trip, rc2, edges)
    assert list(centres) == [0] and count[0, 0] == 4 and not degen.any()
    # symmetric, r 3: the unordered pairs of {1, 2, 3}: 90 (1, 2), 180 (1, 3), 90 (2, 3)
    assert {m: int(h) for m, h in enumerate(hist[0]) if h} == {9: 2, 17: 1}
    # same types, cutoffs 2 and 3: ordered (j in {1, 2}, k in {1, 2, 3}, j != k): (1,2) (1,3) (2,1) (2,3)
    assert {m: int(h) for m, h in enumerate(hist[1]) if h} == {9: 3, 17: 1}
    # 2-1-3 and 3-1-2: three ordered pairs each, all 90 degrees
    assert {m: int(h) for m, h in enumerate(hist[2]) if h} == {9: 3}
    assert np.array_equal(hist[2], hist[3])
    bh, bd = R.brute_hist(xyz, box, types, trip, rc2, edges)
    assert np.array_equal(bh, hist) and np.array_equal(bd, degen)


def _random_system(seed, n, box, n_frames=1):
    rng = np.random.default_rng(seed)
    L = np.asarray(box, dtype=np.float64)
    return np.round(rng.uniform(0, 1, (n_frames, 3, n)) * L[None, :, None], 3), np.tile(L, (n_frames, 1))


def test_table_binning_agrees_with_arccos():
    xyz, box = _random_system(20261019, 400, [12.0, 9.0, 7.0])
    x, L = xyz[0], box[0]
    edges = R.cos_edges(1.0)
    n_cos = 0
    for c in range(40):
        d = x - x[:, c:c + 1]
        d = np.stack([R._wrap(d[k], L[k]) for k in range(3)])
        rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        nb = np.flatnonzero((rsq < 3.5 ** 2) & (np.arange(400) != c))
        dd = d[:, nb]
        nrm = np.sqrt(rsq[nb])
        cos = ((dd[0][:, None] * dd[0][None] + dd[1][:, None] * dd[1][None]) + dd[2][:, None] * dd[2][None]) \
            / (nrm[:, None] * nrm[None])
        cos = cos[np.triu_indices(len(nb), 1)]
        assert np.array_equal(R.bin_of(cos, edges), R.arccos_bin(cos, 1.0, 180))
        n_cos += len(cos)
    assert n_cos > 10 ** 4


def test_restatement_equals_loops_on_a_random_system():
    xyz, box = _random_system(5, 60, [6.0, 5.0, 4.0])
    types = np.arange(60) % 3 + 1
    mol_of = np.arange(60) // 3
    xyz[0][:, 7] = xyz[0][:, 3]  # an atom on a centre: NaN
    trip = [(2, 1, 2), (2, 1, 3), (1, 1, 1), (3, 2, 3)]
    rc2 = np.array([[2.5, 2.5], [2.5, 2.0], [3.0, 3.0], [2.0, 2.5]]) ** 2
    edges = R.cos_edges(7.0)
    for mol in (None, mol_of):
        hist, degen, _, _ = R.angle_hist(xyz, box, types, trip, rc2, edges, mol_of=mol)
        bh, bd = R.brute_hist(xyz[0], box[0], types, trip, rc2, edges, mol_of=mol)
        assert np.array_equal(hist, bh) and np.array_equal(degen, bd)
        assert hist.sum() > 100
    assert R.angle_hist(xyz, box, types, trip, rc2, edges)[1].sum() > 0


# ---- the public function ----

@pytest.fixture
def A(monkeypatch):
    """structural.angular_distribution with backend.angle_hist replaced by the restatement."""
    from mdproptools_amd import backend
    from mdproptools_amd.structural import angular_distribution

    def fake(xyz, box, types, triplets, r_cut_sq, cos_edges, mol_of=None, cap=64, ctx=None):
        hist, degen, count, centres = R.angle_hist(xyz, box, types, triplets, r_cut_sq, cos_edges, mol_of=mol_of)
        return hist.astype(np.uint64), degen.astype(np.uint64), count.astype(np.int32), centres.astype(np.int32)

    monkeypatch.setattr(backend, "angle_hist", fake)
    return angular_distribution


def test_signature():
    from mdproptools_amd.structural import angular_distribution as M

    E = inspect.Parameter.empty
    want = [("r_cut", E), ("bin_size", E), ("triplets", E), ("filename", E), ("num_mols", None),
            ("num_atoms_per_mol", None), ("exclude_same_molecule", False), ("path_or_buff", "adf.csv"),
            ("save_mode", True)]
    sig = inspect.signature(M.calc_angular_distribution)
    assert [(p.name, p.default) for p in sig.parameters.values()] == want


def test_value_errors(tmp_path):
    from mdproptools_amd.structural import angular_distribution as M

    f = str(tmp_path / "none.*.dump")
    with pytest.raises(ValueError, match="num_mols and num_atoms_per_mol"):
        M.calc_angular_distribution(3.5, 1.0, [(2, 1, 2)], f, exclude_same_molecule=True, save_mode=False)
    with pytest.raises(ValueError, match="not strictly decreasing"):
        M.calc_angular_distribution(3.5, 1e-7, [(2, 1, 2)], f, save_mode=False)
    with pytest.raises(ValueError, match="bins"):
        M.calc_angular_distribution(3.5, 0.01, [(2, 1, 2)], f, save_mode=False)
    with pytest.raises(ValueError, match="histogram cells"):
        M.calc_angular_distribution(3.5, 0.1, [(2, 1, 2), (3, 1, 3), (2, 1, 3)], f, save_mode=False)
    with pytest.raises(ValueError, match="per triplet"):
        M.calc_angular_distribution([(3.5, 3.5)], 1.0, [(2, 1, 2), (3, 1, 3)], f, save_mode=False)
    with pytest.raises(ValueError, match="at most 8 triplets"):
        M.calc_angular_distribution(3.5, 10.0, [(2, 1, 2)] * 9, f, save_mode=False)


def test_normalisation_and_summary(A, tmp_path):
    """Two frames of the simple cubic lattice, every atom a centre: per frame 768 right and 192 straight angles."""
    xyz, box = R.simple_cubic(4, 2.0)
    xyz, box = np.concatenate([xyz, xyz]), np.concatenate([box, box])
    pattern = R.write_dumps(xyz, box, np.ones(64, dtype=np.int64), str(tmp_path))
    out = tmp_path / "adf.csv"
    adf, summary = A.calc_angular_distribution(2.5, 7.0, [(1, 1, 1)], pattern, path_or_buff=str(out))
    assert list(adf.columns) == ["angle", "adf_1-1-1", "count_1-1-1"] and len(adf) == 26
    assert np.array_equal(adf["angle"].to_numpy(), (np.arange(26) + 0.5) * 7.0)
    assert adf["count_1-1-1"].dtype == np.int64
    cnt = adf["count_1-1-1"].to_numpy()
    assert {m: int(h) for m, h in enumerate(cnt) if h} == {12: 1536, 25: 384}
    assert np.array_equal(adf["adf_1-1-1"].to_numpy(), cnt / (1920 * 7.0))
    assert (adf["adf_1-1-1"] * 7.0).sum() == pytest.approx(1.0)
    assert list(summary.columns) == ["triplet", "n_angles", "n_degenerate", "mean_angle", "angles_per_centre_frame"]
    row = summary.iloc[0]
    assert (row["triplet"], row["n_angles"], row["n_degenerate"]) == ("1-1-1", 1920, 0)
    assert row["mean_angle"] == pytest.approx((1536 * 87.5 + 384 * 178.5) / 1920)
    assert row["angles_per_centre_frame"] == 15.0
    import pandas as pd

    back = pd.read_csv(out)
    assert list(back.columns) == list(adf.columns) and np.array_equal(back["count_1-1-1"].to_numpy(), cnt)


def test_altered_types_exclusion_and_empty_triplet(A, tmp_path):
    """Molecules of 2 atoms (altered types 1, 2): with exclusion the partner atom of the centre's molecule is out."""
    xyz, box = R.simple_cubic(4, 2.0)
    pattern = R.write_dumps(xyz, box, np.ones(64, dtype=np.int64), str(tmp_path))
    kw = dict(num_mols=[32], num_atoms_per_mol=[2], save_mode=False)
    types = np.tile([1, 2], 32)
    edges = R.cos_edges(7.0)
    trip = [(2, 1, 2), (1, 1, 1), (3, 1, 3)]
    for excl in (False, True):
        adf, summary = A.calc_angular_distribution(2.5, 7.0, trip, pattern, exclude_same_molecule=excl, **kw)
        want, _, _, _ = R.angle_hist(xyz, box, types, trip, np.full((3, 2), 2.5 ** 2), edges,
                                     mol_of=np.arange(64) // 2 if excl else None)
        for t, name in enumerate(["2-1-2", "1-1-1", "3-1-3"]):
            assert np.array_equal(adf["count_" + name].to_numpy(), want[t])
        assert np.isnan(adf["adf_3-1-3"]).all() and np.isnan(summary["mean_angle"].iloc[2])
        assert summary["n_angles"].iloc[2] == 0
    assert want[0].sum() < R.angle_hist(xyz, box, types, trip, np.full((3, 2), 2.5 ** 2), edges)[0][0].sum()


def test_changing_types_raise(A, tmp_path):
    from mdproptools_amd.io import write_dump

    xyz, box = R.simple_cubic(2, 2.0)
    for f, types in enumerate([np.ones(8), np.array([1, 1, 1, 1, 1, 1, 1, 2.0])]):
        tab = np.column_stack([np.arange(1, 9), types, xyz[0].T])
        write_dump(str(tmp_path / ("t.%d.dump" % f)), f, np.column_stack([np.zeros(3), box[0]]),
                   ["id", "type", "x", "y", "z"], tab)
    with pytest.raises(ValueError, match="same atom types"):
        A.calc_angular_distribution(2.5, 7.0, [(1, 1, 1)], str(tmp_path / "t.*.dump"), save_mode=False)


def test_where_the_batches_are_cut_shows_in_no_result(A, tmp_path, monkeypatch):
    """Three different frames in batches of one frame, two frames and everything: equal DataFrames, the same CSV bytes."""
    from mdproptools_amd import backend
    from mdproptools_amd.common import trajectory

    fake, calls = backend.angle_hist, []
    monkeypatch.setattr(backend, "angle_hist", lambda xyz, *a, **kw: calls.append(len(xyz)) or fake(xyz, *a, **kw))
    n = 30
    xyz, box = _random_system(11, n, [6.0, 5.0, 4.0], n_frames=3)
    pattern = R.write_dumps(xyz, box, np.arange(n) % 3 + 1, str(tmp_path))
    frame_bytes = 5 * n * 8  # the planes id type x y z of one frame
    results = []
    for k, cap in enumerate((frame_bytes, 2 * frame_bytes, trajectory.TYPED_BATCH_BYTES)):
        monkeypatch.setattr(trajectory, "TYPED_BATCH_BYTES", cap)
        out = tmp_path / ("adf%d.csv" % k)
        adf, summary = A.calc_angular_distribution([(2.5, 2.5), (2.5, 2.0)], 7.0, [(2, 1, 2), (2, 1, 3)], pattern,
                                                   path_or_buff=str(out))
        results.append((adf, summary, out.read_bytes()))
    assert calls == [1, 1, 1, 2, 1, 3]
    assert results[0][0]["count_2-1-2"].sum() > 100 and results[0][0]["count_2-1-3"].sum() > 100
    for adf, summary, text in results[1:]:
        assert adf.equals(results[0][0]) and summary.equals(results[0][1]) and text == results[0][2]
