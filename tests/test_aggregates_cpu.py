"""
calc_aggregates without a GPU: the numpy restatement (tests/aggregates_ref.py) on systems whose components are known in
closed form and against scipy's connected components, the host census on hand-made labels, the argument checks, and the
whole drop-in with backend.contact_components replaced by the restatement.
"""
import numpy as np
import pytest

import aggregates_ref as R


def _components(xyz, box, r_cut):
    n = xyz.shape[2]
    return R.contact_components(xyz, box, *R.all_atoms(n)[:4], [[r_cut ** 2]], *R.all_atoms(n)[4:])


def test_restatement_on_the_line():
    """12 atoms in shuffled order on a ring, spacing 2, cutoff 3: one component, every atom two neighbours."""
    xyz, box = R.line(12, 2.0, seed=3)
    assert sorted(xyz[0, 0]) == [2.0 * k for k in range(12)] and list(xyz[0, 0]) != sorted(xyz[0, 0])
    label, n_comp, n_con = _components(xyz, box, 3.0)
    assert np.array_equal(label, np.zeros((1, 12))) and list(n_comp) == [1] and list(n_con) == [24]
    xyz, box = R.line(12, 2.0, seed=3, cut=(0, 5))  # two atoms taken out: the arcs 1..4 and 6..11
    label, n_comp, n_con = _components(xyz, box, 3.0)
    assert list(n_comp) == [2] and list(n_con) == [2 * (3 + 5)]
    assert sorted(np.bincount(label[0])[np.unique(label[0])]) == [4, 6]
    for lab in np.unique(label[0]):  # the label is the smallest member
        assert lab == np.flatnonzero(label[0] == lab).min()


def test_restatement_on_the_lattice_and_the_paths():
    xyz, box = R.simple_cubic(4, 2.0)
    label, n_comp, n_con = _components(xyz, box, 2.5)
    assert list(n_comp) == [1] and list(n_con) == [64 * 6] and not label.any()
    label, n_comp, n_con = _components(xyz, box, 1.9)
    assert list(n_comp) == [64] and list(n_con) == [0] and np.array_equal(label[0], np.arange(64))
    xyz, box, parity = R.path(65, seed=1)
    label, n_comp, _ = _components(xyz, box, 1.5)
    assert list(n_comp) == [1] and not label.any()
    xyz, box, parity = R.path(65, seed=1, split=True)
    idx = np.arange(65)
    label, n_comp, n_con = R.contact_components(xyz, box, idx, parity, idx, parity, np.diag([2.25, 2.25]), idx, 65)
    assert list(n_comp) == [2] and list(n_con) == [2 * (32 + 31)]
    for p in (0, 1):
        assert set(label[0][parity == p]) == {idx[parity == p].min()}
    assert _components(xyz, box, 1.5)[1][0] == 1  # (without the classes the two chains are one)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_against_scipy(seed):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    rng = np.random.default_rng(seed)
    n = 150
    L = np.array([14.0, 12.0, 10.0])
    xyz = np.round(rng.uniform(0, 1, (1, 3, n)) * L[None, :, None], 3)
    label, n_comp, n_con = _components(xyz, L[None], 1.6)
    d = np.abs(xyz[0][:, :, None] - xyz[0][:, None, :])
    d = np.minimum(d, np.abs(d - L[:, None, None]))
    adj = ((d ** 2).sum(axis=0) < 1.6 ** 2) & ~np.eye(n, dtype=bool)
    k, lab = connected_components(sp.csr_matrix(adj), directed=False)
    assert 1 < k < n and k == n_comp[0] and n_con[0] == adj.sum()
    assert sorted(np.bincount(lab)) == sorted(np.bincount(label[0])[np.unique(label[0])])
    assert len(set(zip(lab, label[0]))) == k  # the same partition


def test_host_census_on_hand_made_labels():
    from mdproptools_amd.structural import aggregates as M

    # 7 nodes: types 1 1 1 2 2 2 2; frame 0: {0,3} {1,4,5} {2} {6}; frame 1: {0,3} {1,4} {2} {5} {6}
    node_type = np.array([1, 1, 1, 2, 2, 2, 2])
    labels = np.array([[0, 1, 2, 0, 1, 1, 6], [0, 1, 2, 0, 1, 5, 6]])
    census, sizes, per = M.census_of_labels(labels, node_type, [1, 2], ["Mg", "TFSI"], steps=[10, 20],
                                            n_contacts=[3, 2])
    assert list(census.columns) == ["Mg", "TFSI", "n_aggregates", "per_frame", "fraction"]
    # ordering: n_aggregates descending, then the composition columns ascending: (0,1) x3, (1,1) x3, (1,0) x2, (1,2) x1
    assert census[["Mg", "TFSI", "n_aggregates"]].to_numpy().tolist() == [[0, 1, 3], [1, 1, 3], [1, 0, 2], [1, 2, 1]]
    assert census["per_frame"].tolist() == [1.5, 1.5, 1.0, 0.5]
    assert census["fraction"].sum() == pytest.approx(1.0, abs=1e-15) and census["fraction"].iloc[0] == 3 / 9
    assert sizes.to_numpy().tolist() == [[1, 5, 5 / 14], [2, 3, 6 / 14], [3, 1, 3 / 14]]  # (singletons are counted)
    assert sizes["fraction_of_nodes"].sum() == pytest.approx(1.0, abs=1e-15)
    assert per.to_numpy().tolist() == [[10, 4, 3, 3], [20, 5, 2, 2]]
    rows, rsizes, rper = R.census(labels, node_type, steps=[10, 20], n_contacts=[3, 2])
    assert rows == [((0, 1), 3), ((1, 1), 3), ((1, 0), 2), ((1, 2), 1)]
    assert rsizes == {1: 5, 2: 3, 3: 1} and rper == [(10, 4, 3, 3), (20, 5, 2, 2)]


@pytest.fixture
def A(monkeypatch):
    """structural.aggregates with backend.contact_components replaced by the restatement."""
    from mdproptools_amd import backend
    from mdproptools_amd.structural import aggregates

    def fake(xyz, box, atoms_a, class_a, atoms_b, class_b, rsq_cut, node_of, n_nodes, ctx=None):
        label, n_comp, n_con = R.contact_components(xyz, box, atoms_a, class_a, atoms_b, class_b, rsq_cut, node_of,
                                                    n_nodes)
        return label.astype(np.int32), n_comp.astype(np.int32), n_con.astype(np.uint64)

    monkeypatch.setattr(backend, "contact_components", fake)
    return aggregates


def test_signature_and_argument_errors(A, tmp_path):
    import inspect

    sig = inspect.signature(A.calc_aggregates)
    assert list(sig.parameters) == ["contacts", "filename", "num_mols", "num_atoms_per_mol", "mol_names", "mol_types",
                                    "return_labels", "path_or_buff", "save_mode"]
    assert sig.parameters["path_or_buff"].default == "aggregates.csv" and sig.parameters["save_mode"].default is True
    xyz, box = R.line(12, 2.0, seed=3)
    pattern = R.write_dumps(xyz, box, np.arange(12) % 2 + 1, str(tmp_path))
    for bad in ([], None, [(1, 2)]):
        with pytest.raises(ValueError, match="non-empty list"):
            A.calc_aggregates(bad, pattern, save_mode=False)
    for dup in ([(1, 2, 3.0), (1, 2, 2.0)], [(1, 2, 3.0), (2, 1, 3.0)]):
        with pytest.raises(ValueError, match="given twice"):
            A.calc_aggregates(dup, pattern, save_mode=False)
    with pytest.raises(ValueError, match="no participating atom holds atom type 3"):
        A.calc_aggregates([(1, 3, 3.0)], pattern, save_mode=False)
    with pytest.raises(ValueError, match="no participating atom holds atom type 2"):
        A.calc_aggregates([(1, 2, 3.0)], pattern, mol_types=[1], save_mode=False)
    with pytest.raises(ValueError, match="no participating molecule holds atom type 4"):
        A.calc_aggregates([(1, 4, 3.0)], pattern, num_mols=[2, 5], num_atoms_per_mol=[1, 2], save_mode=False)
    with pytest.raises(ValueError, match="no participating molecule holds atom type 2"):
        A.calc_aggregates([(1, 2, 3.0)], pattern, num_mols=[2, 5], num_atoms_per_mol=[1, 2], mol_types=[1],
                          save_mode=False)
    with pytest.raises(ValueError, match=r"Length of values \(11\) does not match length of index \(12\)"):
        A.calc_aggregates([(1, 2, 3.0)], pattern, num_mols=[1, 5], num_atoms_per_mol=[1, 2], save_mode=False)


def test_dropin_on_the_line(A, tmp_path):
    """Atoms as nodes: the ring and its two arcs, two frames each; the census file."""
    out = tmp_path / "agg.csv"
    for cut, want_rows, want_sizes in (((), [[12, 2, 1.0, 1.0]], [[12, 2, 1.0]]),
                                       ((0, 5), [[4, 2, 1.0, 0.5], [6, 2, 1.0, 0.5]], [[4, 2, 0.4], [6, 2, 0.6]])):
        xyz, box = R.line(12, 2.0, seed=3, cut=cut)
        n = xyz.shape[2]
        xyz2, box2 = np.concatenate([xyz, xyz]), np.concatenate([box, box])
        pattern = R.write_dumps(xyz2, box2, np.ones(n, dtype=np.int64), str(tmp_path), stem="l%d" % len(cut))
        census, sizes, per, labels = A.calc_aggregates([(1, 1, 3.0)], pattern, return_labels=True,
                                                       path_or_buff=str(out))
        assert list(census.columns) == ["type_1", "n_aggregates", "per_frame", "fraction"]
        assert census.to_numpy().tolist() == want_rows and sizes.to_numpy().tolist() == want_sizes
        n_con = 24 if not cut else 16
        assert per.to_numpy().tolist() == [[0, len(want_rows), want_rows[-1][0], n_con],
                                           [1, len(want_rows), want_rows[-1][0], n_con]]
        assert labels.shape == (2, n) and labels.dtype == np.int32
        assert np.array_equal(labels, np.tile(_components(xyz, box, 3.0)[0], (2, 1)))
        assert out.read_text().splitlines()[0] == "type_1,n_aggregates,per_frame,fraction"
        assert len(out.read_text().splitlines()) == 1 + len(want_rows)


def test_dropin_with_a_molecule_layout(A, tmp_path):
    """2 cations (one atom), 3 anions (two atoms: altered types 2 and 3), 2 solvent molecules (three atoms: 4, 5, 6).
    Anion 0 bridges the two cations through its two atoms; anion 1 has both atoms next to each other and to nothing
    else; the solvent takes no part unless a contact names one of its atoms."""
    xyz, box = R.bridge_system()
    pattern = R.write_dumps(xyz, box, np.ones(14, dtype=np.int64), str(tmp_path))
    kw = dict(num_mols=[2, 3, 2], num_atoms_per_mol=[1, 2, 3], save_mode=False)
    census, sizes, per, labels = A.calc_aggregates([(1, 2, 1.5), (3, 1, 1.5), (2, 3, 1.5)], pattern,
                                                   mol_names=["Mg", "TFSI", "DME"], return_labels=True, **kw)
    assert list(census.columns)[:2] == ["Mg", "TFSI"]  # (no contact names a solvent atom)
    assert labels.tolist() == [[0, 0, 0, 3, 4]]  # nodes: cations 0, 1, anions 0, 1, 2
    assert census.to_numpy().tolist() == [[0, 1, 2, 2.0, 2 / 3], [2, 1, 1, 1.0, 1 / 3]]
    assert sizes.to_numpy().tolist() == [[1, 2, 0.4], [3, 1, 0.6]]
    assert per.to_numpy().tolist() == [[0, 3, 3, 2]]  # (the two atoms of anion 1 are no contact)
    # the same pairs whichever side is listed
    again = A.calc_aggregates([(2, 1, 1.5), (1, 3, 1.5), (3, 2, 1.5)], pattern, return_labels=True, **kw)
    assert again[3].tolist() == labels.tolist() and again[2]["n_contacts"].tolist() == [2]
    assert list(again[0].columns)[:2] == ["mol_1", "mol_2"]
    # a contact that names a solvent atom brings the solvent molecules in as nodes
    census, _, per = A.calc_aggregates([(1, 2, 1.5), (3, 1, 1.5), (1, 4, 1.5)], pattern, **kw)
    assert list(census.columns)[:3] == ["mol_1", "mol_2", "mol_3"] and per["n_aggregates"].tolist() == [5]
    # mol_types narrows the participants: without the anions nothing can link (and the contact is refused)
    with pytest.raises(ValueError, match="no participating molecule holds atom type 2"):
        A.calc_aggregates([(1, 2, 1.5)], pattern, mol_types=[1, 3], **kw)
    census, _, per = A.calc_aggregates([(1, 2, 1.5), (3, 1, 1.5), (1, 4, 1.5)], pattern, mol_types=[1, 2, 3], **kw)
    assert per["n_aggregates"].tolist() == [5]


def test_changing_types_raise(A, tmp_path):
    from mdproptools_amd.io import write_dump

    xyz, box = R.line(12, 2.0, seed=3)
    tab = np.column_stack([np.arange(1, 13), np.ones(12), xyz[0].T])
    for f, types in enumerate((np.ones(12), np.arange(12) % 2 + 1)):
        tab[:, 1] = types
        write_dump(str(tmp_path / ("t.%d.dump" % f)), f, np.column_stack([np.zeros(3), box[0]]),
                   ["id", "type", "x", "y", "z"], tab)
    with pytest.raises(ValueError, match="every frame must hold the same atom types in id order"):
        A.calc_aggregates([(1, 1, 3.0)], str(tmp_path / "t.*.dump"), save_mode=False)


def test_where_the_batches_are_cut_shows_in_no_result(A, tmp_path, monkeypatch):
    """Three different frames (the ring, its two arcs, the ring) in batches of one frame, two frames and everything:
    equal DataFrames and labels, the same CSV bytes."""
    from mdproptools_amd import backend
    from mdproptools_amd.common import trajectory

    fake, calls = backend.contact_components, []
    monkeypatch.setattr(backend, "contact_components",
                        lambda xyz, *a, **kw: calls.append(len(xyz)) or fake(xyz, *a, **kw))
    ring, box = R.line(12, 2.0, seed=3)
    arcs = ring.copy()
    arcs[0, :, [0, 5]] += 1.0  # two atoms moved off the line, out of reach: the ring falls into arcs and singletons
    xyz, boxes = np.concatenate([ring, arcs, ring]), np.concatenate([box, box, box])
    pattern = R.write_dumps(xyz, boxes, np.ones(12, dtype=np.int64), str(tmp_path))
    frame_bytes = 5 * 12 * 8  # the planes id type x y z of one frame
    results = []
    for k, cap in enumerate((frame_bytes, 2 * frame_bytes, trajectory.TYPED_BATCH_BYTES)):
        monkeypatch.setattr(trajectory, "TYPED_BATCH_BYTES", cap)
        out = tmp_path / ("agg%d.csv" % k)
        tables = A.calc_aggregates([(1, 1, 3.0)], pattern, return_labels=True, path_or_buff=str(out))
        results.append((tables, out.read_bytes()))
    assert calls == [1, 1, 1, 2, 1, 3]
    first = results[0][0]
    assert first[2]["n_aggregates"].tolist()[0] == 1 and first[2]["n_aggregates"].tolist()[1] > 1
    assert len(first[0]) > 1 and first[3].shape == (3, 12)
    for tables, text in results[1:]:
        assert all(t.equals(f) for t, f in zip(tables[:3], first[:3])) and np.array_equal(tables[3], first[3])
        assert text == results[0][1]
