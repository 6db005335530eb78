"""
backend.contact_components / calc_aggregates and their kernels (csrc/aggregates.hip) on the GPU: every integer compared
with == against the numpy restatement (tests/aggregates_ref.py) — systems whose components are known in closed form, a
deep tree, many unions of one component at once, the edges of the arithmetic (rsq == r_cut**2 exactly, d == +-L/2
exactly, links across each boundary, a per-frame box), class tables, molecules as nodes, and the structural cases (A
counts around the tile width, B counts around the chunk, a node without a listed atom, device input, repeated calls,
more than 65 535 frames, the library's limits).
"""
import numpy as np
import pytest

import aggregates_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(B, xyz, box, aa, ca, ab, cb, cut, node_of, n_nodes, xin=None):
    """backend.contact_components against the restatement; returns the restatement's (label, n_components,
    n_contacts)."""
    label, n_comp, n_con = B.contact_components(xin if xin is not None else xyz, box, aa, ca, ab, cb, cut, node_of,
                                                n_nodes)
    wl, wc, wn = R.contact_components(xyz, box, aa, ca, ab, cb, cut, node_of, n_nodes)
    assert label.dtype == np.int32 and n_comp.dtype == np.int32 and n_con.dtype == np.uint64
    assert label.shape == (len(xyz), n_nodes)
    assert np.array_equal(n_con.astype(np.int64), wn)
    assert np.array_equal(n_comp, wc)
    assert np.array_equal(label, wl)
    return wl, wc, wn


def _check_atoms(B, xyz, box, r_cut, **kw):
    aa, ca, ab, cb, node_of, n = R.all_atoms(xyz.shape[2])
    return _check(B, xyz, box, aa, ca, ab, cb, [[r_cut ** 2]], node_of, n, **kw)


def _check_types(B, xyz, box, types, contacts, node_of=None, n_nodes=None):
    aa, ca, ab, cb, cut = R.lists(types, contacts)
    n = xyz.shape[2]
    return _check(B, xyz, box, aa, ca, ab, cb, cut, np.arange(n) if node_of is None else node_of,
                  n if n_nodes is None else n_nodes)


def _check_dropin(census, sizes, per, labels, node_type, names, n_con):
    """The DataFrames of calc_aggregates against the dictionary restatement of the host tables."""
    rows, rsizes, rper = R.census(labels, node_type, n_contacts=n_con)
    F, n = labels.shape
    total = sum(c for _, c in rows)
    assert list(census.columns) == names + ["n_aggregates", "per_frame", "fraction"]
    assert census.to_numpy().tolist() == [list(comp) + [c, c / F, c / total] for comp, c in rows]
    assert sizes.to_numpy().tolist() == [[s, rsizes[s], s * rsizes[s] / (n * F)] for s in sorted(rsizes)]
    assert list(per.columns) == ["step", "n_aggregates", "largest", "n_contacts"]
    assert per.to_numpy().tolist() == [list(r) for r in rper]


# ---- closed forms ----

CLOSED = {"ring": (lambda: R.line(12, 2.0, seed=3), 3.0, [12], 24),
          "arcs": (lambda: R.line(12, 2.0, seed=3, cut=(0, 5)), 3.0, [4, 6], 16),
          "lattice": (lambda: R.simple_cubic(4, 2.0), 2.5, [64], 384),
          "lattice_apart": (lambda: R.simple_cubic(4, 2.0), 1.9, [1] * 64, 0)}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_forms_backend_and_dropin(B, name, tmp_path):
    from mdproptools_amd.structural.aggregates import calc_aggregates

    make, r_cut, want_sizes, want_contacts = CLOSED[name]
    xyz, box = make()
    n = xyz.shape[2]
    wl, wc, wn = _check_atoms(B, xyz, box, r_cut)
    assert sorted(np.bincount(wl[0])[np.unique(wl[0])]) == want_sizes and list(wn) == [want_contacts]
    assert wl[0].min() == 0 and (len(want_sizes) > 1 or not wl.any())
    xyz2, box2 = np.concatenate([xyz, xyz]), np.concatenate([box, box])
    pattern = R.write_dumps(xyz2, box2, np.ones(n, dtype=np.int64), str(tmp_path))
    out = tmp_path / "agg.csv"
    census, sizes, per, labels = calc_aggregates([(1, 1, r_cut)], pattern, return_labels=True, path_or_buff=str(out))
    assert labels.dtype == np.int32 and np.array_equal(labels, np.tile(wl, (2, 1)))
    _check_dropin(census, sizes, per, labels, np.ones(n, dtype=np.int64), ["type_1"], [want_contacts] * 2)
    assert sizes["size"].tolist() == sorted(set(want_sizes))
    assert out.read_text().splitlines()[0] == "type_1,n_aggregates,per_frame,fraction"


def test_molecules_as_nodes_backend_and_dropin(B, tmp_path):
    """Two atoms of one molecule within the cutoff: no link and no count; a molecule linked through two different
    atoms joins what they touch."""
    from mdproptools_amd.structural.aggregates import calc_aggregates

    xyz, box = R.bridge_system()
    altered = np.array([1, 1, 2, 3, 2, 3, 2, 3, 4, 5, 6, 4, 5, 6])
    mol = np.array([0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, 6, 6, 6])
    contacts = [(1, 2, 1.5), (3, 1, 1.5), (2, 3, 1.5)]
    wl, wc, wn = _check_types(B, xyz, box, altered, contacts, node_of=mol, n_nodes=5)
    assert wl.tolist() == [[0, 0, 0, 3, 4]] and list(wn) == [2]
    assert _check_types(B, xyz, box, altered, contacts)[2][0] == 3  # atoms as nodes: anion 1's own pair counts
    pattern = R.write_dumps(xyz, box, np.ones(14, dtype=np.int64), str(tmp_path))
    census, sizes, per, labels = calc_aggregates(contacts, pattern, num_mols=[2, 3, 2], num_atoms_per_mol=[1, 2, 3],
                                                 mol_names=["Mg", "TFSI", "DME"], return_labels=True, save_mode=False)
    assert np.array_equal(labels, wl)
    _check_dropin(census, sizes, per, labels, np.array([1, 1, 2, 2, 2]), ["Mg", "TFSI"], wn)
    assert census.to_numpy().tolist() == [[0, 1, 2, 2.0, 2 / 3], [2, 1, 1, 1.0, 1 / 3]]


# ---- a deep tree, and many unions of one component at once ----

def test_deep_tree(B):
    """A path of 4 097 nodes in shuffled index order: one component with label 0; its odd and even halves next to
    each other with classes that link only equal parities: two."""
    xyz, box, _ = R.path(4097, seed=7)
    wl, wc, wn = _check_atoms(B, xyz, box, 1.5)
    assert list(wc) == [1] and not wl.any() and list(wn) == [2 * 4096]
    xyz, box, parity = R.path(4097, seed=7, split=True)
    idx = np.arange(4097)
    wl, wc, wn = _check(B, xyz, box, idx, parity, idx, parity, np.diag([1.5 ** 2] * 2), idx, 4097)
    assert list(wc) == [2] and list(wn) == [2 * (2048 + 2047)]
    assert {int(wl[0][parity == p].max()) for p in (0, 1)} == {int(idx[parity == p].min()) for p in (0, 1)}


def test_contention(B):
    """64 A atoms and 512 B atoms in one ball smaller than the cutoff: 32 768 unions into one component."""
    xyz, box, aa, ab = R.contention(64, 512)
    n = xyz.shape[2]
    assert n == 577
    wl, wc, wn = _check(B, xyz, box, aa, np.zeros(64), ab, np.zeros(513), [[2.5 ** 2]], np.arange(n), n)
    assert list(wn) == [64 * 512] and list(wc) == [2]
    assert not wl[0, :576].any() and wl[0, 576] == 576


# ---- the edges of the arithmetic ----

@pytest.mark.parametrize("seed,n", [(1, 18), (2, 201), (3, 402)])
def test_random_systems_with_edges(B, seed, n):
    xyz, box, types = R.edge_system(seed, n)
    wl, wc, wn = _check_types(B, xyz, box, types, [(1, 2, 3.5)])
    d = xyz[0][:, 1] - xyz[0][:, 0]
    assert float((d ** 2).sum()) == 3.5 ** 2                      # the pair at exactly r_cut ...
    closer = xyz[:1].copy()
    closer[0, 0, 1] = 8.499
    aa, ca, ab, cb, cut = R.lists(types, [(1, 2, 3.5)])
    assert R.contact_components(closer, box[:1], aa, ca, ab, cb, cut, np.arange(n), n)[2][0] == wn[0] + 1  # ... is out
    if n == 18:  # nothing else around: the links of the edges themselves
        lab = wl[0]
        assert lab[1] != lab[0]                                   # exactly r_cut: no link
        assert lab[4] == lab[3] and lab[7] == lab[6]              # d == +L/2 and d == -L/2
        assert lab[10] == lab[13] == lab[16] == lab[9]            # across each of the three boundaries


def test_class_tables(B):
    xyz, box, types = R.edge_system(5, 300, n_frames=3)
    n = len(types)
    one = _check_types(B, xyz, box, types, [(1, 2, 3.5), (1, 3, 3.5)])
    two = _check_types(B, xyz, box, types, [(1, 2, 3.5), (1, 3, 2.0)])  # inside the larger cutoff, outside its own
    assert 0 < two[2].sum() < one[2].sum()
    only = _check_types(B, xyz, box, types, [(1, 2, 3.5)])
    aa, ca, ab, cb, cut = R.lists(types, [(1, 2, 3.5), (1, 3, 2.0)])
    for dead in (0.0, -1.0):  # an entry <= 0 never links, whatever is near
        cut[0, 1] = dead
        got = _check(B, xyz, box, aa, ca, ab, cb, cut, np.arange(n), n)
        assert np.array_equal(got[0], only[0]) and np.array_equal(got[2], only[2])
    both = _check_types(B, xyz, box, types, [(1, 1, 3.0), (2, 1, 2.5)])  # a type listed on both sides
    assert both[2].sum() > 0 and both[1].max() < n
    mol = np.arange(n) // 3  # molecules of three atoms as nodes; some of their own atoms are within the cutoff
    xyz[0][:, 22] = xyz[0][:, 21] + [0.5, 0.0, 0.0]
    as_mol = _check_types(B, xyz, box, types, [(1, 2, 3.5), (3, 1, 3.0)], node_of=mol, n_nodes=n // 3)
    as_atoms = _check_types(B, xyz, box, types, [(1, 2, 3.5), (3, 1, 3.0)])
    assert as_mol[2][0] < as_atoms[2][0]


# ---- structural cases ----

@pytest.mark.parametrize("n_a", [1, 15, 16, 17, 33])
def test_a_counts_around_the_tile(B, n_a):
    rng = np.random.default_rng(n_a)
    n = n_a + 150
    xyz = np.round(rng.uniform(0, 1, (2, 3, n)) * np.array([9.0, 8.0, 7.0])[None, :, None], 3)
    types = np.where(np.arange(n) < n_a, 1, 2)
    _check_types(B, xyz, np.tile([9.0, 8.0, 7.0], (2, 1)), types, [(1, 2, 1.4)])


@pytest.mark.parametrize("n_b", [4095, 4096, 4097])
def test_b_counts_around_the_chunk(B, n_b):
    """A dilute box: the three A atoms are joined only through the last two candidates of the list."""
    rng = np.random.default_rng(n_b)
    L = 200.0
    xyz = np.round(rng.uniform(0, 1, (1, 3, 3 + n_b)) * L, 3)
    types = np.where(np.arange(3 + n_b) < 3, 1, 2)
    xyz[0][:, :3] = np.array([[50.0, 100.0, 150.0], [54.0, 100.0, 150.0], [58.0, 100.0, 150.0]]).T
    xyz[0][:, 3] = [49.0, 100.5, 150.0]        # the first candidate: next to A 0 only
    xyz[0][:, 2 + n_b] = [52.0, 100.0, 150.0]  # the last one: between A 0 and A 1
    xyz[0][:, 1 + n_b] = [56.0, 100.0, 150.0]  # the one before: between A 1 and A 2
    wl, wc, wn = _check_types(B, xyz, np.full((1, 3), L), types, [(1, 2, 3.5)])
    assert wl[0][[0, 1, 2, 3, 1 + n_b, 2 + n_b]].tolist() == [0] * 6 and 5 <= wn[0] <= 12
    cutoff = xyz[:, :, :1 + n_b]  # without the last two the three stay apart
    assert R.contact_components(cutoff, np.full((1, 3), L), *R.lists(types[:1 + n_b], [(1, 2, 3.5)]),
                                np.arange(1 + n_b), 1 + n_b)[0][0][:3].tolist() == [0, 1, 2]


def test_node_without_a_listed_atom(B):
    """Nodes 0, 7 and the last three belong to no listed atom: they are their own labels. The two atoms that no list
    names carry a node index that is not one: it is never read."""
    xyz, box = R.line(12, 2.0, seed=3)
    node_of = np.full(12, -5)
    atoms = np.argsort(xyz[0, 0])[:10]  # the last two atoms of the ring are in no list: a chain of ten remains
    node_of[atoms] = [1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
    wl, wc, wn = _check(B, xyz, box, atoms, np.zeros(10), atoms, np.zeros(10), [[9.0]], node_of, 15)
    assert list(wc) == [6] and list(wn) == [18] and wl[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 7, 1, 1, 1, 1, 12, 13, 14]


def test_device_input_and_repeated_calls(B):
    import torch

    xyz, box, types = R.edge_system(4, 300, n_frames=3)
    aa, ca, ab, cb, cut = R.lists(types, [(1, 2, 3.5), (3, 1, 3.0)])
    args = (box, aa, ca, ab, cb, cut, np.arange(300), 300)
    _check(B, xyz, *args, xin=torch.as_tensor(xyz, device="cuda"))
    first = B.contact_components(xyz, *args)
    second = B.contact_components(xyz, *args)  # (the parent rows and the counters are initialised again)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert first[1].max() < 300


def test_more_than_65535_frames(B):
    rng = np.random.default_rng(9)
    F = 70001
    xyz = np.round(rng.uniform(0, 5, (F, 3, 5)), 3)
    wl, wc, wn = _check_atoms(B, xyz, np.full((F, 3), 5.0), 1.5)
    assert wn.sum() > F and wc.min() == 1 and wc.max() == 5


def test_library_limits(B):
    from mdproptools_amd._lib import MdhipError

    xyz, box = R.simple_cubic(2, 2.0)
    idx, z = np.arange(8), np.zeros(8)
    with pytest.raises(MdhipError, match="n_ca and n_cb must be in \\[1, 16\\]"):
        B.contact_components(xyz, box, idx, z, idx, z, np.full((17, 1), 6.25), idx, 8)
    with pytest.raises(MdhipError, match="n_ca and n_cb must be in \\[1, 16\\]"):
        B.contact_components(xyz, box, idx, z, idx, z, np.full((1, 17), 6.25), idx, 8)
    with pytest.raises(MdhipError, match="no positive cutoff"):
        B.contact_components(xyz, box, idx, z, idx, z, [[0.0, -1.0]], idx, 8)
    for bad in (-1, 8):
        with pytest.raises(MdhipError, match="A atom 3: atom index %d out of range" % bad):
            B.contact_components(xyz, box, np.where(idx == 3, bad, idx), z, idx, z, [[6.25]], idx, 8)
        with pytest.raises(MdhipError, match="B atom 7: atom index %d out of range" % bad):
            B.contact_components(xyz, box, idx, z, np.where(idx == 7, bad, idx), z, [[6.25]], idx, 8)
        with pytest.raises(MdhipError, match="atom 2: node %d out of range" % bad):
            B.contact_components(xyz, box, idx, z, idx, z, [[6.25]], np.where(idx == 2, bad, idx), 8)
    with pytest.raises(MdhipError, match="B atom 1: class 1 out of range"):
        B.contact_components(xyz, box, idx, z, idx, np.where(idx == 1, 1, 0), [[6.25]], idx, 8)
    # at the limits: 16 x 16 classes
    cls = idx % 16
    label, n_comp, n_con = B.contact_components(xyz, box, idx, cls, idx, cls, np.full((16, 16), 6.25), idx, 8)
    assert not label.any() and list(n_comp) == [1] and list(n_con) == [8 * 3]
