"""
get_clusters / get_cluster_compositions and their kernels (csrc/clusters.hip) on the GPU: the reference's files byte
for byte on every recorded case, shells against the numpy restatement (tests/cluster_ref.py) on randomised systems
built to hit every edge (rsq == r_cut**2 exactly, d == +-L/2 exactly, ragged and boundary-spanning molecules, centres
in the first and last atom positions, centre counts off the tile width, device input), overflowing capacities, more
than 65 535 frames, and the force sums against pandas' groupby().sum() bit for bit.
"""
import os

import numpy as np
import pandas as pd
import pytest

import cluster_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def CA():
    from mdproptools_amd.structural import cluster_analysis

    return cluster_analysis


def _written(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.startswith("Cluster_"):
            with open(os.path.join(d, f), "rb") as fh:
                out[f] = fh.read()
    return out


@pytest.mark.parametrize("key", sorted(R.CASES))
def test_dropin_files(z, CA, key, tmp_path):
    want, n_want = R.expected_files(z, key)
    src, out = tmp_path / "dumps", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    pattern, sel = R.write_dumps(z, key, str(src))
    _, num_mols = R.frames_of(z, key)
    n = CA.get_clusters(pattern, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, elements=R.ELEMENTS,
                        working_dir=str(out), **sel, **R.CASES[key])
    assert n == n_want
    got = _written(str(out))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("key", ["A", "C", "D"])
def test_compositions(z, CA, key, tmp_path):
    pattern, sel = R.write_dumps(z, key, str(tmp_path))
    frames, num_mols = R.frames_of(z, key)
    kw = dict(R.CASES[key])
    clusters, conf = CA.get_cluster_compositions(pattern, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS,
                                                 mol_names=["dme", "tfsi", "mg"], **sel, **kw)
    ref = R.compositions(frames, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, **kw)
    cols = ["num_dme", "num_tfsi", "num_mg"]
    assert list(clusters.columns) == ["frame", "timestep", "centre_id"] + cols
    got = [(int(a), int(b), int(c), tuple(int(v) for v in r)) for a, b, c, r in
           zip(clusters["frame"], clusters["timestep"], clusters["centre_id"], clusters[cols].to_numpy())]
    assert got == ref
    # the same counts read back from the files the reference wrote: the molecules after the centre's own (an Mg ion,
    # absent when it failed the filter), told apart by their first atom (DME starts with O, TFSI with N, Mg alone)
    files, _ = R.expected_files(z, key)
    size = {b"O": (0, 16), b"N": (1, 15), b"Mg": (2, 1)}
    own_ok = [len(rows) > 0 and rows[0] == p for fr in frames
              for p, _, _, rows in R.frame_clusters(fr, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, **kw)]
    for row, name, skip in zip(got, sorted(files), own_ok):
        els = [ln.split(b"\t")[0] for ln in files[name].split(b"\n")[2:] if ln]
        i, counts = (1 if skip else 0), [0, 0, 0]
        while i < len(els):
            k, n = size[els[i]]
            counts[k] += 1
            i += n
        assert tuple(counts) == row[3], name
    assert conf["count"].sum() == len(clusters)
    assert list(conf["count"]) == sorted(conf["count"], reverse=True)
    np.testing.assert_allclose(conf["%"].sum(), 100.0)
    for _, r in conf.iterrows():
        assert ((clusters[cols] == r[cols].to_numpy()).all(axis=1)).sum() == r["count"]


def _random_system(rng, F, n_mols, L, grid=True):
    sizes = rng.integers(1, 9, n_mols)
    mol_of = np.repeat(np.arange(n_mols), sizes).astype(np.int32)
    N = len(mol_of)
    box = np.tile(np.asarray(L, dtype=np.float64), (F, 1))
    if grid:  # molecules as clumps on a 1/4 grid, some straddling the boundary: rsq == r_cut**2 and d == +-L/2 exactly
        base = rng.integers(0, 8, (F, 3, n_mols)).astype(np.float64) * (L[0] / 8)
        xyz = np.mod(base[:, :, mol_of] + rng.integers(-3, 4, (F, 3, N)) / 4.0, L[0])
    else:
        xyz = rng.uniform(0, 1, (F, 3, N)) * np.asarray(L)[None, :, None]
    return xyz, box, mol_of


def _oracle_shells(xyz, box, centres, mol_of, rc2):
    return [[R.shell(xyz[f], box[f], p, mol_of, rc2) for p in centres] for f in range(len(xyz))]


def _check(mols, count, want):
    for f, row in enumerate(want):
        for c, s in enumerate(row):
            assert count[f, c] == len(s)
            np.testing.assert_array_equal(mols[f, c, :len(s)], s)
            assert (mols[f, c, len(s):] == -1).all()


@pytest.mark.parametrize("seed,C,r_cut", [(0, 1, 2.0), (1, 17, 2.5), (2, 33, 3.0), (3, 16, 1.75), (4, 40, 4.0)])
def test_shell_members_random(B, seed, C, r_cut):
    rng = np.random.default_rng(seed)
    xyz, box, mol_of = _random_system(rng, 3, 150, [16.0, 16.0, 16.0])
    N = xyz.shape[2]
    # the last atom always, the first one too when there are two or more centres (C off the 16-centre tile: 1, 17, 33, 40)
    centres = [N - 1] if C == 1 else np.concatenate(([0], 1 + rng.choice(N - 2, C - 2, replace=False), [N - 1]))
    centres = np.asarray(centres, dtype=np.int32)
    rc2 = r_cut ** 2
    d = xyz[:, :, None, :] - xyz[:, :, centres][:, :, :, None]
    assert (np.abs(d) == 8.0).any()  # d == L/2 exactly somewhere
    mols, count = B.shell_members(xyz, box, centres, mol_of, rc2)
    want = _oracle_shells(xyz, box, centres, mol_of, rc2)
    _check(mols, count, want)
    exact = sum(int((R.rsq(xyz[f][:, p], xyz[f], box[f]) == rc2).sum()) for f in range(3) for p in centres)
    assert exact > 0 or C == 1  # rsq == r_cut**2 exactly occurred (and was excluded)
    import torch

    mols2, count2 = B.shell_members(torch.from_numpy(xyz).cuda(), box, centres, mol_of, rc2)
    np.testing.assert_array_equal(mols2, mols)
    np.testing.assert_array_equal(count2, count)


def test_shell_members_uniform_and_overflow(B):
    rng = np.random.default_rng(7)
    xyz, box, mol_of = _random_system(rng, 4, 300, [20.0, 21.0, 22.0], grid=False)
    centres = np.arange(0, xyz.shape[2], 37, dtype=np.int32)
    rc2 = 6.0 ** 2
    want = _oracle_shells(xyz, box, centres, mol_of, rc2)
    big = max(len(s) for row in want for s in row)
    assert big > 4
    m1, c1 = B.shell_members(xyz, box, centres, mol_of, rc2)
    m2, c2 = B.shell_members(xyz, box, centres, mol_of, rc2, cap=4)  # every frame re-run
    _check(m1, c1, want)
    _check(m2, c2, want)
    import torch

    m3, c3 = B.shell_members(torch.from_numpy(xyz).cuda(), box, centres, mol_of, rc2, cap=3)
    _check(m3, c3, want)


def test_shell_members_across_a_chunk_edge(B):
    xyz, box, mol_of, _, centres, K = R.chunk_straddling_system(np.random.default_rng(5))
    rc2 = 3.0 ** 2
    hits = [np.flatnonzero(R.rsq(xyz[1][:, p], xyz[1], box[1])[4094:4098] < rc2) + 4094 for p in centres[[0, 16]]]
    assert hits[0].tolist() == [4095, 4096] and hits[1].tolist() == [4097]
    want = _oracle_shells(xyz, box, centres, mol_of, rc2)
    for cap in (B.SHELL_CAP, 1):  # the default, and every row with more than one molecule re-run
        mols, count = B.shell_members(xyz, box, centres, mol_of, rc2, cap=cap)
        _check(mols, count, want)
        assert (mols[1, 0] == K).sum() == 1 and (mols[1, 16] == K).sum() == 1


def test_shell_members_past_launch_limit(B):
    F = 65535 * 2 + 3
    rng = np.random.default_rng(3)
    mol_of = np.array([0, 0, 1, 2, 2, 3], dtype=np.int32)
    xyz = rng.integers(0, 8 * 1024, (F, 3, 6)).astype(np.float64) / 1024.0
    box = np.full((F, 3), 8.0)
    centres = np.array([0, 3, 5], dtype=np.int32)
    rc2 = 3.0 ** 2
    mols, count = B.shell_members(xyz, box, centres, mol_of, rc2)
    # vectorised oracle over all frames (the restatement's arithmetic, per centre)
    for c, p in enumerate(centres):
        d = xyz[:, :, p:p + 1] - xyz
        L = box[:, :, None]
        d = np.where((d > L / 2) | (d < -L / 2), d - np.sign(d) * L, d)
        hit = (d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2) < rc2  # [F, N]
        per_mol = np.stack([hit[:, mol_of == m].any(axis=1) for m in range(4)], axis=1)
        np.testing.assert_array_equal(count[:, c], per_mol.sum(axis=1))
        for k in range(mols.shape[2]):
            want = np.array([np.flatnonzero(r)[k] if k < r.sum() else -1 for r in per_mol[-70000:]])
            np.testing.assert_array_equal(mols[-70000:, c, k], want)


def test_mol_kahan_sums_match_pandas(z, B):
    mol_of, seg_off, mol_type = R.layout(R.NUM_MOLS, R.NUM_ATOMS)
    force = z["f50_force"]
    got = B.mol_kahan_sums(force[None], seg_off)[0]
    df = pd.DataFrame({"m": mol_of, "fx": force[0], "fy": force[1], "fz": force[2]})
    want = df.groupby("m").agg({"fx": "sum", "fy": "sum", "fz": "sum"}).to_numpy().T
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
