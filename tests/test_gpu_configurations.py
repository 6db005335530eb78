"""
The configuration census on the GPU (csrc/configurations.hip): get_configurations against the reference's recorded
CSVs and upstream's published digests, against the file route on files get_clusters wrote, and on the case the
reference cannot run; backend.shell_coordination against the numpy restatement (tests/config_ref.py) on randomised
systems built to hit every edge (rsq == r**2 exactly at both radii, d == +-L/2 exactly, centres in the first and last
atom positions, centre counts off the tile width, unsorted molecule types, a pass mask that fails own molecules,
device input), overflowing capacities and more than 65 535 frames.
"""
import hashlib
import os

import numpy as np
import pytest

import cluster_ref as R
import config_ref as CR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def g():
    return CR.load()


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def CA():
    from mdproptools_amd.structural import cluster_analysis

    return cluster_analysis


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _census(CA, z, key, src, working_dir=None, **over):
    """get_configurations on the dumps of census case `key` (written into `src`)."""
    case = CR.CASES[key]
    pattern, sel = R.write_dumps(z, case["files"], str(src))
    _, num_mols = R.frames_of(z, case["files"])
    kw = dict(R.CASES[case["files"]])
    kw.update(CR.census_kwargs(key))
    kw["coord_r_cut"], kw["r_cut"] = kw["r_cut"], R.CASES[case["files"]]["r_cut"]
    kw.update(over)
    return CA.get_configurations(pattern, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, elements=R.ELEMENTS,
                                 working_dir=working_dir, **sel, **kw)


@pytest.mark.parametrize("key", sorted(CR.CASES))
def test_trajectory_route_reproduces_the_reference(z, g, CA, key, tmp_path):
    src, out = tmp_path / "dumps", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    df, conf = _census(CA, z, key, src, working_dir=str(out))
    want, picks = CR.recorded(g, key)
    assert CR.csv_bytes(df) == want["clusters"]  # names, column order, values
    assert CR.csv_bytes(conf) == want["configurations"]  # order, count, %
    files, _ = R.expected_files(z, CR.CASES[key]["files"])
    assert sorted(os.listdir(str(out))) == sorted([n + ".csv" for n in want] +
                                                  ["conf_%d.xyz" % (k + 1) for k in range(len(picks))])
    for name in want:
        assert _read(str(out / (name + ".csv"))) == want[name], name
    for k, name in enumerate(picks):
        assert _read(str(out / ("conf_%d.xyz" % (k + 1)))) == files[name], name
    if key == "B":
        assert len(picks) == 5
        for name, oid, size in zip(CR.CSVS, g["upstream_oid"], g["upstream_size"]):
            data = _read(str(out / (name + ".csv")))
            assert (hashlib.sha256(data).hexdigest(), len(data)) == (str(oid), int(size)), name


def test_failing_own_molecules_are_counted(z, CA, tmp_path):
    """Case C, which the reference cannot run: all 33 centres, the ones whose own molecule fails the filter too."""
    frames, num_mols = R.frames_of(z, "C")
    pattern, sel = R.write_dumps(z, "C", str(tmp_path))
    df, conf = CA.get_configurations(pattern, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, elements=R.ELEMENTS,
                                     type_coord_atoms=["O", "N", "Mg"], find_top=False, **sel, **R.CASES["C"])
    rows = CR.direct_census(frames, num_mols, R.CASES["C"], R.CASES["C"]["r_cut"], R.ELEMENTS, ["O", "N", "Mg"])
    cl = R.frame_clusters(frames[0], num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, **R.CASES["C"])
    assert len(rows) == 33 and sum(1 for p, own, passing, _ in cl if own not in passing) == 6
    want_df, want_conf, _ = CR.tables(rows, 3, find_top=False)
    assert CR.csv_bytes(df) == CR.csv_bytes(want_df)
    assert CR.csv_bytes(conf) == CR.csv_bytes(want_conf)


@pytest.mark.parametrize("key", ["D2", "D3"])
def test_file_route_equals_trajectory_route(z, g, CA, key, tmp_path):
    src, out = tmp_path / "dumps", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    pattern, sel = R.write_dumps(z, "D", str(src))
    _, num_mols = R.frames_of(z, "D")
    n = CA.get_clusters(pattern, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, elements=R.ELEMENTS,
                        working_dir=str(out), **sel, **R.CASES["D"])
    assert n == len(R.expected_files(z, "D")[0])
    df_f, conf_f = CA.get_unique_configurations("Cluster_*.xyz", molecules=CR.molecules(g), mol_num=CR.MOL_NUM,
                                                working_dir=str(out), zip=False, **CR.census_kwargs(key))
    df_t, conf_t = _census(CA, z, key, src)
    assert CR.csv_bytes(df_t) == CR.csv_bytes(df_f)
    assert CR.csv_bytes(conf_t) == CR.csv_bytes(conf_f)


def _random_system(rng, F, n_mols, L, grid=True):
    sizes = rng.integers(1, 9, n_mols)
    mol_of = np.repeat(np.arange(n_mols), sizes).astype(np.int32)
    seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    N = len(mol_of)
    box = np.tile(np.asarray(L, dtype=np.float64), (F, 1))
    if grid:  # molecules as clumps on a 1/4 grid, some straddling the boundary: rsq == r**2 and d == +-L/2 exactly
        base = rng.integers(0, 8, (F, 3, n_mols)).astype(np.float64) * (L[0] / 8)
        xyz = np.mod(base[:, :, mol_of] + rng.integers(-3, 4, (F, 3, N)) / 4.0, L[0])
    else:
        xyz = rng.uniform(0, 1, (F, 3, N)) * np.asarray(L)[None, :, None]
    mol_type = rng.integers(1, 4, n_mols).astype(np.int32)  # not sorted: the rank is by type, not by index
    cls = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), N)
    return xyz, box, mol_of, seg_off, mol_type, cls


def _check(mols, words, count, want):
    for f, row in enumerate(want):
        for c, ent in enumerate(row):
            k = len(ent)
            assert count[f, c] == k
            assert [(int(m), int(w)) for m, w in zip(mols[f, c, :k], words[f, c, :k])] == ent, (f, c)
            assert (mols[f, c, k:] == -1).all() and (words[f, c, k:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


# r_coord below, equal to and above r_shell; every radius squared is a multiple of 1/16, as the grid's rsq are. The
# seeds are ones at which the system itself (no kernel involved) has what the assertions ahead of the call ask for;
# with a single centre, the last atom, few do.
@pytest.mark.parametrize("seed,C,r_shell,r_coord,masked", [(3, 1, 2.25, 1.75, True), (1, 17, 2.5, 2.5, True),
                                                          (2, 33, 3.0, 2.0, False), (3, 40, 1.75, 4.0, True)])
def test_shell_coordination_random(B, seed, C, r_shell, r_coord, masked):
    rng = np.random.default_rng(seed)
    xyz, box, mol_of, seg_off, mol_type, cls = _random_system(rng, 3, 150, [16.0, 16.0, 16.0])
    N = xyz.shape[2]
    centres = [N - 1] if C == 1 else np.concatenate(([0], 1 + rng.choice(N - 2, C - 2, replace=False), [N - 1]))
    centres = np.asarray(centres, dtype=np.int32)
    rs2, rc2 = r_shell ** 2, r_coord ** 2
    passes = (rng.uniform(size=(3, 150)) < 0.7) if masked else None
    d = xyz[:, :, None, :] - xyz[:, :, centres][:, :, :, None]
    assert (np.abs(d) == 8.0).any()  # d == L/2 exactly somewhere
    for r2 in (rs2, rc2):  # rsq == r**2 exactly occurs at both radii (and is excluded: the rows below)
        assert sum(int((R.rsq(xyz[f][:, p], xyz[f], box[f]) == r2).sum()) for f in range(3) for p in centres) > 0
    if masked:
        assert not passes[:, mol_of[centres]].all()  # some centres' own molecule fails
    want = CR.coordination_rows(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2, passes)
    assert max(len(e) for row in want for e in row) > 1
    mols, words, count = B.shell_coordination(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2,
                                              passes=passes)
    _check(mols, words, count, want)
    import torch

    mols2, words2, count2 = B.shell_coordination(torch.from_numpy(xyz).cuda(), box, centres, mol_of, seg_off,
                                                 mol_type, cls, rs2, rc2, passes=passes)
    np.testing.assert_array_equal(mols2, mols)
    np.testing.assert_array_equal(words2, words)
    np.testing.assert_array_equal(count2, count)


def test_shell_coordination_overflow(B):
    rng = np.random.default_rng(7)
    xyz, box, mol_of, seg_off, mol_type, cls = _random_system(rng, 4, 300, [20.0, 21.0, 22.0], grid=False)
    centres = np.arange(0, xyz.shape[2], 37, dtype=np.int32)
    rs2, rc2 = 6.0 ** 2, 4.5 ** 2
    passes = rng.uniform(size=(4, 300)) < 0.8
    want = CR.coordination_rows(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2, passes)
    assert max(len(e) for row in want for e in row) > 4
    args = (box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2)
    _check(*B.shell_coordination(xyz, *args, passes=passes), want)
    _check(*B.shell_coordination(xyz, *args, passes=passes, cap=4), want)  # every frame re-run, with its own mask
    import torch

    _check(*B.shell_coordination(torch.from_numpy(xyz).cuda(), *args, passes=passes, cap=3), want)


def test_shell_coordination_across_a_chunk_edge(B):
    rng = np.random.default_rng(5)
    xyz, box, mol_of, seg_off, centres, K = R.chunk_straddling_system(rng)
    n_mols = len(seg_off) - 1
    mol_type = rng.integers(1, 4, n_mols).astype(np.int32)
    cls = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), len(mol_of))
    cls[4094:4098] = [0, 1, 2, 1]
    passes = rng.uniform(size=(2, n_mols)) < 0.7
    passes[:, K] = True
    rs2, rc2 = 3.0 ** 2, 2.0 ** 2
    hits = [np.flatnonzero(R.rsq(xyz[1][:, p], xyz[1], box[1])[4094:4098] < rs2) + 4094 for p in centres[[0, 16]]]
    assert hits[0].tolist() == [4095, 4096] and hits[1].tolist() == [4097]
    want = CR.coordination_rows(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2, passes)
    assert (K, (1 << 8) + (1 << 16)) in want[1][0] and (K, 1 << 8) in want[1][16]
    for cap in (B.SHELL_CAP, 1):  # the default, and every row with more than one record re-run
        mols, words, count = B.shell_coordination(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2,
                                                  passes=passes, cap=cap)
        _check(mols, words, count, want)
        assert (mols[1, 0] == K).sum() == 1 and (mols[1, 16] == K).sum() == 1


def test_shell_coordination_past_launch_limit(B):
    F = 65535 * 2 + 3
    rng = np.random.default_rng(3)
    mol_of = np.array([0, 0, 1, 2, 2, 3], dtype=np.int32)
    seg_off = np.array([0, 2, 3, 5, 6], dtype=np.int64)
    mol_type = np.array([2, 1, 2, 1], dtype=np.int32)
    cls = np.array([0, 1, 0xFF, 1, 1, 0], dtype=np.uint8)
    xyz = rng.integers(0, 8 * 1024, (F, 3, 6)).astype(np.float64) / 1024.0
    box = np.full((F, 3), 8.0)
    centres = np.array([0, 3, 5], dtype=np.int32)
    rs2, rc2 = 3.0 ** 2, 2.5 ** 2
    passes = rng.uniform(size=(F, 4)) < 0.8
    mols, words, count = B.shell_coordination(xyz, box, centres, mol_of, seg_off, mol_type, cls, rs2, rc2,
                                              passes=passes, cap=4)
    assert mols.shape == (F, 3, 4)
    # vectorised oracle over all frames (the restatement's arithmetic, per centre)
    weight = np.where(cls == 0xFF, 0, 1 << (8 * np.minimum(cls, 7).astype(np.int64)))
    none = np.int64(1) << 62
    for c, p in enumerate(centres):
        d = xyz[:, :, p:p + 1] - xyz
        L = box[:, :, None]
        d = np.where((d > L / 2) | (d < -L / 2), d - np.sign(d) * L, d)
        rsq = d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2  # [F, N]
        member = np.stack([(rsq[:, mol_of == m] < rs2).any(axis=1) for m in range(4)], axis=1) & passes
        member[:, mol_of[p]] = False
        word = np.stack([((rsq[:, mol_of == m] < rc2) * weight[mol_of == m]).sum(axis=1) for m in range(4)], axis=1)
        key = np.where(member, (mol_type.astype(np.int64) << 32) + (word << 8) + np.arange(4), none)
        order = np.argsort(key, axis=1)
        is_m = np.take_along_axis(member, order, axis=1)
        np.testing.assert_array_equal(count[:, c], member.sum(axis=1))
        np.testing.assert_array_equal(mols[:, c], np.where(is_m, order, -1))
        np.testing.assert_array_equal(words[:, c], np.where(is_m, np.take_along_axis(word, order, axis=1),
                                                            -1).astype(np.uint64))


def test_too_many_classes_or_atoms_are_refused(B):
    xyz = np.zeros((1, 3, 256))
    box = np.full((1, 3), 8.0)
    centres = np.array([0], dtype=np.int32)
    nine = (np.arange(256) % 9).astype(np.uint8)
    one = np.arange(256, dtype=np.int32) // 128
    with pytest.raises(ValueError, match="classes"):
        B.shell_coordination(xyz, box, centres, one, [0, 128, 256], [1, 1], nine, 1.0, 1.0)
    with pytest.raises(ValueError, match="255 atoms"):
        B.shell_coordination(xyz, box, centres, np.zeros(256, dtype=np.int32), [0, 256], [1], nine % 8, 1.0, 1.0)
