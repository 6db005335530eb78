"""
The configuration census without a GPU: the numpy restatement (tests/config_ref.py) against the reference's recorded
CSVs (tests/golden/configurations.npz), and get_unique_configurations — the file route, host only — against upstream's
published answer for its own test call (the sha256 and sizes of its git-LFS pointer files, its conf_*.xyz picks).
"""
import hashlib
import inspect
import os
import warnings
import zipfile

import pandas as pd
import pytest

import cluster_ref as R
import config_ref as CR


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def g():
    return CR.load()


@pytest.fixture(scope="module")
def CA():
    from mdproptools_amd.structural import cluster_analysis

    return cluster_analysis


def _put(files, d):
    for name, data in files.items():
        with open(os.path.join(str(d), name), "wb") as fh:
            fh.write(data)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("key", sorted(CR.CASES))
def test_restatement_reproduces_the_recorded_csvs(z, g, key):
    case = CR.CASES[key]
    files, _ = R.expected_files(z, case["files"])
    rows = CR.file_census(files, case["r_cut"], CR.molecules(g), CR.MOL_NUM, case["type_coord_atoms"])
    df, conf, top = CR.case_tables(key, rows)
    want, picks = CR.recorded(g, key)
    assert CR.csv_bytes(df) == want["clusters"]
    assert CR.csv_bytes(conf) == want["configurations"]
    assert (top is not None) == ("top_conf" in want)
    if top is not None:
        assert CR.csv_bytes(top) == want["top_conf"]
        assert list(top["cluster"]) == picks
    # the census taken from the frames gives the same rows
    frames, num_mols = R.frames_of(z, case["files"])
    direct = CR.direct_census(frames, num_mols, R.CASES[case["files"]], case["r_cut"], R.ELEMENTS,
                              case["type_coord_atoms"])
    assert direct == rows


@pytest.mark.parametrize("key", sorted(CR.CASES))
def test_no_shell_atom_is_near_the_cutoff(z, key):
    """What lets the two routes agree: 10-decimal text and < against <= cannot matter at a gap above 1e-6."""
    case = CR.CASES[key]
    files, _ = R.expected_files(z, case["files"])
    gap = CR.shell_gaps(files, case["r_cut"]).min()
    print(key, "smallest |distance - r_cut|:", gap)
    assert gap > 1e-6


def test_file_route_reproduces_upstream(z, g, CA, tmp_path):
    files, _ = R.expected_files(z, "B")
    _put(files, tmp_path)
    kw = CR.census_kwargs("B")
    df, conf = CA.get_unique_configurations("Cluster_*.xyz", molecules=CR.molecules(g), mol_num=CR.MOL_NUM,
                                            working_dir=str(tmp_path), zip=False, **kw)
    want, picks = CR.recorded(g, "B")
    for name, oid, size in zip(CR.CSVS, g["upstream_oid"], g["upstream_size"]):
        data = _read(str(tmp_path / (name + ".csv")))
        assert (hashlib.sha256(data).hexdigest(), len(data)) == (str(oid), int(size)), name
        assert data == want[name]
    assert len(picks) == 5
    assert sorted(p.name for p in tmp_path.glob("conf_*.xyz")) == ["conf_%d.xyz" % (k + 1) for k in range(5)]
    for k, name in enumerate(picks):
        assert _read(str(tmp_path / ("conf_%d.xyz" % (k + 1)))) == files[name]
    assert sorted(p.name for p in tmp_path.glob("Cluster_*.xyz")) == sorted(files)  # zip=False: left in place
    # the returned frames are the CSVs
    assert CR.csv_bytes(df) == want["clusters"]
    assert CR.csv_bytes(conf) == want["configurations"]
    back = pd.read_csv(str(tmp_path / "clusters.csv")).fillna("")
    pd.testing.assert_frame_equal(df, back, check_dtype=False)
    assert list(df.columns) == ["cluster", "num_dme", "num_tfsi", "num_mg", "atoms_dme", "atoms_tfsi", "atoms_mg"]
    assert list(conf.columns) == list(df.columns)[1:] + ["count", "%"]


@pytest.mark.parametrize("key", ["A", "D1", "D2", "D3"])
def test_file_route_other_cases(z, g, CA, key, tmp_path):
    case = CR.CASES[key]
    files, _ = R.expected_files(z, case["files"])
    _put(files, tmp_path)

    class Mol:  # what a pymatgen Molecule offers the census
        def __init__(self, species):
            self.species = species

    df, conf = CA.get_unique_configurations("Cluster_*.xyz", molecules=[Mol(s) for s in CR.molecules(g)],
                                            mol_num=CR.MOL_NUM, working_dir=str(tmp_path), zip=False,
                                            **CR.census_kwargs(key))
    want, picks = CR.recorded(g, key)
    for name in CR.CSVS:
        path = str(tmp_path / (name + ".csv"))
        assert os.path.exists(path) == (name in want)
        if name in want:
            assert _read(path) == want[name], name
    for k, name in enumerate(picks):
        assert _read(str(tmp_path / ("conf_%d.xyz" % (k + 1)))) == files[name]
    assert len(list(tmp_path.glob("conf_*.xyz"))) == len(picks)
    assert CR.csv_bytes(df) == want["clusters"] and CR.csv_bytes(conf) == want["configurations"]


def test_zip_moves_the_cluster_files(z, g, CA, tmp_path):
    files, _ = R.expected_files(z, "B")
    _put(files, tmp_path)
    CA.get_unique_configurations("Cluster_*.xyz", molecules=CR.molecules(g), mol_num=CR.MOL_NUM,
                                 working_dir=str(tmp_path), **CR.census_kwargs("B"))
    assert not list(tmp_path.glob("Cluster_*.xyz")) and not (tmp_path / "Clusters").exists()
    with zipfile.ZipFile(str(tmp_path / "Clusters.zip")) as zf:
        assert sorted(zf.namelist()) == sorted(files) and len(files) == 33
        for name in files:
            assert zf.read(name) == files[name]
    assert len(list(tmp_path.glob("conf_*.xyz"))) == 5


def test_signature_is_the_references(CA):
    sig = inspect.signature(CA.get_unique_configurations)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("cluster_pattern", inspect.Parameter.empty), ("r_cut", inspect.Parameter.empty),
        ("molecules", inspect.Parameter.empty), ("mol_num", inspect.Parameter.empty), ("type_coord_atoms", None),
        ("working_dir", None), ("find_top", True), ("perc", None), ("cum_perc", 90), ("mol_names", None),
        ("zip", True)]


def test_percentage_rules(z, g, CA, tmp_path):
    files, _ = R.expected_files(z, "B")
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
        _put(files, d)
    common = dict(molecules=CR.molecules(g), mol_num=CR.MOL_NUM, type_coord_atoms=["O", "N", "Mg"], zip=False)
    with pytest.warns(UserWarning, match="using cum_perc"):
        CA.get_unique_configurations("Cluster_*.xyz", 2.3, working_dir=str(a), perc=50, cum_perc=100, **common)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        CA.get_unique_configurations("Cluster_*.xyz", 2.3, working_dir=str(b), perc=None, cum_perc=100, **common)
    assert _read(str(a / "top_conf.csv")) == _read(str(b / "top_conf.csv"))  # cum_perc won
    assert len(list(a.glob("conf_*.xyz"))) == 5
    with pytest.raises(ValueError, match="No percentage type"):
        CA.get_unique_configurations("Cluster_*.xyz", 2.3, working_dir=str(c), perc=None, cum_perc=None, **common)


def test_unmatched_file_is_an_error_before_anything_is_written(z, g, CA, tmp_path):
    files, _ = R.expected_files(z, "C")  # some centres' own molecule failed the filter: their files start elsewhere
    _put(files, tmp_path)
    with pytest.raises(ValueError, match=r"Cluster_0_\d\d\.xyz"):
        CA.get_unique_configurations("Cluster_*.xyz", 2.3, molecules=CR.molecules(g), mol_num=CR.MOL_NUM,
                                     working_dir=str(tmp_path), cum_perc=100)
    assert sorted(os.listdir(str(tmp_path))) == sorted(files)
    for name, data in files.items():
        assert _read(str(tmp_path / name)) == data
    with pytest.raises(ValueError):
        CR.file_census(files, 2.3, CR.molecules(g), CR.MOL_NUM)
