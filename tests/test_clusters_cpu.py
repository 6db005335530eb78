"""
get_clusters without a GPU: the numpy restatement (tests/cluster_ref.py) reproduces every case the reference recorded
in tests/golden/clusters.npz byte for byte, and the drop-in's signature, file naming and error match the reference's.
"""
import inspect
import os

import numpy as np
import pytest

import cluster_ref as R


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.mark.parametrize("key", sorted(R.CASES))
def test_restatement_reproduces_reference(z, key):
    want, n = R.expected_files(z, key)
    frames, num_mols = R.frames_of(z, key)
    got = R.get_clusters(frames, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, elements=R.ELEMENTS, **R.CASES[key])
    assert len(got) == n == len(want)
    assert {k: v.encode() for k, v in got.items()} == want


def test_cases_cover_the_filter_and_padding(z):
    """C drops centres whose own molecule fails (6 files have no Mg row); D pads frame numbers to two digits."""
    files, _ = R.expected_files(z, "C")
    assert sum(1 for t in files.values() if b"\nMg\t" not in t) == 6
    files, _ = R.expected_files(z, "D")
    assert len(z["d_xyz"]) >= 11 and all(k.startswith("Cluster_") and len(k.split("_")[1]) == 2 for k in files)


def test_force_sums_are_the_compensated_sums(z):
    """The compensated per-molecule sums differ from plain sequential sums on frame 50 (why the kernel keeps them)."""
    _, seg_off, _ = R.layout(R.NUM_MOLS, R.NUM_ATOMS)
    fx = z["f50_force"][0]
    k = R.kahan_sums(fx, seg_off)
    plain = np.array([sum(float(v) for v in fx[a:b]) for a, b in zip(seg_off[:-1], seg_off[1:])])
    assert (k != plain).any()


def test_signature_matches_reference():
    from mdproptools_amd.structural import cluster_analysis as CA

    sig = inspect.signature(CA.get_clusters)
    want = [("filename", inspect.Parameter.empty), ("atom_type", inspect.Parameter.empty),
            ("r_cut", inspect.Parameter.empty), ("num_mols", inspect.Parameter.empty),
            ("num_atoms_per_mol", inspect.Parameter.empty), ("full_trajectory", False), ("frame", None),
            ("elements", None), ("alter_atom_types", False), ("max_force", 0.75), ("working_dir", None)]
    assert [(p.name, p.default) for p in sig.parameters.values()] == want
    assert CA.FORCE_CONSTANT == 0.043363 / 16.0


@pytest.mark.parametrize("args,name", [((0, 1, 0, 33), "Cluster_0_00.xyz"), ((3, 12, 7, 5), "Cluster_03_7.xyz"),
                                       ((11, 12, 32, 33), "Cluster_11_32.xyz"), ((5, 100, 9, 10), "Cluster_005_09.xyz"),
                                       ((0, 1, 0, 100), "Cluster_0_000.xyz"), ((10, 10, 0, 1), "Cluster_10_0.xyz")])
def test_file_names(args, name):
    from mdproptools_amd.structural import cluster_analysis as CA

    assert CA.cluster_file_name(*args) == name == R.file_name(*args)


def test_missing_elements_raise(z, tmp_path):
    from mdproptools_amd.structural import cluster_analysis as CA

    pattern, sel = R.write_dumps(z, "A", str(tmp_path))
    with pytest.raises(ValueError, match="The elements of the atoms in the system should be provided if they are "
                                         "not in the dump files."):
        CA.get_clusters(pattern, 9, 2.3, R.NUM_MOLS, R.NUM_ATOMS, working_dir=str(tmp_path), **sel)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("Cluster_")]
