#!/usr/bin/env python
"""
tools/make_configuration_golden.py — tests/golden/configurations.npz from the REAL reference's
get_unique_configurations, run on the cluster files already recorded in tests/golden/clusters.npz.

Build container only (the reference is not on the GPU box; what travels is this script's output, as data):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_configuration_golden.py

The reference is imported read-only with the stand-ins of oracle/shims (oracle/shims/README.md). Upstream builds the
census on pymatgen's Molecule, which is not installed: after the import, the name `Molecule` of the reference's module
is bound to the small stand-in below (xyz parsing, indexing, .species, get_neighbors as dist <= r without the site
itself, site equality, species_string — what pymatgen documents for them). Two more names of that module are bound for
a reproducible record: `glob` to a sorted glob (with find_top=False the reference leaves the clusters in the directory's
own listing order, which is the file system's business) and `tqdm` to the identity.

Cases (files of clusters.npz; molecules [dme, tfsi, mg] as element lists, mol_num 2, zip=False):
  B   case B, r_cut 2.3, ["O", "N", "Mg"], cum_perc=100, mol_names dme/tfsi/mg (upstream test_get_unique_configurations)
  A   case A, r_cut 2.3, no element filter, no top selection
  D1  case D, r_cut 2.3, ["O", "N", "Mg"], no top selection
  D2  case D, r_cut 3.5, ["O", "F"], perc=5, cum_perc=None
  D3  case D, r_cut 6.0, no element filter, no top selection (Mg counts under the letter M)
Case C is never run: the reference does not terminate on a file whose own molecule failed the force filter.

Before anything is saved, case B's three CSVs are checked against the sha256 oids and sizes of upstream's git-LFS
pointer files (tests/structural/test_files/{clusters,configurations,top_conf}.csv) and its conf picks against
upstream's committed conf_*.xyz.
"""

import glob
import hashlib
import os
import re
import sys
import tempfile

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
sys.path[:0] = [os.path.join(REPO, "oracle", "shims"), REPO, os.path.join(REPO, "tests"), REF]

import numpy as np  # noqa: E402

import mdproptools.structural.cluster_analysis as ref_mod  # noqa: E402

import cluster_ref  # noqa: E402  (tests/cluster_ref.py: the recorded cluster files)

UPSTREAM = os.path.join(REF, "tests", "structural", "test_files")
OUT = os.environ.get("MDHIP_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden", "configurations.npz")
CSVS = ["clusters", "configurations", "top_conf"]
CASES = {
    "B": dict(files="B", r_cut=2.3, type_coord_atoms=["O", "N", "Mg"], find_top=True, perc=None, cum_perc=100,
              mol_names=["dme", "tfsi", "mg"]),
    "A": dict(files="A", r_cut=2.3, type_coord_atoms=None, find_top=False),
    "D1": dict(files="D", r_cut=2.3, type_coord_atoms=["O", "N", "Mg"], find_top=False),
    "D2": dict(files="D", r_cut=3.5, type_coord_atoms=["O", "F"], find_top=True, perc=5, cum_perc=None),
    "D3": dict(files="D", r_cut=6.0, type_coord_atoms=None, find_top=False),
}


class Site:
    def __init__(self, species_string, coords):
        self.species_string = species_string
        self.coords = coords

    def __eq__(self, other):
        return self.species_string == other.species_string and bool(np.allclose(self.coords, other.coords, atol=1e-5))

    __hash__ = None


class Molecule:
    """What the reference's census asks of pymatgen's Molecule, for xyz files."""

    def __init__(self, sites):
        self.sites = sites

    @classmethod
    def from_file(cls, path):
        with open(path) as fh:
            lines = fh.read().split("\n")
        n = int(lines[0])
        sites = []
        for ln in lines[2:2 + n]:
            el, x, y, z = ln.split()
            sites.append(Site(el, np.array([float(x), float(y), float(z)])))
        return cls(sites)

    def __getitem__(self, i):
        return self.sites[i]

    def __len__(self):
        return len(self.sites)

    @property
    def species(self):
        return [s.species_string for s in self.sites]

    def get_neighbors(self, site, r):
        return [s for s in self.sites if np.linalg.norm(s.coords - site.coords) <= r and s != site]


def sorted_glob(pattern):
    return sorted(glob.glob(pattern))


class _SortedGlob:
    glob = staticmethod(sorted_glob)


def pointer(name):
    with open(os.path.join(UPSTREAM, name + ".csv")) as fh:
        text = fh.read()
    return re.search(r"oid sha256:([0-9a-f]{64})", text).group(1), int(re.search(r"size (\d+)", text).group(1))


def run_ref(files, molecules, **kw):
    with tempfile.TemporaryDirectory() as wd:
        for name, data in files.items():
            with open(os.path.join(wd, name), "wb") as fh:
                fh.write(data)
        ref_mod.get_unique_configurations(cluster_pattern="Cluster_*.xyz", molecules=molecules, mol_num=2,
                                          working_dir=wd, zip=False, **kw)
        out = {}
        for name in CSVS:
            p = os.path.join(wd, name + ".csv")
            if os.path.exists(p):
                with open(p, "rb") as fh:
                    out[name] = fh.read()
        picks = []
        for p in sorted(glob.glob(os.path.join(wd, "conf_*.xyz")), key=lambda s: int(re.findall(r"conf_(\d+)", s)[-1])):
            with open(p, "rb") as fh:
                data = fh.read()
            same = [n for n in sorted(files) if files[n] == data]
            picks.append((same, data))
    return out, picks


def main():
    ref_mod.Molecule = Molecule
    ref_mod.glob = _SortedGlob
    ref_mod.tqdm = lambda it, **kw: it

    z = cluster_ref.load()
    _, seg_off, _ = cluster_ref.layout(cluster_ref.NUM_MOLS, cluster_ref.NUM_ATOMS)
    first = np.concatenate(([0], np.cumsum(cluster_ref.NUM_MOLS)[:-1]))  # the first molecule of every type
    species = [[cluster_ref.ELEMENTS[int(t) - 1] for t in z["f50_type"][seg_off[m]:seg_off[m + 1]]] for m in first]
    molecules = [Molecule([Site(s, np.zeros(3)) for s in sp]) for sp in species]

    store = {"molecules": np.array([" ".join(sp) for sp in species])}
    for key, case in CASES.items():
        kw = dict(case)
        files, _ = cluster_ref.expected_files(z, kw.pop("files"))
        csvs, picks = run_ref(files, molecules, **kw)
        assert ("top_conf" in csvs) == case["find_top"] and bool(picks) == case["find_top"], key
        names = []
        for k, (same, data) in enumerate(picks):
            # the sample is the first cluster in name order with the configuration: two clusters never hold equal text
            assert len(same) == 1, (key, k, same)
            names.append(same[0])
        if key == "B":
            for name in CSVS:
                oid, size = pointer(name)
                got = hashlib.sha256(csvs[name]).hexdigest()
                assert (got, len(csvs[name])) == (oid, size), "case B %s.csv: %s, %d bytes; upstream %s, %d" % (
                    name, got, len(csvs[name]), oid, size)
            for k, (_, data) in enumerate(picks):
                with open(os.path.join(UPSTREAM, "conf_%d.xyz" % (k + 1)), "rb") as fh:
                    assert fh.read() == data, "case B conf_%d.xyz differs from upstream's" % (k + 1)
            assert len(picks) == len(glob.glob(os.path.join(UPSTREAM, "conf_*.xyz")))
        for name, data in csvs.items():
            store["%s_%s" % (key, name)] = np.frombuffer(data, dtype=np.uint8)
        store[key + "_picks"] = np.array(names, dtype=str)
    store["upstream_oid"] = np.array([pointer(n)[0] for n in CSVS])
    store["upstream_size"] = np.array([pointer(n)[1] for n in CSVS], dtype=np.int64)

    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {k: list(store[k + "_picks"]) for k in CASES})


if __name__ == "__main__":
    main()
