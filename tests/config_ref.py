"""
Plain-numpy restatement of the configuration census (get_unique_configurations, structural/cluster_analysis.py:238-457
of the reference): the test oracle of mdproptools_amd.structural.cluster_analysis' two routes.

- file census, the reference's rules on the text of the cluster files: the atoms other than the first at
  Euclidean distance <= r_cut of it (pymatgen's get_neighbors), optionally of the given elements; the first
  len(molecules[mol_num]) atoms skipped; the rest matched greedily against the molecules' element sequences in list
  order; per molecule the count of every first character of its coordinating elements, written count then letter
  over ascending letters; per type the sorted strings joined with ":";
- direct census, from the frames: cluster_ref.frame_clusters gives every centre's passing shell molecules, and per
  molecule other than the centre's own the atoms with cluster_ref.rsq < r_coord**2 (strict) are counted the same way;
- tables: the distinct rows counted by hand, ordered by count with pandas' default sort (its tie order is what the
  recorded CSVs hold), %, the top selection and one sample per distinct atoms_* key.

Recorded answers: tests/golden/configurations.npz (tools/make_configuration_golden.py), the real reference run on the
files of tests/golden/clusters.npz.
"""

import os
import warnings
from collections import Counter

import numpy as np
import pandas as pd

import cluster_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configurations.npz")
CSVS = ["clusters", "configurations", "top_conf"]
MOL_NUM = 2  # the centres are Mg ions: molecules [dme, tfsi, mg]
# per case: the cluster case of clusters.npz whose files / dumps it runs on, and the census arguments
CASES = {
    "B": dict(files="B", r_cut=2.3, type_coord_atoms=["O", "N", "Mg"], find_top=True, perc=None, cum_perc=100,
              mol_names=["dme", "tfsi", "mg"]),
    "A": dict(files="A", r_cut=2.3, type_coord_atoms=None, find_top=False),
    "D1": dict(files="D", r_cut=2.3, type_coord_atoms=["O", "N", "Mg"], find_top=False),
    "D2": dict(files="D", r_cut=3.5, type_coord_atoms=["O", "F"], find_top=True, perc=5, cum_perc=None),
    "D3": dict(files="D", r_cut=6.0, type_coord_atoms=None, find_top=False),
}


def load():
    return dict(np.load(GOLDEN))


def molecules(g):
    """[dme, tfsi, mg] as lists of element strings."""
    return [str(s).split() for s in g["molecules"]]


def recorded(g, key):
    """({csv name: bytes} the reference wrote for the case, [cluster file copied to conf_1.xyz, conf_2.xyz, ...])."""
    return ({n: g["%s_%s" % (key, n)].tobytes() for n in CSVS if "%s_%s" % (key, n) in g},
            [str(n) for n in g[key + "_picks"]])


def census_kwargs(key):
    kw = dict(CASES[key])
    kw.pop("files")
    return kw


def parse_xyz(data):
    lines = data.decode().split("\n")
    n = int(lines[0])
    rows = [ln.split() for ln in lines[2:2 + n]]
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows]).reshape(n, 3)


def site_string(elements):
    """'1N2O' for N, O, O: how often every first letter occurs, letters ascending."""
    firsts = [e[:1] for e in elements]
    return "".join("%d%s" % (firsts.count(ch), ch) for ch in sorted(set(firsts)))


def shell_gaps(files, r_cut):
    """|distance - r_cut| of every atom of every file to the file's first atom."""
    out = []
    for data in files.values():
        els, xyz = parse_xyz(data)
        if len(els):
            out.append(np.abs(np.linalg.norm(xyz - xyz[0], axis=1) - r_cut))
    return np.concatenate(out)


def file_census(files, r_cut, sequences, mol_num, type_coord_atoms=None):
    """
    [(file name, [molecules per type], [atoms string per type])] in name order; ValueError naming a file whose atoms
    spell none of `sequences` (element lists, one per molecule type) at some position.
    """
    out = []
    for name in sorted(files):
        els, xyz = parse_xyz(files[name])
        own = len(sequences[mol_num])  # the atom of interest comes first, in its own molecule
        counted = set()
        for i in range(1, len(els)):
            dist = float(np.sqrt(((xyz[i] - xyz[0]) ** 2).sum()))
            if dist <= r_cut and (not type_coord_atoms or els[i] in type_coord_atoms):
                counted.add(i)
        per_type = [[] for _ in sequences]
        pos = own
        while pos < len(els):
            fits = [t for t, seq in enumerate(sequences) if els[pos:pos + len(seq)] == seq]
            if not fits:
                raise ValueError(name)
            t = fits[0]
            span = range(pos, pos + len(sequences[t]))
            per_type[t].append(site_string([els[i] for i in span if i in counted]))
            pos = span.stop
        out.append((name, [len(v) for v in per_type], [":".join(sorted(v)) for v in per_type]))
    return out


def direct_census(frames, num_mols, cluster_kw, r_coord, element_of_type, type_coord_atoms=None):
    """The same rows from the frames (cluster_kw: the get_clusters arguments of cluster_ref.CASES)."""
    mol_of, seg_off, mol_type = R.layout(num_mols, R.NUM_ATOMS)
    out = []
    for i, fr in enumerate(frames):
        els = [element_of_type[int(t) - 1] for t in fr["types"]]
        L = R._lengths(fr["bounds"])
        cl = R.frame_clusters(fr, num_mols=num_mols, num_atoms_per_mol=R.NUM_ATOMS, **cluster_kw)
        for c, (p, own, passing, rows) in enumerate(cl):
            rsq = R.rsq(fr["xyz"][:, p], fr["xyz"], L)
            sites = {t: [] for t in range(len(num_mols))}
            for m in passing:
                if m == own:
                    continue
                hit = [els[b] for b in range(seg_off[m], seg_off[m + 1])
                       if rsq[b] < r_coord ** 2 and (not type_coord_atoms or els[b] in type_coord_atoms)]
                sites[mol_type[m] - 1].append(hit)
            out.append((R.file_name(i, len(frames), c, len(cl)), [len(sites[k]) for k in sites],
                        [":".join(sorted(site_string(s) for s in sites[k])) for k in sites]))
    return out


def tables(rows, n_types, mol_names=None, find_top=True, perc=None, cum_perc=90):
    """
    (clusters, configurations, top configurations or None) of census rows, by hand: the distinct (num, atoms) keys in
    ascending order with their counts, put in descending count order by pandas' default sort (the one step whose tie
    order is pandas' own), the share in %; the top rows by running share <= cum_perc, else by share >= perc; per
    distinct atoms key of the top rows its first row, with the first cluster in name order that shows those atoms.
    """
    labels = list(mol_names) if mol_names else [str(i + 1) for i in range(n_types)]
    num_cols, atoms_cols = ["num_" + n for n in labels], ["atoms_" + n for n in labels]
    rows = sorted(rows, key=lambda r: r[0])
    clusters = pd.DataFrame([[r[0]] + list(r[1]) + list(r[2]) for r in rows], columns=["cluster"] + num_cols + atoms_cols)
    tally = Counter((tuple(r[1]), tuple(r[2])) for r in rows)
    keys = sorted(tally)
    conf = pd.DataFrame([list(k[0]) + list(k[1]) + [tally[k]] for k in keys], columns=num_cols + atoms_cols + ["count"])
    conf = conf.sort_values("count", ascending=False)
    conf["%"] = [c * 100 / len(rows) for c in conf["count"]]
    if not find_top:
        return clusters, conf, None
    if cum_perc and perc:
        warnings.warn("Two percentage types are provided for determining the top configurations; using cum_perc")
    if not cum_perc and not perc:
        raise ValueError("No percentage type is provided for determining the top configurations")
    running, picked, seen = 0.0, [], set()
    for pos, (_, r) in enumerate(conf.iterrows()):
        running += r["%"]
        if (running <= cum_perc) if cum_perc else (r["%"] >= perc):
            key = tuple(r[c] for c in atoms_cols)
            if key not in seen:
                seen.add(key)
                picked.append((pos, next(row[0] for row in rows if tuple(row[2]) == key)))
    top = conf.iloc[[p for p, _ in picked]].copy()
    top["cluster"] = [n for _, n in picked]
    return clusters, conf, top


def csv_bytes(df):
    return df.to_csv(index=False).encode()


def case_tables(key, rows):
    kw = census_kwargs(key)
    return tables(rows, 3, kw.get("mol_names"), kw["find_top"], kw.get("perc"), kw.get("cum_perc", 90))


def coordination_rows(xyz, box, centres, mol_of, seg_off, mol_type, cls, r_shell_sq, r_coord_sq, passes=None):
    """
    What backend.shell_coordination returns, one centre at a time: per (frame, centre) the list of (molecule, word)
    in (type, word, molecule) order — the passing molecules other than the centre's own with an atom at
    rsq < r_shell_sq, word = sum of 1 << (8 * cls[b]) over their atoms b with cls[b] != 255 and rsq < r_coord_sq.
    """
    out = []
    for f in range(len(xyz)):
        row_f = []
        for p in centres:
            rsq = R.rsq(xyz[f][:, p], xyz[f], box[f])
            ent = []
            for m in np.unique(mol_of[rsq < r_shell_sq]):
                if m == mol_of[p] or (passes is not None and not passes[f, m]):
                    continue
                word = 0
                for b in range(seg_off[m], seg_off[m + 1]):
                    if cls[b] != 0xFF and rsq[b] < r_coord_sq:
                        word += 1 << (8 * int(cls[b]))
                ent.append((int(mol_type[m]), word, int(m)))
            row_f.append([(m, w) for _, w, m in sorted(ent)])
        out.append(row_f)
    return out
