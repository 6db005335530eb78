"""
Plain-numpy restatement of the reference's get_clusters (structural/cluster_analysis.py:47-235): the test oracle of
mdproptools_amd.structural.cluster_analysis. One centre at a time, every step in the reference's arithmetic:

- rsq: d = centre - atom, wrapped once when d > L/2 or d < -L/2 as d - sign(d) L, dx**2 + dy**2 + dz**2
  (rdf_cn.py:36-58); a molecule is in the shell when one of its atoms has rsq < r_cut**2;
- force filter: pandas' compensated sum per molecule (groupby().sum()), min over (Sx, Sy, Sz) times 0.043363 / 16
  against max_force, for the shell's molecules only;
- rows: the centre, the other atoms of its molecule, then the other passing molecules in (type, id) order, each in
  id order; a failing own molecule drops the centre row too (the reference's final inner merge);
- coordinates shifted once relative to the centre (x - sign(x - c) L when |x - c| > L/2);
- text: "{n}\\n\\n" and element\\t%15.10f\\t%15.10f\\t%15.10f per row; files Cluster_{frame}_{centre}.xyz with
  zero-padded counters.

A frame is a dict: ids [N], types [N] (LAMMPS types), xyz [3, N], force [3, N], bounds [3, 2], timestep; rows in
ascending id order.
"""

import os

import numpy as np

FORCE_CONSTANT = 0.043363 / 16.0


def rsq(centre, xyz, lengths):
    d = np.asarray(centre, dtype=np.float64)[:, None] - xyz
    for k in range(3):
        L = lengths[k]
        dk = d[k]
        cond = (dk > L / 2) | (dk < -L / 2)
        dk[cond] = dk[cond] - np.sign(dk[cond]) * L
    return d[0] ** 2 + d[1] ** 2 + d[2] ** 2


def layout(num_mols, num_atoms_per_mol):
    """(mol_of [N], seg_off [M + 1], mol_type [M] 1-based) of the id-ordered molecule layout."""
    sizes = np.repeat(np.asarray(num_atoms_per_mol, dtype=np.int64), np.asarray(num_mols, dtype=np.int64))
    seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    mol_of = np.repeat(np.arange(len(sizes)), sizes)
    mol_type = np.repeat(np.arange(1, len(num_mols) + 1), num_mols)
    return mol_of, seg_off, mol_type


def altered_types(ids, num_mols, num_atoms):
    """rdf_cn.py:197-215, one atom at a time."""
    cut = np.cumsum(np.multiply(num_mols, num_atoms))
    out = []
    for v in np.asarray(ids, dtype=np.float64):
        t = v
        for i, c in enumerate(cut):
            if v <= c:
                t = (v - c) % num_atoms[i]
                if t == 0:
                    t = num_atoms[i]
                t += sum(num_atoms[:i])
                break
        out.append(t)
    return np.array(out)


def kahan_sums(values, seg_off):
    """pandas' group_sum: per segment, y = v - c; t = s + y; c = (t - s) - y; s = t."""
    out = np.zeros(len(seg_off) - 1)
    for m in range(len(out)):
        s = c = 0.0
        for v in values[seg_off[m]:seg_off[m + 1]]:
            y = float(v) - c
            t = s + y
            c = (t - s) - y
            s = t
        out[m] = s
    return out


def shell(xyz, lengths, p, mol_of, r_cut_sq):
    """Ascending molecule indices with an atom within the cutoff of atom p."""
    return np.unique(mol_of[rsq(xyz[:, p], xyz, lengths) < r_cut_sq])


def chunk_straddling_system(rng, n_frames=2, L=(40.0, 41.0, 42.0)):
    """
    A uniform random system of about 4 150 atoms in ragged molecules, built around atom 4096: the first candidate of the
    second chunk of the shell sweep (shell::CHUNK of csrc/shell_search.h). Molecule K owns the atoms 4094..4097, on both
    sides of the chunk edge. Of the 17 centres (one more than a tile), in the last frame, the first (atom 5) is 1.0 and
    0.5 away from atoms 4095 and 4096 of K and 5.0 from the other two; the last (the last atom) is 1.0 away from atom
    4097 and at least 6.5 from the others. With a cutoff of 3, K is a first hit at 4095 and a later hit at 4096, on
    either side of the edge, for the one, and a first hit behind the edge for the other.
    -> (xyz [F, 3, N], box [F, 3], mol_of [N], seg_off [M + 1], centres [17], K)
    """
    sizes = rng.integers(1, 9, 2000)
    sizes = sizes[:np.searchsorted(np.cumsum(sizes), 4094, side="right")]
    sizes = np.concatenate((sizes, [4094 - sizes.sum()] if sizes.sum() < 4094 else [], [4], rng.integers(1, 9, 10)))
    sizes = sizes.astype(np.int64)
    seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    mol_of = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    K = int(mol_of[4094])
    assert seg_off[K] == 4094 and seg_off[K + 1] == 4098
    N = len(mol_of)
    box = np.tile(np.asarray(L, dtype=np.float64), (n_frames, 1))
    xyz = rng.uniform(0, 1, (n_frames, 3, N)) * box[0][None, :, None]
    last = xyz[-1]
    for a, x in ((4094, 10.0), (4095, 14.0), (4096, 14.5), (4097, 20.0), (5, 15.0), (N - 1, 21.0)):
        last[:, a] = [x, 10.0, 10.0]
    others = 6 + rng.choice(4094 - 6, 15, replace=False)
    centres = np.concatenate(([5], others, [N - 1])).astype(np.int32)
    return xyz, box, mol_of, seg_off, centres, K


def padded(i, n):
    return "0" * (len(str(n)) - len(str(i))) + str(i)


def file_name(frame_index, n_frames, centre_index, n_centres):
    return "Cluster_{}_{}.xyz".format(padded(frame_index, n_frames), padded(centre_index, n_centres))


def _lengths(bounds):
    b = np.asarray(bounds, dtype=np.float64)
    return [b[0][1] - b[0][0], b[1][1] - b[1][0], b[2][1] - b[2][0]]


def frame_clusters(fr, atom_type, r_cut, num_mols, num_atoms_per_mol, alter_atom_types=False, max_force=0.75):
    """Per centre (in id order): (centre position, own molecule, passing shell molecules, row positions)."""
    mol_of, seg_off, _ = layout(num_mols, num_atoms_per_mol)
    types = altered_types(fr["ids"], num_mols, num_atoms_per_mol) if alter_atom_types else np.asarray(fr["types"])
    L = _lengths(fr["bounds"])
    force = np.asarray(fr["force"], dtype=np.float64)
    out = []
    for p in np.flatnonzero(types == atom_type):
        own = mol_of[p]
        passing = []
        for m in shell(fr["xyz"], L, p, mol_of, r_cut ** 2):
            sums = [kahan_sums(force[k][seg_off[m]:seg_off[m + 1]], [0, seg_off[m + 1] - seg_off[m]])[0] for k in range(3)]
            if min(sums) * FORCE_CONSTANT < max_force:
                passing.append(int(m))
        rows = []
        if own in passing:
            rows = [p] + [q for q in range(seg_off[own], seg_off[own + 1]) if q != p]
        for m in passing:
            if m != own:
                rows += list(range(seg_off[m], seg_off[m + 1]))
        out.append((int(p), int(own), passing, np.array(rows, dtype=np.int64)))
    return out


def cluster_text(fr, p, rows, element_of):
    L = _lengths(fr["bounds"])
    xyz = np.array(fr["xyz"], dtype=np.float64)[:, rows]
    for k in range(3):
        d = xyz[k] - fr["xyz"][k][p]
        cond = (d > L[k] / 2) | (d < -L[k] / 2)
        xyz[k][cond] = xyz[k][cond] - np.sign(d[cond]) * L[k]
    lines = ["%s\t%15.10f\t%15.10f\t%15.10f\n" % (element_of[q], xyz[0][i], xyz[1][i], xyz[2][i])
             for i, q in enumerate(rows)]
    return "{}\n\n".format(len(rows)) + "".join(lines)


def get_clusters(frames, atom_type, r_cut, num_mols, num_atoms_per_mol, elements, alter_atom_types=False,
                 max_force=0.75):
    """{file name: text} of the selected frames (what get_clusters writes), elements by LAMMPS type."""
    files = {}
    for i, fr in enumerate(frames):
        element_of = [elements[int(t) - 1] for t in fr["types"]]
        cl = frame_clusters(fr, atom_type, r_cut, num_mols, num_atoms_per_mol, alter_atom_types, max_force)
        for c, (p, own, passing, rows) in enumerate(cl):
            files[file_name(i, len(frames), c, len(cl))] = cluster_text(fr, p, rows, element_of)
    return files


def compositions(frames, atom_type, r_cut, num_mols, num_atoms_per_mol, alter_atom_types=False, max_force=0.75):
    """[(frame index, timestep, centre id, (passing molecules of each type other than the centre's own))]."""
    _, _, mol_type = layout(num_mols, num_atoms_per_mol)
    out = []
    for i, fr in enumerate(frames):
        for p, own, passing, rows in frame_clusters(fr, atom_type, r_cut, num_mols, num_atoms_per_mol,
                                                     alter_atom_types, max_force):
            n = [sum(1 for m in passing if m != own and mol_type[m] == t) for t in range(1, len(num_mols) + 1)]
            out.append((i, int(fr["timestep"]), int(fr["ids"][p]), tuple(n)))
    return out


# ---- the fixtures of tests/golden/clusters.npz (tools/make_cluster_golden.py) ----

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clusters.npz")
ELEMENTS = ["O", "C", "H", "N", "S", "O", "C", "F", "Mg"]
NUM_MOLS = [591, 66, 33]
NUM_ATOMS = [16, 15, 1]
DUMP_COLS = ["id", "type", "x", "y", "z", "fx", "fy", "fz"]
# keyword arguments of get_clusters per case; A-C run on frame 50 (a one-frame dump here), D on the sub-system
CASES = {
    "A": dict(atom_type=9, r_cut=2.3, max_force=0.75, alter_atom_types=False),
    "B": dict(atom_type=32, r_cut=2.3, max_force=0.75, alter_atom_types=True),
    "C": dict(atom_type=9, r_cut=2.3, max_force=-0.01, alter_atom_types=False),
    "D": dict(atom_type=9, r_cut=6.0, max_force=0.3, alter_atom_types=False),
}


def load():
    return dict(np.load(GOLDEN))


def expected_files(z, key):
    """{file name: bytes} the reference wrote for case `key`, and its return value."""
    blob, off = z[key + "_blob"].tobytes(), z[key + "_off"]
    return {str(n): blob[off[i]:off[i + 1]] for i, n in enumerate(z[key + "_names"])}, int(z[key + "_return"])


def frames_of(z, key):
    """The frames case `key` processes, and its num_mols."""
    if key != "D":
        n = len(z["f50_id"])
        return [dict(ids=z["f50_id"].astype(np.int64), types=z["f50_type"].astype(np.int64), xyz=z["f50_xyz"],
                     force=z["f50_force"], bounds=z["f50_bounds"], timestep=int(z["f50_timestep"]))], NUM_MOLS
    n = len(z["d_type"])
    return [dict(ids=np.arange(1, n + 1), types=z["d_type"].astype(np.int64), xyz=z["d_xyz"][f],
                 force=z["d_force"][f], bounds=z["d_bounds"][f], timestep=int(z["d_timestep"][f]))
            for f in range(len(z["d_xyz"]))], [int(v) for v in z["d_num_mols"]]


def write_dumps(z, key, directory):
    """The case's frames as LAMMPS dumps (repr round trip: the same doubles parse back); returns the glob pattern
    and the get_clusters arguments (frame, full_trajectory) that select them as the reference's call did."""
    from mdproptools_amd.io import write_dump

    frames, _ = frames_of(z, key)
    for fr in frames:
        tab = np.column_stack([fr["ids"], fr["types"], fr["xyz"].T, fr["force"].T])
        write_dump(os.path.join(directory, "dump.%d.dump" % fr["timestep"]), fr["timestep"], fr["bounds"], DUMP_COLS,
                   tab)
    pattern = os.path.join(directory, "dump.*.dump")
    return pattern, (dict(full_trajectory=True) if key == "D" else dict(full_trajectory=False, frame=0))
