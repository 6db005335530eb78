"""
The numpy restatement of the spatial distribution histograms (tests/sdf_ref.py) and the host layer of
structural/spatial_distribution.py, without a GPU: the restatement is pinned on its own — a lattice with a closed form,
rigid clusters placed in a chosen body frame (handedness and axis order), the edge cases it is later trusted with — so
that a mistake shared with the kernels cannot hide; the drop-in runs on the restatement through `compute=`.
"""
import numpy as np
import pytest

import sdf_ref as R
from mdproptools_amd import backend
from mdproptools_amd.structural.spatial_distribution import calc_spatial_distribution, write_cube


def _cells(h):
    return {tuple(int(v) for v in ix): int(h[tuple(ix)]) for ix in np.argwhere(h)}


# ---- the lattice with a closed form ----

def test_lattice_closed_form():
    xyz, box, _, _ = R.lattice()
    o, p, q = [0], [1], [2]
    mol_of = np.concatenate([[0, 0, 0], 1 + np.arange(61)])
    cand = np.arange(3, 64)
    h, d, n_hits, bad = R.sdf_hist(xyz, box, o, p, q, cand, np.zeros(61, dtype=int), 1, 2.5, 1.0, mol_of=mol_of)
    assert h.shape == (1, 5, 5, 5) and bad == 0 and d.sum() == 0
    assert _cells(h[0]) == {(0, 2, 2): 1, (2, 0, 2): 1, (2, 2, 4): 1, (2, 2, 0): 1}
    assert n_hits.tolist() == [[4]]
    # without exclusion and with the molecule's own atoms observed: p at +x, q at +y
    cand = np.arange(64)
    cls = np.concatenate([[1, 2, 3], np.zeros(61, dtype=int)])
    h, d, n_hits, _ = R.sdf_hist(xyz, box, o, p, q, cand, cls, 4, 2.5, 1.0)
    assert _cells(h[0]) == {(0, 2, 2): 1, (2, 0, 2): 1, (2, 2, 4): 1, (2, 2, 0): 1}
    assert _cells(h[2]) == {(4, 2, 2): 1} and _cells(h[3]) == {(2, 4, 2): 1}
    assert h[1].sum() == 0 and n_hits.tolist() == [[6]]  # (the origin atom itself is never a hit)


def test_lattice_through_the_dropin(tmp_path):
    xyz, box, num_mols, num_atoms = R.lattice()
    pattern = R.write_dumps(xyz, box, str(tmp_path))
    out = tmp_path / "sdf.npz"
    sdf, counts, axes, summary = calc_spatial_distribution(2.5, 1.0, (1, 1, 2, 3), [4], pattern, num_mols, num_atoms,
                                                           path_or_buff=str(out), cube=True, compute=R.sdf_hist)
    assert counts.dtype == np.int64 and sdf.dtype == np.float64 and counts.shape == (1, 5, 5, 5)
    assert _cells(counts[0]) == {(0, 2, 2): 1, (2, 0, 2): 1, (2, 2, 4): 1, (2, 2, 0): 1}
    assert np.array_equal(axes, [-2.0, -1.0, 0.0, 1.0, 2.0])
    assert sdf[0, 0, 2, 2] == 1.0 / (1 * 1.0 ** 3 * (61 / 512.0))  # one valid row, rho = 61 atoms in 8**3
    assert list(summary.columns) == ["species", "n_hits", "n_degenerate", "max_g", "hits_per_centre_frame"]
    assert summary.iloc[0].tolist() == [4, 4, 0, 512.0 / 61, 4.0]
    z = np.load(str(out))
    assert sorted(z.files) == ["axes", "counts", "n_degenerate", "n_valid_rows", "sdf", "species"]
    assert np.array_equal(z["counts"], counts) and int(z["n_valid_rows"]) == 1 and z["species"].tolist() == [4]
    # the cube file: two comment lines, atom count and origin (Bohr), three voxel vectors, the dummy atom, the values
    lines = (tmp_path / "sdf_4.cube").read_text().splitlines()
    bohr = 0.529177210903
    head = [ln.split() for ln in lines[2:7]]
    assert int(head[0][0]) == 1 and np.allclose([float(v) for v in head[0][1:]], [-2.0 / bohr] * 3, atol=1e-6)
    for k in range(3):
        assert int(head[1 + k][0]) == 5
        assert np.allclose([float(v) for v in head[1 + k][1:]], np.eye(3)[k] / bohr, atol=1e-6)
    assert [float(v) for v in head[4]] == [0.0] * 5
    vals = np.array([float(v) for ln in lines[7:] for v in ln.split()]).reshape(5, 5, 5)
    assert np.allclose(vals, sdf[0], rtol=1e-5)
    # the molecule's own atoms under observation, exclusion off: (4,2,2) and (2,4,2)
    _, counts, _, summary = calc_spatial_distribution(2.5, 1.0, (1, 1, 2, 3), [4, 2, 3], pattern, num_mols, num_atoms,
                                                      exclude_same_molecule=False, save_mode=False, compute=R.sdf_hist)
    assert _cells(counts[1]) == {(4, 2, 2): 1} and _cells(counts[2]) == {(2, 4, 2): 1}
    assert summary["n_hits"].tolist() == [4, 1, 1]


# ---- handedness and axis order, independent of the restatement's own algebra ----

CHOSEN = {(5, 3, 3): (2.0, 0.0, 0.0),     # +x
          (4, 5, 3): (1.0, 2.0, 0.0),     # +x +y
          (3, 3, 5): (0.0, 0.0, 2.0),     # +z only
          (3, 2, 1): (0.0, -1.0, -2.0)}   # -y -z


def handed_cluster(seed, points=None):
    """The chosen cells' centres (r_cut 3.5, bin_size 1: G = 7, cell i is centred at i - 3) as observed points around
    the molecule, rotated, moved so that the cluster's bounding box is centred on a corner of the box, and wrapped: it
    straddles all three faces."""
    rng = np.random.default_rng(seed)
    box = np.array([11.0, 12.0, 13.0])
    rot = R.random_rotation(rng)
    assert np.allclose(rot @ rot.T, np.eye(3)) and np.linalg.det(rot) > 0.99
    points = list(CHOSEN.values()) if points is None else points
    lab = np.concatenate([R.MOLECULE, np.asarray(points)]) @ rot.T
    xyz = R.rigid_cluster(points, rot, -0.5 * (lab.min(axis=0) + lab.max(axis=0)), box)
    assert all(((xyz[0, k] > box[k] / 2).any() and (xyz[0, k] < box[k] / 2).any()) for k in range(3))
    return xyz, box[None, :]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_handedness_and_axis_order(seed):
    xyz, box = handed_cluster(seed)
    h, d, n_hits, bad = R.sdf_hist(xyz, box, [0], [1], [2], np.arange(3, 7), np.zeros(4, dtype=int), 1, 3.5, 1.0)
    assert bad == 0 and d.sum() == 0 and n_hits.tolist() == [[4]]
    assert _cells(h[0]) == {cell: 1 for cell in CHOSEN}
    # a reflected cluster (left-handed placement) must NOT give the chosen cells: the z entries change sides
    xyz, box = handed_cluster(seed, [(x, y, -z) for x, y, z in CHOSEN.values()])
    h, _, _, _ = R.sdf_hist(xyz, box, [0], [1], [2], np.arange(3, 7), np.zeros(4, dtype=int), 1, 3.5, 1.0)
    assert _cells(h[0]) == {(5, 3, 3): 1, (4, 5, 3): 1, (3, 3, 1): 1, (3, 2, 5): 1}


# ---- the edge system the GPU tests rely on ----

def test_edge_system_holds_its_edges():
    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(1, 240)
    rc, bs, M = R.EDGE_R_CUT, R.EDGE_BIN, R.EDGE_MOLS
    G = R.grid(rc, bs)
    assert G == 8
    e, valid = R.body_frames(xyz, box, o, p, q)
    assert np.array_equal(e[0, 0], np.eye(3)) and valid[0].tolist() == [True] * 6 + [False, False] + [True] * 2
    f, c = xyz[0], lambda i: 3 * M + i  # noqa: E731
    assert float(((f[:, c(0)] - f[:, 0]) ** 2).sum()) == rc * rc                 # exactly r_cut ...
    assert (f[0, c(1)] - f[0, 0] + rc) / bs == 5.0                               # exactly on the edge of cell 5
    assert f[2, c(2)] - f[2, 3] == 0.5 * box[0, 2] and f[2, c(3)] - f[2, 6] == -0.5 * box[0, 2]
    x = f[0, c(7)] - f[0, 12]
    assert x * x < rc * rc and (x + rc) / bs == G                                # in the shell, and clamped

    def one(centre, atom):  # the cells of candidate `atom` alone around molecule `centre`
        h, d, nh, _ = R.sdf_hist(xyz[:1], box[:1], o[centre:centre + 1], p[centre:centre + 1], q[centre:centre + 1],
                                 [atom], [0], 1, rc, bs)
        return _cells(h[0]), int(d[0]), int(nh[0, 0])

    assert one(0, c(0)) == ({}, 0, 0)                                            # ... is out
    assert one(0, c(1)) == ({(5, 4, 4): 1}, 0, 1)
    assert one(1, c(2)) == ({(4, 4, 7): 1}, 0, 1) and one(2, c(3)) == ({(4, 4, 0): 1}, 0, 1)  # +L/2, -L/2: not wrapped
    assert one(3, c(4)) == ({(3, 4, 4): 1}, 0, 1) and one(3, c(5)) == ({(4, 3, 4): 1}, 0, 1)
    assert one(3, c(6)) == ({(4, 4, 3): 1}, 0, 1)                                # across each boundary
    assert one(4, c(7)) == ({(7, 4, 4): 1}, 0, 1)                                # the clamp
    assert one(5, c(8)) == ({(4, 4, 4): 1}, 0, 1)                                # on the origin atom: the central cell
    assert one(6, c(9)) == ({}, 1, 1) and one(6, c(10)) == ({}, 1, 1)            # degenerate rows: counted, not binned
    assert one(7, c(11)) == ({}, 1, 1) and one(7, c(12)) == ({}, 1, 1)
    assert one(5, 3 * 5) == ({}, 0, 0)                                           # the origin atom is no hit of itself
    h, d, nh, bad = R.sdf_hist(xyz, box, o, p, q, cand, cls, 3, rc, bs, mol_of=mol_of)
    assert bad == 2 and d.sum() >= 4 and h.sum() + d.sum() == nh.sum() and (h.sum(axis=(1, 2, 3)) > 0).all()


def test_nonfinite_input_stays_home():
    xyz, box, o, p, q, cand, cls, mol_of = R.edge_system(2, 240)
    rc, bs = R.EDGE_R_CUT, R.EDGE_BIN
    clean = R.sdf_hist(xyz, box, o, p, q, cand, cls, 3, rc, bs)
    for value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[1, 0, cand[5]] = value           # a candidate
        bad[1, 1, o[8]] = value              # o of molecule 8: no hits
        bad[0, 2, p[9]] = value              # p of molecule 9: a degenerate row
        h, d, nh, rows = R.sdf_hist(bad, box, o, p, q, cand, cls, 3, rc, bs)
        assert nh[1, 8] == 0 and rows == clean[3] + 2  # (a non-finite o leaves no finite a or b either)
        touched = np.zeros_like(nh, dtype=bool)
        touched[1, :] = True                 # (the candidate may have been a hit of any row of frame 1)
        touched[0, 9] = True
        assert np.array_equal(nh[~touched], clean[2][~touched])
        assert np.array_equal(nh[0, 9], clean[2][0, 9])  # a degenerate row keeps its hits
        assert h.sum() + d.sum() == nh.sum()


# ---- the host layer ----

def test_argument_checks(tmp_path):
    xyz, box, num_mols, num_atoms = R.lattice()
    pattern = R.write_dumps(xyz, box, str(tmp_path))

    def call(reference=(1, 1, 2, 3), observed=(4,), r_cut=2.5, bin_size=1.0, **kw):
        return calc_spatial_distribution(r_cut, bin_size, reference, list(observed), pattern, num_mols, num_atoms,
                                         save_mode=False, compute=R.sdf_hist, **kw)

    with pytest.raises(ValueError, match="reference must be \\(mol_type, origin, x_atom, xy_atom\\)"):
        call(reference=(1, 1, 2))
    with pytest.raises(ValueError, match="three distinct atoms"):
        call(reference=(1, 1, 2, 2))
    with pytest.raises(ValueError, match="reference atom 4: molecule type 1 has 3 atoms"):
        call(reference=(1, 1, 2, 4))
    with pytest.raises(ValueError, match="reference atom 0"):
        call(reference=(1, 0, 2, 3))
    with pytest.raises(ValueError, match="molecule type 3: the layout has 2"):
        call(reference=(3, 1, 2, 3))
    with pytest.raises(ValueError, match="at most 8 observed species per call \\(9 given\\)"):
        call(observed=range(1, 10))
    with pytest.raises(ValueError, match="distinct atom types"):
        call(observed=(4, 4))
    with pytest.raises(ValueError, match="at most 256 cells per axis and 33554432 cells per call"):
        call(bin_size=5.0 / 257)
    with pytest.raises(ValueError, match="8 species x 162\\*\\*3 cells"):
        call(observed=range(1, 9), r_cut=81.0, bin_size=1.0)
    with pytest.raises(ValueError, match="positive and finite"):
        call(bin_size=0.0)
    assert backend.SDF_MAX_SPECIES == 8 and backend.SDF_MAX_GRID == 256 and backend.SDF_MAX_CELLS == 2 ** 25
    assert backend.sdf_grid(2.5, 1.0) == 5 and backend.sdf_grid(3.5, 0.875) == 8 == R.grid(3.5, 0.875)


def test_cube_header(tmp_path):
    grid = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    grid[1, 1, 1] = np.nan  # (written as 0)
    write_cube(str(tmp_path / "g.cube"), grid, 3.0, 2.0, "title line")
    lines = (tmp_path / "g.cube").read_text().splitlines()
    assert lines[0] == "title line" and len(lines) == 7 + 9
    assert lines[2].split()[0] == "1" and lines[6].split()[0] == "0"
    vals = np.array([float(v) for ln in lines[7:] for v in ln.split()]).reshape(3, 3, 3)
    assert vals[2, 1, 0] == 21.0 and vals[0, 0, 2] == 2.0 and vals[1, 1, 1] == 0.0  # e1 outermost, e3 innermost


def test_uniform_gas_normalises_to_one(tmp_path):
    """20 000 observed atoms at random and 40 reference molecules in a box of 30: the mean g over the cells wholly
    inside the sphere is 1 within 5 % (about 13 000 counts there: a relative spread near 1 %). A sanity bound on the
    rho_s formula, through the drop-in on written dumps with the restatement as `compute`."""
    rng = np.random.default_rng(20000)
    n_ref, n_obs, L, rc, bs = 40, 20000, 30.0, 6.0, 1.5
    xyz = rng.uniform(0, L, (1, 3, 3 * n_ref + n_obs))
    for k in (1, 2):
        xyz[0, :, k:3 * n_ref:3] = xyz[0, :, 0:3 * n_ref:3] + rng.uniform(-1, 1, (3, n_ref))
    pattern = R.write_dumps(xyz, np.full((1, 3), L), str(tmp_path))
    sdf, counts, axes, summary = calc_spatial_distribution(rc, bs, (1, 1, 2, 3), [4], pattern, [n_ref, n_obs], [3, 1],
                                                           save_mode=False, compute=R.sdf_hist)
    far = np.abs(axes) + 0.5 * bs  # the far face of every cell, per axis
    inside = (far[:, None, None] ** 2 + far[None, :, None] ** 2 + far[None, None, :] ** 2) < rc * rc
    assert inside.sum() >= 100 and counts[0][inside].sum() > 10000
    mean_g = float(sdf[0][inside].mean())
    print("mean g inside:", mean_g, "cells:", int(inside.sum()), "counts:", int(counts[0][inside].sum()))
    assert abs(mean_g - 1.0) < 0.05
    want = R.normalise(counts, 40, bs, [n_obs], np.full((1, 3), L))
    assert np.array_equal(sdf, want)
    assert summary["hits_per_centre_frame"].iloc[0] == counts.sum() / 40
