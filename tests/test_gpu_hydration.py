"""
get_hydration_number / calc_hydration_orientation and their kernels (csrc/hydration.hip) on the GPU: the reference's
CSV and DataFrame bit for bit on every recorded case, and both modes against the numpy restatement
(tests/hydration_ref.py) on randomised systems built to hit every edge (rsq == r_cut**2 exactly, d == +-L/2 exactly, a
water across the boundary, an ion on an O, a cosine of exactly -0.72, ion counts off the tile width, overflowing rows,
device input, more than 65 535 frames), over more than 10**6 cosines.
"""
import itertools
import os

import numpy as np
import pytest

import hydration_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def H():
    from mdproptools_amd.structural import hydration_number

    return hydration_number


@pytest.mark.parametrize("key", sorted(R.CASES))
def test_dropin_csv_and_frame(z, H, key, tmp_path):
    frames, kw = R.case_args(z, key)
    pattern = R.write_dumps(frames, str(tmp_path))
    if str(z[key + "_error"]):
        with pytest.raises(ZeroDivisionError):
            H.get_hydration_number(pattern, working_dir=str(tmp_path), **kw)
        assert not os.path.exists(tmp_path / "angles_df.csv")
        return
    df = H.get_hydration_number(pattern, working_dir=str(tmp_path), **kw)
    assert (tmp_path / "angles_df.csv").read_bytes() == z[key + "_csv"].tobytes()
    assert list(df.columns) == ["angles_distribution", "hydration_factor"]
    assert df["angles_distribution"].to_numpy().tobytes() == z[key + "_cos"].tobytes()
    assert df["hydration_factor"].iloc[0] == z[key + "_factor"]


def _exact_cos_pair():
    """Integer d (|d|**2 < 12.25) and v whose cosine, in the reference's arithmetic, is exactly the double -0.72."""
    r = np.arange(-30, 31, dtype=np.float64)
    V = np.stack(np.meshgrid(r, r, r, indexing="ij")).reshape(3, -1)
    n2 = np.sqrt((V[0] * V[0] + V[1] * V[1]) + V[2] * V[2])
    for d in itertools.product(range(-3, 4), repeat=3):
        d = np.array(d, dtype=np.float64)
        if (d * d).sum() >= 12.25:
            continue
        with np.errstate(all="ignore"):
            c = (((0.0 + d[0] * V[0]) + d[1] * V[1]) + d[2] * V[2]) / (np.sqrt((d * d).sum()) * n2)
        k = np.flatnonzero(c == -0.72)
        if len(k):
            return d, V[:, k[0]]
    raise AssertionError("no exact -0.72 pair in the search range")


def _system(rng, n_frames, n_ion, n_wat, box, edges=True):
    """xyz [F,3,N] (ions first, then O H1 H2 per water), box [F,3], ion indices, water first-atom indices."""
    n = n_ion + 3 * n_wat
    L = np.asarray(box, dtype=np.float64)
    xyz = np.round(rng.uniform(0, 1, (n_frames, 3, n)) * L[None, :, None], 3)
    o = n_ion + 3 * np.arange(n_wat)
    for h in (1, 2):
        xyz[:, :, o + h] = np.round(xyz[:, :, o] + rng.normal(0, 0.6, (n_frames, 3, n_wat)), 3)
    if edges:
        f = xyz[0]
        f[:, 0] = f[:, o[0]]  # an ion on an O: NaN
        f[:, 1] = [5.0, 5.0, 2.0]  # O at exactly r_cut = 3.5
        f[:, o[1]] = [8.5, 5.0, 2.0]
        f[:, 2] = [4.0, 9.0, 1.0]  # d_z == -Lz/2 and +Lz/2 exactly (Lz = 6): not wrapped, opposite signs
        f[:, o[2]] = [4.0, 9.5, 4.0]
        f[:, 3] = [9.0, 4.0, 5.0]
        f[:, o[3]] = [9.5, 4.0, 2.0]
        f[:, 4] = [0.2, 12.0, 3.0]  # a water across the x boundary, H1 on the other side
        f[:, o[4]] = [L[0] - 0.3, 12.0, 3.0]
        f[:, o[4] + 1] = [0.4, 12.5, 3.2]
        d, v = _exact_cos_pair()  # cos exactly -0.72: O, H1 = O + v, H2 = O
        f[:, o[5]] = [10.0, 10.0, 3.0]
        f[:, 5] = f[:, o[5]] + d
        f[:, o[5] + 1] = f[:, o[5]] + v
        f[:, o[5] + 2] = f[:, o[5]]
    return xyz, np.tile(L, (n_frames, 1)), np.arange(n_ion), o


def _frames(xyz, box):
    return [dict(xyz=xyz[f], bounds=np.column_stack([np.zeros(3), box[f]]), timestep=f) for f in range(len(xyz))]


def _check_lists(B, xyz, box, ions, wat, r_cut, cap, xin=None):
    idx, cos, count = B.hydration_cosines(xin if xin is not None else xyz, box, ions, wat, r_cut ** 2, cap=cap)
    n_cos = 0
    for f, fr in enumerate(_frames(xyz, box)):
        for c, (sel, want) in enumerate(R.frame_rows(fr, ions, wat, r_cut)):
            k = count[f, c]
            assert k == len(sel) and np.array_equal(idx[f, c, :k], sel), (f, c)
            assert cos[f, c, :k].tobytes() == want.tobytes(), (f, c)
            n_cos += k
    return idx, cos, count, n_cos


def test_random_systems_with_edges(B):
    rng = np.random.default_rng(7)
    xyz, box, ions, wat = _system(rng, 5, 21, 700, [16.0, 16.0, 6.0])
    _, cos, count, n = _check_lists(B, xyz, box, ions, wat, 3.5, cap=16)
    assert count.max() > 16  # rows overflowed the first cap and were re-run
    assert np.isnan(cos[0, 0, :count[0, 0]]).sum() == 1
    assert (cos[0, 5, :count[0, 5]] == -0.72).sum() >= 1
    sel, _ = R.frame_rows(_frames(xyz, box)[0], ions, wat, 3.5)[1]
    assert 1 not in sel  # the O at exactly r_cut is out
    for c in (2, 3):  # d == -L/2 and +L/2: both in, with opposite signs of d_z
        sel, _ = R.frame_rows(_frames(xyz, box)[0], ions, wat, 3.5)[c]
        assert c in sel


def _check_counts(B, xyz, box, ions, wat, cos, count):
    n_water, n_away, hist = B.hydration_counts(xyz, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    assert np.array_equal(n_water, count)
    valid = np.arange(cos.shape[2])[None, None, :] < count[:, :, None]
    assert np.array_equal(n_away, ((cos < -0.72) & valid).sum(axis=2))
    c = cos[valid]
    c = c[~np.isnan(c)]
    want = np.bincount(np.clip(np.trunc((c + 1.0) / 0.02).astype(np.int64), 0, 99), minlength=100)
    assert np.array_equal(hist.astype(np.int64), want)
    rw, ra, rh = R.counts(_frames(xyz, box), 1, 2, 3.5, [len(ions), len(wat)], [1, 3])
    assert np.array_equal(n_water, rw) and np.array_equal(n_away, ra) and np.array_equal(hist.astype(np.int64), rh)


def test_counts_match_lists_and_restatement(B):
    rng = np.random.default_rng(11)
    xyz, box, ions, wat = _system(rng, 4, 37, 900, [16.0, 16.0, 6.0])
    _, cos, count = B.hydration_cosines(xyz, box, ions, wat, 3.5 ** 2)
    _check_counts(B, xyz, box, ions, wat, cos, count)


def test_waters_past_one_chunk(B):
    """4097 waters: the O of the last one is candidate 4096, the first of the sweep's second chunk (shell::CHUNK of
    csrc/shell_search.h). The last cation (alone in the short last tile of centres) has the last two waters in its
    row: candidates of both chunks, appended by different blocks."""
    rng = np.random.default_rng(13)
    xyz, box, ions, wat = _system(rng, 2, 17, 4097, [16.0, 16.0, 6.0], edges=False)
    xyz[1][:, ions[16]] = [8.0, 8.0, 3.0]
    xyz[1][:, wat[4095]] = [9.0, 8.0, 3.0]
    xyz[1][:, wat[4096]] = [8.0, 9.5, 3.0]
    idx, cos, count, _ = _check_lists(B, xyz, box, ions, wat, 3.5, cap=4)  # every row overflows and is re-run
    row = idx[1, 16, :count[1, 16]]
    assert 4095 in row and 4096 in row and (row < 4095).any()
    _check_counts(B, xyz, box, ions, wat, cos, count)


def test_a_million_cosines_against_numpy(B):
    rng = np.random.default_rng(3)
    xyz, box, ions, wat = _system(rng, 12, 1000, 4000, [40.0, 40.0, 40.0], edges=False)
    _, _, count, n = _check_lists(B, xyz, box, ions, wat, 7.0, cap=16)
    assert n >= 10 ** 6, n


def test_device_input(B):
    import torch

    rng = np.random.default_rng(5)
    xyz, box, ions, wat = _system(rng, 3, 21, 700, [16.0, 16.0, 6.0])
    dev = torch.as_tensor(xyz, device="cuda")
    _check_lists(B, xyz, box, ions, wat, 3.5, cap=4, xin=dev)  # overflowing rows re-run from the device
    got = B.hydration_counts(dev, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    want = B.hydration_counts(xyz, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_more_than_65535_frames(B):
    rng = np.random.default_rng(9)
    F = 70001
    xyz, box, ions, wat = _system(rng, F, 3, 4, [5.0, 5.0, 5.0], edges=False)
    idx, cos, count = B.hydration_cosines(xyz, box, ions, wat, 2.5 ** 2, cap=4)
    frames = _frames(xyz, box)
    for f in list(range(0, F, 997)) + [F - 1]:
        for c, (sel, want) in enumerate(R.frame_rows(frames[f], ions, wat, 2.5)):
            assert count[f, c] == len(sel) and cos[f, c, :len(sel)].tobytes() == want.tobytes(), (f, c)
    n_water, n_away, hist = B.hydration_counts(xyz, box, ions, wat, 2.5 ** 2, -0.72, 0.02, 100)
    assert np.array_equal(n_water, count) and int(hist.sum()) == int((cos == cos).sum())


def test_orientation_counts_on_golden_box(z, H, tmp_path):
    frames, kw = R.case_args(z, "box")
    pattern = R.write_dumps(frames, str(tmp_path))
    per, dist = H.calc_hydration_orientation(os.path.join(str(tmp_path), pattern), 1, 2, 3.5, kw["num_mols"],
                                             kw["num_atoms_per_mol"])
    rw, ra, rh = R.counts(frames, 1, 2, 3.5, kw["num_mols"], kw["num_atoms_per_mol"])
    assert list(per.columns) == ["frame", "timestep", "cation_id", "n_water", "n_away", "factor"]
    assert np.array_equal(per["n_water"].to_numpy(), rw.ravel())
    assert np.array_equal(per["n_away"].to_numpy(), ra.ravel())
    assert np.array_equal(per["factor"].to_numpy(), ra.ravel() / rw.ravel())
    assert np.array_equal(dist["count"].to_numpy(), rh) and len(dist) == 100
    assert dist["fraction"].sum() == pytest.approx(1.0)
    # the zero case: no error here, factor NaN for the ions without water
    per0, _ = H.calc_hydration_orientation(os.path.join(str(tmp_path), pattern), 1, 2, 0.5, kw["num_mols"],
                                           kw["num_atoms_per_mol"])
    assert np.isnan(per0["factor"]).any() and (per0["n_water"] == 0).any()
