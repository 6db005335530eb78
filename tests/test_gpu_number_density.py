"""
calc_number_density / calc_density_profile and their kernel (csrc/density.hip) on the GPU: the reference's DataFrame
and CSV bit for bit on every recorded case, and backend.axis_profile against the numpy restatement
(tests/number_density_ref.py) by equality — counts, the extent by bytes, outside — on seeded systems built to hit every
edge: b / bin_size an exact integer, s == dist_from_interface exactly, b == 0.0 and -0.0, k == n_bins - 1, n_bins,
-n_bins and -n_bins - 1, NaN coordinates, atom counts off the block size, a frame of 2 000 003 atoms (the split path),
70 001 small frames, 8 x 20 000 bins (no LDS histogram), codes per frame and shared, device input, and in one call more
than 10**7 binned atoms.
"""
import os

import numpy as np
import pytest

import number_density_ref as R

pytestmark = pytest.mark.gpu

W, D, NB = 0.5, 12.0, 24


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ND():
    from mdproptools_amd.structural import number_density

    return number_density


def _same(got, want):
    counts, extent, outside = got
    assert counts.dtype == np.uint32 and outside.dtype == np.uint32
    assert counts.shape == want[0].shape
    assert np.array_equal(counts, want[0])
    assert extent.tobytes() == want[1].tobytes()
    assert np.array_equal(outside, want[2])


@pytest.mark.parametrize("key", list(R.CASES))
def test_dropin_frame_and_csv(z, ND, key, tmp_path):
    frames, kw = R.case_args(z, key)
    pattern = R.write_dumps(frames, str(tmp_path))
    if key in R.RAISES:
        with pytest.raises(Exception) as info:
            ND.calc_number_density(pattern, working_dir=str(tmp_path), **kw)
        assert type(info.value).__name__ == str(z[key + "_error"])
        assert not os.path.exists(tmp_path / "number_density.csv")
        return
    df = ND.calc_number_density(pattern, working_dir=str(tmp_path), **kw)
    assert (tmp_path / "number_density.csv").read_bytes() == z[key + "_csv"].tobytes()
    assert [str(c) for c in df.columns] == [str(c) for c in z[key + "_columns"]]
    assert df.to_numpy().tobytes() == z[key + "_values"].tobytes()
    quiet = ND.calc_number_density(pattern, working_dir=str(tmp_path), results_file="other.csv", save_mode=False, **kw)
    assert quiet.to_numpy().tobytes() == z[key + "_values"].tobytes() and not os.path.exists(tmp_path / "other.csv")


def _edge_system(rng, n_frames=6, n=2203, n_rows=3):
    """x [F,N], codes [F,N] for W, D, NB. Frame 0: surface from 1.0 to 5.0 (range 4) and one atom per edge of the
    reference modes; frame 1: one surface atom at +0.0 (range 0: b == -0.0, k == n_bins - 1); frame 2: surface atoms
    at -0.0, +0.0 and NaN; frame 3: no surface atom; the rest random."""
    x = np.round(rng.uniform(-10.0, 30.0, (n_frames, n)), 3)
    row = rng.integers(-1, n_rows, (n_frames, n))
    surf = np.zeros((n_frames, n), dtype=bool)
    surf[:, :20] = True
    x[:, :20] = np.round(rng.uniform(1.0, 5.0, (n_frames, 20)), 3)
    x[:, 0], x[:, 1] = 1.0, 5.0
    row[:, 20:40] = rng.integers(0, n_rows, (n_frames, 20))
    x[0, 20:29] = [8.0,    # b = 3.0: b / w == 6 exactly
                   13.0,   # s == D: not selected (positive mode); s / w == n_bins: outside (negative mode)
                   5.0,    # b == 0.0
                   -7.0,   # b = -12: k == -n_bins, wraps to bin 0
                   -7.5,   # b = -12.5: k == -n_bins - 1, outside
                   np.nan,
                   -11.0,  # s == -D: not selected (negative mode)
                   12.9,   # negative mode: k == n_bins - 1
                   4.9]    # b in (-w, 0): bin 0
    surf[1] = False
    surf[1, 0] = True
    x[1, 0] = 0.0
    x[1, 20:26] = [-0.0, 0.0, 11.75, 12.0, -12.0, -12.5]
    surf[2] = False
    surf[2, :3] = True
    x[2, :3] = [-0.0, 0.0, np.nan]
    surf[3] = False
    row[4, 5] = 1  # a surface atom that is counted as well
    codes = np.where(row < 0, R.NONE, row) | np.where(surf, R.SURFACE, 0)
    return x, codes.astype(np.uint16)


def test_edges_reference_modes(B):
    x, codes = _edge_system(np.random.default_rng(11))
    for mode, d in ((R.REF_POS, D), (R.REF_NEG, -D)):
        want = R.axis_profile(x, codes, mode, W, d, NB, 3)
        _same(B.axis_profile(x, codes, mode, W, d, NB, 3), want)
        assert want[2][0] >= 1 and want[2][1] >= 1  # the constructed atoms without a bin
        assert np.isnan(want[1][3]).all() and want[0][3].sum() == 0 and want[2][3] == 0
        assert np.signbit(want[1][2][0]) and not np.signbit(want[1][2][1]) and (want[1][2] == 0).all()
    # the constructed atoms of frame 0 alone, one at a time, in the positive mode: where each one lands
    sel = np.r_[0, 1, 20:29]
    lands = [("bin", 6), ("none", 0), ("bin", 0), ("bin", 0), ("out", 0), ("none", 0), ("out", 0), ("bin", 15),
             ("bin", 0)]
    for i, (kind, k) in zip(range(20, 29), lands):
        c = np.full(len(sel), R.NONE, dtype=np.uint16)
        c[:2] |= R.SURFACE
        c[2 + i - 20] = 0
        got = B.axis_profile(x[:1, sel], c, R.REF_POS, W, D, NB, 1)
        _same(got, R.axis_profile(x[:1, sel], c, R.REF_POS, W, D, NB, 1))
        assert got[0].sum() == (kind == "bin") and got[2][0] == (kind == "out"), (i, kind)
        if kind == "bin":
            assert got[0][0, 0, k] == 1, (i, k)
    # frame 1 (range 0): without the surface atom nothing is selected
    got = B.axis_profile(x[1:2, 20:26], np.zeros(6, dtype=np.uint16), R.REF_NEG, W, -D, NB, 1)
    _same(got, R.axis_profile(x[1:2, 20:26], np.zeros(6, dtype=np.uint16), R.REF_NEG, W, -D, NB, 1))
    assert np.isnan(got[1]).all() and got[0].sum() == 0
    c1 = np.r_[np.uint16(R.SURFACE | R.NONE), np.zeros(6, dtype=np.uint16)]
    x1 = x[1:2, np.r_[0, 20:26]]
    neg = B.axis_profile(x1, c1, R.REF_NEG, W, -D, NB, 1)
    _same(neg, R.axis_profile(x1, c1, R.REF_NEG, W, -D, NB, 1))
    assert neg[0][0, 0, 0] == 2 and neg[0][0, 0, NB - 1] == 1 and neg[2][0] == 1  # -0.0, 0.0 | 11.75 | 12.0
    pos = B.axis_profile(x1, c1, R.REF_POS, W, D, NB, 1)
    _same(pos, R.axis_profile(x1, c1, R.REF_POS, W, D, NB, 1))
    assert pos[0][0, 0, 0] == 3 and pos[0][0, 0, NB - 1] == 1 and pos[2][0] == 1  # -0.0, 0.0, -12.0 | 11.75 | -12.5


def test_edges_profile_mode(B):
    rng = np.random.default_rng(12)
    x, codes = _edge_system(rng)
    given = np.round(rng.uniform(0.0, 5.0, len(x)), 3)
    for origin in ("lo", "hi", given, 2.5):
        want = R.axis_profile(x, codes, R.PROFILE, W, -6.0, NB, 3, origin=origin)
        _same(B.axis_profile(x, codes, R.PROFILE, W, -6.0, NB, 3, origin=origin), want)
        assert want[2].sum() > 0 and want[0].sum() > 0
    # t == n_bins exactly is outside, t == 0 and t == n_bins - 1 are bins, NaN and t < 0 are outside
    xs = np.array([[2.0, 8.0, -4.0, 7.5, np.nan, -4.001]])
    cs = np.array([R.SURFACE | R.NONE, 0, 0, 0, 0, 0], dtype=np.uint16)
    got = B.axis_profile(xs, cs, R.PROFILE, W, -6.0, NB, 1, origin="hi")
    _same(got, R.axis_profile(xs, cs, R.PROFILE, W, -6.0, NB, 1, origin="hi"))
    assert got[0][0, 0, 0] == 1 and got[0][0, 0, NB - 1] == 1 and got[0].sum() == 2 and got[2][0] == 3


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1024, 1025, 5000, 16383, 16384, 16385, 20011])
def test_sizes_around_the_block_and_the_chunk(B, n):
    rng = np.random.default_rng(n)
    x = np.round(rng.uniform(-2.0, 14.0, (5, n)), 3)
    row = rng.integers(-1, 4, n)
    surf = rng.uniform(size=n) < 0.1
    x[:, surf] = np.round(rng.uniform(0.0, 3.0, (5, int(surf.sum()))), 3)
    codes = B.axis_profile_codes(row, surf)
    for mode, d in ((R.REF_POS, D), (R.REF_NEG, -15.0), (R.PROFILE, -3.0)):
        nb = int(abs(15.0) / W)
        _same(B.axis_profile(x, codes, mode, W, d, nb, 4), R.axis_profile(x, codes, mode, W, d, nb, 4))


def test_shared_and_per_frame_codes_and_device_input(B):
    import torch

    rng = np.random.default_rng(21)
    F, n = 40, 5003
    x = np.round(rng.uniform(-5.0, 25.0, (F, n)), 3)
    row = rng.integers(-1, 5, (F, n))
    surf = rng.uniform(size=(F, n)) < 0.05
    per_frame = B.axis_profile_codes(row, surf)
    shared = B.axis_profile_codes(row[0], surf[0])
    xd = torch.from_numpy(x).cuda()
    for codes in (shared, per_frame):
        want = R.axis_profile(x, codes, R.REF_POS, 0.173, 20.0, int(20.0 / 0.173), 5)
        _same(B.axis_profile(x, codes, R.REF_POS, 0.173, 20.0, int(20.0 / 0.173), 5), want)
        _same(B.axis_profile(xd, codes, R.REF_POS, 0.173, 20.0, int(20.0 / 0.173), 5), want)
    same = np.broadcast_to(shared, (F, n))
    _same(B.axis_profile(x, np.ascontiguousarray(same), R.PROFILE, 0.25, -5.0, 100, 5, origin="hi"),
          B.axis_profile(xd, shared, R.PROFILE, 0.25, -5.0, 100, 5, origin="hi"))


def test_ten_million_atoms_in_full_frames(B):
    """700 frames of 16 384 atoms (every lane of the one-workgroup path holds its 16 atoms), every atom binned."""
    rng = np.random.default_rng(31)
    F, n = 700, 16384
    x = np.round(rng.normal(8.0, 3.0, (F, n)), 3)
    row = rng.integers(0, 3, n)
    surf = np.arange(n) < 100
    x[:, :100] = np.round(rng.uniform(0.0, 2.0, (F, 100)), 3)
    codes = B.axis_profile_codes(row, surf)
    got = B.axis_profile(x, codes, R.PROFILE, 0.1, -40.0, 800, 3, origin="lo")
    assert int(got[0].sum(dtype=np.int64)) == F * n > 10 ** 7 and not got[2].any()
    _same(got, R.axis_profile(x, codes, R.PROFILE, 0.1, -40.0, 800, 3, origin="lo"))


def test_one_frame_of_two_million_atoms(B):
    """The split path: chunks of one frame over many workgroups, with the histogram in LDS and (8 x 20 000) without."""
    rng = np.random.default_rng(41)
    n = 2_000_003
    x = np.round(rng.uniform(-3.0, 20.0, (1, n)), 4)
    row = rng.integers(-1, 8, n)
    surf = rng.uniform(size=n) < 0.01
    x[0, surf] = np.round(rng.uniform(0.0, 4.0, int(surf.sum())), 4)
    x[0, 5::100_000] = np.nan
    codes = B.axis_profile_codes(row, surf)
    for mode, d in ((R.REF_POS, D), (R.REF_NEG, -30.0)):
        nb = int(abs(d) / W)
        _same(B.axis_profile(x, codes, mode, W, d, nb, 8), R.axis_profile(x, codes, mode, W, d, nb, 8))
    got = B.axis_profile(x, codes, R.PROFILE, 0.001, -2.0, 20000, 8, origin="hi")
    _same(got, R.axis_profile(x, codes, R.PROFILE, 0.001, -2.0, 20000, 8, origin="hi"))
    assert got[0].sum() > 10 ** 6 and got[2][0] > 0


def _group_bytes():
    """AP_GROUP_BYTES of csrc/density.hip: the coordinate bytes the split path launches at a time."""
    import re

    from conftest import REPO

    text = open(os.path.join(REPO, "mdproptools_amd", "csrc", "density.hip")).read()
    m = re.search(r"AP_GROUP_BYTES = \(size_t\)(\d+) << 20;", text)
    assert m, "AP_GROUP_BYTES not found"
    return int(m.group(1)) << 20


def test_split_frames_in_several_groups(B):
    """The split path launches its frames in groups of AP_GROUP_BYTES: frames of 20 011 atoms, more than two groups'
    worth of them, codes per frame and an origin per frame, so that every offset of a later group (coordinates, codes,
    origins, counts, extent, outside, the reused partials) is compared; frames without surface atoms in each group."""
    rng = np.random.default_rng(51)
    n = 20011
    group = _group_bytes()
    F = 2 * group // (n * 8) + 24
    per_group = group // (n * 8)
    assert F * n * 8 > 2 * group and F > 2 * per_group  # three groups, the last one short
    x = np.round(rng.uniform(-3.0, 20.0, (F, n)), 3)
    row = rng.integers(-1, 3, (F, n), dtype=np.int8)
    surf = rng.uniform(size=(F, n)) < 0.02
    surf[[7, per_group, 2 * per_group + 3]] = False
    codes = B.axis_profile_codes(row, surf)
    got = B.axis_profile(x, codes, R.REF_POS, W, D, NB, 3)
    _same(got, R.axis_profile(x, codes, R.REF_POS, W, D, NB, 3))
    assert got[0][per_group:].sum() > 0 and got[2][2 * per_group:].sum() > 0 and np.isnan(got[1][per_group]).all()
    org = np.round(rng.uniform(0.0, 4.0, F), 3)
    got = B.axis_profile(x, codes, R.PROFILE, W, -4.0, 40, 3, origin=org)
    _same(got, R.axis_profile(x, codes, R.PROFILE, W, -4.0, 40, 3, origin=org))
    assert got[0][2 * per_group:].sum() > 0
    # shared codes and a device tensor through the same groups
    import torch

    shared = codes[0]
    _same(B.axis_profile(torch.from_numpy(x).cuda(), shared, R.REF_NEG, W, -30.0, 60, 3),
          R.axis_profile(x, shared, R.REF_NEG, W, -30.0, 60, 3))


def test_seventy_thousand_small_frames(B):
    """More frames than a grid's y or z dimension holds: 70 001 frames of 5 atoms, 1000 distinct ones repeated."""
    rng = np.random.default_rng(61)
    F, n, base = 70_001, 5, 1000
    xb = np.round(rng.uniform(-1.0, 13.0, (base + 1, n)), 2)
    cb = B.axis_profile_codes(rng.integers(-1, 2, (base + 1, n)), rng.uniform(size=(base + 1, n)) < 0.4)
    pick = np.arange(F) % base
    pick[-1] = base
    x, codes = np.ascontiguousarray(xb[pick]), np.ascontiguousarray(cb[pick])
    for mode, d in ((R.REF_POS, D), (R.PROFILE, -6.0)):
        want = R.axis_profile(xb, cb, mode, W, d, NB, 2)
        _same(B.axis_profile(x, codes, mode, W, d, NB, 2), tuple(a[pick] for a in want))


def test_histogram_too_large_for_lds(B):
    rng = np.random.default_rng(71)
    F, n = 3, 5000
    x = np.round(rng.uniform(0.0, 14.0, (F, n)), 4)
    codes = B.axis_profile_codes(rng.integers(-1, 8, n), np.arange(n) < 50)
    x[:, :50] = np.round(rng.uniform(0.0, 1.0, (F, 50)), 4)
    for mode in (R.REF_POS, R.REF_NEG):
        d = D if mode == R.REF_POS else -D
        _same(B.axis_profile(x, codes, mode, 0.0006, d, 20000, 8), R.axis_profile(x, codes, mode, 0.0006, d, 20000, 8))


def _profile_frames(z, same_types=False):
    frames = R.frames_of(z, "b")
    if same_types:  # every frame with frame 0's types: the labels (and masses) are then shared by the frames
        frames = [dict(f, types=frames[0]["types"]) for f in frames]
    x = np.stack([f["xyz"][2] for f in frames])
    boxes = np.stack([f["bounds"][:, 1] - f["bounds"][:, 0] for f in frames])
    types = np.stack([f["types"] for f in frames])  # (drawn per frame: the labels differ from frame to frame)
    assert (types != types[0]).any() != same_types
    return frames, x, boxes, types


@pytest.mark.parametrize("origin", ["top", "bottom", 4.25])
def test_density_profile_atom_mode(z, ND, origin, tmp_path):
    frames, x, boxes, types = _profile_frames(z)
    pattern = os.path.join(str(tmp_path), R.write_dumps(frames, str(tmp_path)))
    atom_types = [1, 3, 1, 2]
    df = ND.calc_density_profile(pattern, 3, atom_types, 0.25, "z", -6.0, 9.0, origin=origin, per_frame=True)
    rows = np.select([types == 1, types == 3, types == 2], [0, 1, 2], -1)
    s, mean, std, counts, ext, outside = R.density_profile(x, rows, types == 3, boxes, 2, 0.25, -6.0, 9.0, origin, 3)
    pick = [0, 1, 0, 2]
    assert list(df.columns) == ["s", "rho_1", "rho_3", "rho_1", "rho_2", "std_1", "std_3", "std_1", "std_2"]
    v = df.to_numpy()
    assert v[:, 0].tobytes() == s.tobytes()
    assert v[:, 1:5].T.copy().tobytes() == mean[pick].tobytes() and v[:, 5:].T.copy().tobytes() == std[pick].tobytes()
    assert np.array_equal(df.attrs["counts"], counts[:, pick]) and df.attrs["extent"].tobytes() == ext.tobytes()
    assert np.array_equal(df.attrs["outside"], outside) and outside.sum() > 0 and counts.sum() > 0
    assert df.attrs["timesteps"].tolist() == [f["timestep"] for f in frames]
    # the altered-id route: labels 1 (the slab), 2 and 3 (first and second atom of every two-atom molecule)
    df2 = ND.calc_density_profile(pattern, 1, [3], 0.25, "z", -6.0, 9.0, origin=origin, num_mols=[200, 1000],
                                  num_atoms_per_mol=[1, 2], per_frame=True)
    lab = R.labels_of(frames[0], [200, 1000], [1, 2])
    want = R.density_profile(x, np.where(lab == 3, 0, -1), lab == 1, boxes, 2, 0.25, -6.0, 9.0, origin, 1)
    assert np.array_equal(df2.attrs["counts"], want[3]) and df2["rho_3"].to_numpy().tobytes() == want[1][0].tobytes()


@pytest.mark.parametrize("same_types", [False, True])
@pytest.mark.parametrize("origin", ["top", 4.25])
def test_density_profile_com_mode(z, ND, origin, same_types, tmp_path):
    """same_types False: masses per frame, one segment_com call per frame; True: one call over the whole batch."""
    frames, x, boxes, types = _profile_frames(z, same_types)
    pattern = os.path.join(str(tmp_path), R.write_dumps(frames, str(tmp_path)))
    mass = [15.999, 1.008, 26.982]
    num_mols, num_atoms = [200, 1000], [1, 2]
    df = ND.calc_density_profile(pattern, 3, [2, 1], 0.25, "z", -6.0, 9.0, origin=origin, num_mols=num_mols,
                                 num_atoms_per_mol=num_atoms, mass=mass, position="com", per_frame=True)
    com = df.attrs["com"]
    assert com.shape == (len(frames), 1200)
    # the centres of mass against numpy, at the tolerance tests/test_gpu_parity.py uses for segment_com
    m = np.asarray(mass)[types - 1]  # [F,N]: masses per frame
    seg = np.r_[np.arange(0, 200), np.arange(200, 2201, 2)]
    want_com = np.add.reduceat(x * m, seg[:-1], axis=1) / np.add.reduceat(m, seg[:-1], axis=1)
    np.testing.assert_allclose(com, want_com, rtol=1e-13, atol=1e-13)
    # the counts exactly, from the centres of mass the device returned; the surface extent from the ATOMS
    ext = np.array([R.extent(xf, tf == 3) for xf, tf in zip(x, types)])
    org = ext[:, 1] if origin == "top" else origin
    mol_rows = np.r_[np.full(200, 1), np.zeros(1000, dtype=np.int64)]  # atom_types [2, 1]: molecule type 2 is row 0
    s, mean, std, counts, _, outside = R.density_profile(com, mol_rows, np.zeros(1200, dtype=bool), boxes, 2, 0.25,
                                                         -6.0, 9.0, org, 2)
    assert np.array_equal(df.attrs["counts"], counts) and np.array_equal(df.attrs["outside"], outside)
    assert df.attrs["extent"].tobytes() == ext.tobytes()
    assert df["rho_2"].to_numpy().tobytes() == mean[0].tobytes() and df["std_1"].to_numpy().tobytes() == std[1].tobytes()
    assert counts[:, 1].sum() > 0 and counts[:, 0].sum() > 0
