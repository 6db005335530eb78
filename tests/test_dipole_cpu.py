"""The numpy restatement of the orientational pair sums and the dielectric constant (tests/dipole_ref.py) against closed
forms, and the host logic of structural/orientational_correlation.py and structural/dielectric.py. No GPU."""
import math

import numpy as np
import pytest

import dipole_ref as D
from mdproptools_amd import _lib, backend
from mdproptools_amd.common import constants
from mdproptools_amd.structural import dielectric as DC
from mdproptools_amd.structural import orientational_correlation as OC


def _lattice(n):
    """Sites [1,3,n^3] of a simple cubic lattice of spacing 1 in a box of edge n, and the lattice indices [3,n^3]."""
    idx = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")).reshape(3, -1)
    return idx[None].astype(np.float64) + 0.25, idx


# neighbours of a simple cubic lattice by squared distance, up to 6
SHELLS = {1: 6, 2: 12, 3: 8, 4: 6, 5: 24, 6: 24}


def _lattice_sums(vec, n=6):
    site, _ = _lattice(n)
    N = n ** 3
    box = np.full((1, 3), float(n))
    off = np.array([0, N], dtype=np.int64)
    return D.vector_pair_hist(site, vec, box, off, [(0, 0)], 0.1, 25, _lib.bin_edges(0.1, 25)), N


def test_bisected_edges_are_the_library_s():
    for bin_size, nbins in ((0.1, 25), (0.05, 400), (0.173, 42)):
        assert np.array_equal(D.bin_edges(bin_size, nbins), _lib.bin_edges(bin_size, nbins))


def test_parallel_vectors_give_one_and_the_neighbour_count():
    n = 6
    vec = np.zeros((1, 3, n ** 3))
    vec[0, 2] = 1.0
    (hist, sums, beyond, unsummed, pairs), N = _lattice_sums(vec, n)
    assert unsummed[0] == 0 and int(hist[0].sum()) + int(beyond[0]) == int(pairs[0]) == N * (N - 1)
    want = np.zeros(25, dtype=np.int64)
    for r2, cnt in SHELLS.items():
        want[int(math.sqrt(r2) / 0.1)] += cnt * N
    assert hist[0].tolist() == want.tolist()
    cols = D.pair_columns(hist[0], sums[0], 1, N, N, True, float(n) ** 3, 0.1)
    filled = want > 0
    assert np.all(cols["<cos>"][filled] == 1.0) and np.all(cols["<P2>"][filled] == 1.0)
    assert np.all(np.isnan(cols["<cos>"][~filled]))
    assert cols["G_K"].tolist() == (1.0 + np.cumsum(want) / N).tolist()       # 1 + the neighbours within R
    # the direction sum: the neighbours of a shell come in opposite pairs
    assert all(int(v) == 0 for v in sums[0, 2])


def test_alternating_vectors_give_the_shell_sums():
    n = 6
    _, idx = _lattice(n)
    vec = np.zeros((1, 3, n ** 3))
    vec[0, 2] = 1.0 - 2.0 * (idx.sum(axis=0) % 2)
    (hist, sums, _, unsummed, _), N = _lattice_sums(vec, n)
    assert unsummed[0] == 0
    want = np.zeros(25, dtype=object)
    for r2, cnt in SHELLS.items():
        want[int(math.sqrt(r2) / 0.1)] += (-1) ** r2 * cnt * N * D.ONE      # the parity of dx + dy + dz is that of r^2
    assert sums[0, 0].tolist() == want.tolist()
    assert sums[0, 1].tolist() == [int(h) * D.ONE for h in hist[0]]          # cos^2 = 1 for every pair
    cols = D.pair_columns(hist[0], sums[0], 1, N, N, True, float(n) ** 3, 0.1)
    assert cols["<cos>"][10] == -1.0 and cols["<cos>"][14] == 1.0 and cols["<P2>"][10] == 1.0
    assert cols["G_K"][10] == 1.0 - 6.0 and cols["G_K"][24] == 1.0 - 6 + 12 - 8 + 6 - 24 + 24


def test_a_vector_along_the_pair_direction_gives_one():
    rng = np.random.default_rng(5)
    d = rng.normal(size=(3, 50))
    d *= rng.uniform(0.5, 4.0, 50) / np.linalg.norm(d, axis=0)
    site = np.concatenate([np.full((3, 1), 7.0), 7.0 + d], axis=1)[None]
    vec = np.concatenate([np.array([[1.0], [0.0], [0.0]]), d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])], axis=1)[None]
    box = np.full((1, 3), 20.0)
    off = np.array([0, 1, 51], dtype=np.int64)
    hist, sums, beyond, unsummed, pairs = D.vector_pair_hist(site, vec, box, off, [(0, 1), (1, 0)], 0.5, 10)
    assert beyond.tolist() == [0, 0] and unsummed.tolist() == [0, 0] and pairs.tolist() == [50, 50]
    cols = D.pair_columns(hist[0], sums[0], 1, 1, 50, False, 8000.0, 0.5)
    assert np.all(cols["<cos_r>"][hist[0] > 0] == 1.0)
    # the other way round e is the centre's vector e_x against the direction back to it: minus the x component
    back = np.rint(-vec[0, 0, 1:] * 4294967296.0)
    assert sum(int(v) for v in sums[1, 2]) == int(back.sum())
    assert hist[1].tolist() == hist[0].tolist() and sums[1, 0].tolist() == sums[0, 0].tolist()


def test_sites_anywhere_and_ties():
    """Sites several box lengths outside the cell give the same integers (the coordinates are small dyadic numbers:
    every shift is exact), and d * inv = +-0.5 shifts nothing."""
    rng = np.random.default_rng(8)
    site = np.rint(rng.random((2, 3, 30)) * 8.0 * 64) / 64
    vec = rng.normal(size=(2, 3, 30))
    vec /= np.sqrt((vec ** 2).sum(axis=1))[:, None, :]
    box = np.full((2, 3), 8.0)
    off = np.array([0, 30], dtype=np.int64)
    base = D.vector_pair_hist(site, vec, box, off, [(0, 0)], 0.25, 16)
    far = site + 8.0 * rng.integers(-3, 4, size=site.shape)
    moved = D.vector_pair_hist(far, vec, box, off, [(0, 0)], 0.25, 16)
    assert all(np.array_equal(a, b) for a, b in zip(base, moved))
    tie = np.zeros((1, 3, 2))
    tie[0, 0, 1] = 4.0                                                  # d = +-4 = +-L/2: stays, rsq = 16 either way
    up = np.zeros((1, 3, 2))
    up[0, 2] = 1.0
    hist, sums, beyond, unsummed, _ = D.vector_pair_hist(tie, up, box[:1], np.array([0, 2]), [(0, 0)], 0.5, 9)
    assert hist[0, 8] == 2 and beyond[0] == 0 and unsummed[0] == 0 and int(sums[0, 2, 8]) == 0


def test_what_cannot_be_summed_and_what_is_beyond():
    site = np.array([[[0.0, 0.0, 1.0, 2.0, np.nan], [0.0] * 5, [0.0] * 5]])
    vec = np.zeros((1, 3, 5))
    vec[0, 0] = [1.0, 1.0, np.nan, 3.0, 1.0]
    box = np.full((1, 3), 10.0)
    hist, sums, beyond, unsummed, pairs = D.vector_pair_hist(site, vec, box, np.array([0, 5]), [(0, 0)], 0.5, 8)
    assert pairs[0] == 20 and beyond[0] == 8 and int(hist[0].sum()) == 12
    # coincident 0-1 (2), every pair with the NaN vector (6) and with the vector of length 3 (4 more): none is left to sum
    assert unsummed[0] == 12 and all(int(v) == 0 for v in sums[0].ravel())
    zero_edge = np.array([[10.0, 0.0, 10.0]])
    hist, _, beyond, unsummed, pairs = D.vector_pair_hist(site[:, :, :2], vec[:, :, :2], zero_edge, np.array([0, 2]), [(0, 0)], 0.5, 8)
    assert beyond[0] == 2 and not hist.any() and unsummed[0] == 0


def test_words_combine_to_signed_integers():
    words = np.array([[5, 0], [2 ** 64 - 1, 2 ** 64 - 1], [0, 1], [0, 2 ** 63], [2 ** 64 - 7, 3]], dtype=np.uint64)
    assert backend.combine_words(words).tolist() == [5, -1, 2 ** 64, -(2 ** 127), 3 * 2 ** 64 + 2 ** 64 - 7]
    # a carry across 2^64 built by hand: the kernel's flush of three addends into one pair of words
    lo = hi = 0
    total = 0
    for add in (2 ** 62 + 12345, 2 ** 63 - 1, 2 ** 62, -(2 ** 62) - 5, 2 ** 63 - 9, -3):
        a = add % 2 ** 64
        old, lo = lo, (lo + a) % 2 ** 64
        hi = (hi + (1 if lo < old else 0) + (2 ** 64 - 1 if add < 0 else 0)) % 2 ** 64
        total += add
    assert total > 2 ** 64 and backend.combine_words(np.array([lo, hi], dtype=np.uint64)).tolist() == total
    assert D.split_words(total) == (lo, hi) and D.split_words(-5) == (2 ** 64 - 5, 2 ** 64 - 1)
    for v in (0, -1, 2 ** 100, -(2 ** 100) + 17):
        assert backend.combine_words(np.array(D.split_words(v), dtype=np.uint64)).tolist() == v
    with pytest.raises(ValueError, match="low, high"):
        backend.combine_words(np.zeros(3, dtype=np.uint64))


def test_two_batches_add_to_one():
    traj = D.water_like()
    got = D.mol_moments(traj["x"], traj["L"], [0], [40], [3], [[]], [[(1, 0.4), (2, 0.4)]], [1])
    off = np.array([0, 40], dtype=np.int64)
    whole = OC.PairSums(1, 12)
    whole.add(*D.vector_pair_hist(got["site"], got["vec"], traj["L"], off, [(0, 0)], 0.5, 12), traj["L"])
    parts = OC.PairSums(1, 12)
    for sl in (slice(0, 2), slice(2, 6)):
        parts.add(*D.vector_pair_hist(got["site"][sl], got["vec"][sl], traj["L"][sl], off, [(0, 0)], 0.5, 12), traj["L"][sl])
    assert parts.n_frames == whole.n_frames == 6 and parts.volumes == whole.volumes
    for name in ("hist", "sums", "beyond", "unsummed", "pairs"):
        assert getattr(parts, name).tolist() == getattr(whole, name).tolist(), name
    assert all(isinstance(v, int) for v in parts.sums.ravel().tolist())
    assert any(v < 0 for v in whole.sums[0, 0].tolist()) and whole.unsummed[0] == 0
    ours = OC.pair_columns(whole.hist[0], whole.sums[0], 6, 40, 40, True, float(np.mean(whole.volumes)), 0.5)
    want = D.pair_columns(whole.hist[0], whole.sums[0], 6, 40, 40, True, float(np.mean(whole.volumes)), 0.5)
    assert list(ours) == ["r", "g(r)", "<cos>", "<P2>", "<cos_r>", "G_K"]
    for name in want:
        assert D.same_bits(ours[name], want[name]), name


def test_species_and_pairs_are_checked():
    per = [3, 1]
    water, ion = (1, "dipole", 1), (2, None, "first")
    species, jobs = OC.checked_pairs([(water, water), (ion, water), ((1, (2, 3), "com"), ion)], per, mass=[16.0, 1.0, 23.0])
    assert species == [water, ion, (1, (2, 3), "com")] and jobs == [(0, 0), (1, 0), (2, 1)]
    assert [OC.species_label(s) for s in species] == ["1:dipole@1", "2:-@first", "1:2-3@com"]
    for bad, text in [([], "at least one"), ([(water,)], "a pair is"), ([(water, (1, "dipole"))], "a species is"),
                      ([(water, (3, None, 1))], r"mol_type must be in \[1, 2\]"),
                      ([(water, (1, (1, 4), 1))], r"tail and head must be in \[1, 3\]"),
                      ([(water, (1, (2, 2), 1))], "the same atom"), ([(water, (1, "axis", 1))], "vector must be"),
                      ([(water, (2, "dipole", 1))], "at least two atoms"), ([(water, (1, None, 4))], "site must be an atom index"),
                      ([(water, (1, None, "centre"))], "site must be an atom index"),
                      ([(water, (1, None, "com"))], "needs mass")]:
        with pytest.raises(ValueError, match=text):
            OC.checked_pairs(bad, per)
    q = np.array([-0.8, 0.4, 0.4] * 4 + [1.0] * 2)
    types = np.array([1, 2, 2] * 4 + [3] * 2)
    site_terms, vec_terms = OC.species_terms(species, [4, 2], per, q, types, [16.0, 1.0, 23.0])
    assert site_terms == [[], [], [(1, 1.0 / 18.0), (2, 1.0 / 18.0)]]
    assert vec_terms == [[(1, 0.4), (2, 0.4)], [], [(1, -1.0), (2, 1.0)]]
    assert OC.species_terms([(1, (1, 3), 3)], [4, 2], per) == ([[(2, 1.0)]], [[(2, 1.0)]])
    q[4] = 0.5
    with pytest.raises(ValueError, match="same charges"):
        OC.species_terms(species, [4, 2], per, q, types, [16.0, 1.0, 23.0])
    with pytest.raises(ValueError, match="wrapped"):
        OC.calc_orientational_correlation(5.0, 0.1, [(water, water)], "none.*.dump", [4, 2], per, coords="folded")
    with pytest.raises(ValueError, match=r"must be in \[1, 4096\]"):
        OC.calc_orientational_correlation(500.0, 0.1, [(water, water)], "none.*.dump", [4, 2], per)


def test_dielectric_closed_form():
    """M_x = 3 + 2 (-1)^t, M_y and M_z constant, over an even number of frames: the variance is 4 exactly, whatever the
    constants, and eps_r = 1 + factor * 4 / V to the last digit, in the restatement and in the module alike."""
    F = 8
    t = np.arange(F)
    total = np.zeros((2, 3, F))
    total[0, 0] = 3.0 + 2.0 * (-1.0) ** t
    total[0, 1] = 5.0
    total[1, 2] = -7.0
    sq_total = np.stack([np.full(F, 20.0), np.full(F, 30.0)])
    volume = np.full(F, 1000.0)
    assert constants.VACUUM_PERMITTIVITY == 8.8541878128 * 10 ** -12
    dip, dist = constants.DIPOLE_CONVERSION["real"], constants.DISTANCE_CONVERSION["real"]
    factor = dip ** 2 / (3.0 * constants.VACUUM_PERMITTIVITY * dist ** 3 * constants.BOLTZMANN * 300.0)
    closed = 1.0 + factor * 4.0 / 1000.0
    assert 1.0 < closed < 1000.0
    ref = D.dielectric(total, sq_total, volume, [10, 5], 300.0, dip, dist)
    ours = DC.dielectric_from_series(total, sq_total, volume, [10, 5], 300.0, "real")
    assert ref["eps_r"] == closed and ours["eps_r"] == closed
    assert ref["running"][0] == 1.0 and ref["running"][1] == closed       # one frame: no fluctuation; two: all of it
    assert ours["mu2"].tolist() == [2.0, 6.0] and ref["mu2"].tolist() == [2.0, 6.0]
    assert ours["g_K"].tolist() == [4.0 / 20.0, 0.0] and ref["g_K"].tolist() == [0.2, 0.0]
    for name in ("M", "running", "mu2", "g_K"):
        assert D.same_bits(ours[name], ref[name]), name
    phi = D.acf(ref["M"], 3)
    assert phi.tolist() == [1.0, -1.0, 1.0, -1.0]


def test_the_totals_tree_is_a_sum():
    rng = np.random.default_rng(2)
    for n in (0, 1, 255, 256, 257, 1000):
        v = rng.normal(size=(3, n))
        got = D.tree_sum(v)
        for x in range(3):
            assert abs(got[x] - math.fsum(v[x])) <= (D.W_TOTAL + 3) * D.EPS * np.abs(v[x]).sum()
    assert D.tree_sum(np.arange(1000.0)) == 499500.0
