"""
Non-finite input on the CPU side (tests/nonfinite_cases.py has the patterns; the GPU side is tests/test_gpu_nonfinite.py).

- The C oracle and oracle/cpu_ref.py agree with each other on every poison pattern at every placement, for RDF, CN and
  the rectangular atoms x sites forms, and both give the integers of the frame with the poisoned atoms DELETED — a
  statement that needs no NaN arithmetic at all.
- The numpy restatements the GPU tests compare against (cluster_ref, config_ref, aggregates_ref, residence_design) drop
  a poisoned pair and keep every other row.
- The native dump reader and the pandas route give the same frames for dumps that hold nan, -nan, inf and -inf.
"""
import warnings

import numpy as np
import pytest

import aggregates_ref as AR
import cluster_ref as CR
import config_ref as CFG
import nonfinite_cases as NF
import residence_design as RD
from oracle import cpu_ref as O
from oracle import cref as C

N, L = 300, np.array([12.0, 12.5, 13.0])
R_CUT, DDR, NB = 5.0, 0.05, 100
REL = np.array([[1, 1], [1, 2], [2, 3], [3, 3]])
CUTS = [2.5, 3.5, 5.0, 4.0]
TY = (1 + np.arange(N) % 3).astype(np.int32)


@pytest.fixture(autouse=True)
def _quiet():
    """inf - inf and NaN comparisons are the subject here, not an accident."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


@pytest.fixture(scope="module")
def frame():
    return NF.uniform_frames(7001, 1, N, L)[0]


def _data(x, ty):
    return np.column_stack([ty, x.T])


def _neighbours(x, atoms, rc2):
    """Every atom of `atoms` has a neighbour inside the cutoff in the clean frame."""
    for a in atoms:
        r = CR.rsq(x[:, a], x, L)
        r[a] = np.inf
        assert (r < rc2).any(), a


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_rdf_and_cn_oracles_agree_and_equal_the_deleted_frame(frame, pattern):
    clean = C.rdf_pairs(frame, TY, REL, L, R_CUT * R_CUT, DDR, NB)
    clean_cn = C.cn_pairs(frame, TY, REL, L, [c * c for c in CUTS])
    for place in NF.places(N):
        atoms = NF.atoms_of(pattern, place, N)
        _neighbours(frame, atoms, min(CUTS) ** 2)
        bad = NF.poison(frame, pattern, atoms)
        gone, ty_gone = NF.delete(frame, TY, atoms)
        cf, cp, cov = C.rdf_pairs(bad, TY, REL, L, R_CUT * R_CUT, DDR, NB)
        of, op, oov = O.rdf_pairs(_data(bad, TY), REL, L, R_CUT, DDR, NB)
        df, dp, dov = C.rdf_pairs(gone, ty_gone, REL, L, R_CUT * R_CUT, DDR, NB)
        msg = "%s at %s" % (pattern, atoms)
        np.testing.assert_array_equal(cf, of, err_msg=msg)
        np.testing.assert_array_equal(cp, op, err_msg=msg)
        np.testing.assert_array_equal(cf, df, err_msg=msg)
        np.testing.assert_array_equal(cp, dp, err_msg=msg)
        assert cov == oov == dov
        assert not np.array_equal(cf, clean[0]), msg  # the poison took pairs away
        ccn = C.cn_pairs(bad, TY, REL, L, [c * c for c in CUTS])
        np.testing.assert_array_equal(ccn, O.cn_pairs(_data(bad, TY), REL, L, CUTS), err_msg=msg)
        np.testing.assert_array_equal(ccn, C.cn_pairs(gone, ty_gone, REL, L, [c * c for c in CUTS]), err_msg=msg)
        assert not np.array_equal(ccn, clean_cn), msg


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
@pytest.mark.parametrize("side", ["atom", "site"])
def test_atoms_x_sites_oracles_agree_and_equal_the_deleted_frame(frame, pattern, side):
    M = 90
    sites = NF.uniform_frames(7002, 1, M, L)[0]
    sites[:, :10] = frame[:, :10]  # coincident points: rsq == 0
    st = (1 + np.arange(M) % 2).astype(np.int32)
    rel = np.array([[1, 1], [2, 2], [3, 1], [3, 2]])
    n = N if side == "atom" else M
    clean = C.rdf_rect(frame, TY, sites, st, rel, L, R_CUT * R_CUT, DDR, NB)[0]
    for place in NF.places(n):
        atoms = NF.atoms_of(pattern, place, n)
        x, ty, s, sty = frame, TY, sites, st
        if side == "atom":
            bad_x, bad_s = NF.poison(frame, pattern, atoms), sites
            x, ty = NF.delete(frame, TY, atoms)
        else:
            bad_x, bad_s = frame, NF.poison(sites, pattern, atoms)
            s, sty = NF.delete(sites, st, atoms)
        cp, cov = C.rdf_rect(bad_x, TY, bad_s, st, rel, L, R_CUT * R_CUT, DDR, NB)
        op, oov = O.rdf_mol_pairs(_data(bad_x, TY), _data(bad_s, st), rel, L, R_CUT, DDR, NB)
        dp, dov = C.rdf_rect(x, ty, s, sty, rel, L, R_CUT * R_CUT, DDR, NB)
        msg = "%s %s at %s" % (side, pattern, atoms)
        np.testing.assert_array_equal(cp, op, err_msg=msg)
        np.testing.assert_array_equal(cp, dp, err_msg=msg)
        assert cov == oov == dov
        assert not np.array_equal(cp, clean), msg
        ccn = C.cn_rect(bad_x, TY, bad_s, st, rel, L, [c * c for c in CUTS])
        np.testing.assert_array_equal(ccn, O.cn_mol_pairs(_data(bad_x, TY), _data(bad_s, st), rel, L, CUTS), err_msg=msg)
        np.testing.assert_array_equal(ccn, C.cn_rect(x, ty, s, sty, rel, L, [c * c for c in CUTS]), err_msg=msg)


# ------------------------------------------------------------------------------------------------ the restatements
def _molecules(n, size=3):
    mol_of = (np.arange(n) // size).astype(np.int32)
    seg_off = np.arange(0, n + 1, size).astype(np.int64)
    return mol_of, seg_off


def _far(x, atoms):
    """The finite stand-in of a deleted atom in a frame that keeps its indices: the atoms moved to where nothing is
    within any cutoff used here (the frames below fill [0, 12) of a 60 A box; 30 and 38 are 18 or more from every image
    of that, and 8 from each other; the cutoffs are at most 4)."""
    y = x.copy()
    for k, a in enumerate(atoms):
        y[:, a] = 30.0 + 8.0 * k
    return y


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_cluster_and_configuration_restatements_drop_the_poisoned_atom_only(pattern):
    n, box = 300, np.array([60.0, 60.0, 60.0])
    x = NF.uniform_frames(7003, 1, n, 12.0)[0]
    mol_of, seg_off = _molecules(n)
    mol_type = (1 + np.arange(len(seg_off) - 1) % 2).astype(np.int32)
    cls = (np.arange(n) % 3).astype(np.uint8)
    centres = np.array([0, 5, 64, 150, 299])
    rs, rc = 4.0 ** 2, 3.0 ** 2
    for place in NF.places(n):
        atoms = NF.atoms_of(pattern, place, n)
        bad, far = NF.poison(x, pattern, atoms), _far(x, atoms)
        for p in centres:
            got = CR.shell(bad, box, p, mol_of, rs)
            if p in atoms:
                # a non-finite centre has no shell, not even its own molecule (NaN - NaN, inf - inf); the finite 1e300 is
                # at distance 0 from itself and from nothing else
                assert list(got) == ([mol_of[p]] if pattern == "huge_finite" else [])
            else:
                np.testing.assert_array_equal(got, CR.shell(far, box, p, mol_of, rs))
        ok = [p for p in centres if p not in atoms]
        a = CFG.coordination_rows(bad[None], box[None], ok, mol_of, seg_off, mol_type, cls, rs, rc)
        b = CFG.coordination_rows(far[None], box[None], ok, mol_of, seg_off, mol_type, cls, rs, rc)
        assert a == b
        assert a != CFG.coordination_rows(x[None], box[None], ok, mol_of, seg_off, mol_type, cls, rs, rc) or \
            not any(CR.rsq(x[:, p], x, box)[list(atoms)].min() < rs for p in ok)


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_contact_components_restatement_links_nothing_through_a_poisoned_atom(pattern):
    n, box = 120, np.array([[60.0, 60.0, 60.0]])
    x = NF.uniform_frames(7004, 1, n, 9.0)
    aa, ca, ab, cb, node_of, n_nodes = AR.all_atoms(n)
    cut = np.array([[2.0 ** 2]])
    clean = AR.contact_components(x, box, aa, ca, ab, cb, cut, node_of, n_nodes)
    for place in NF.places(n):
        atoms = NF.atoms_of(pattern, place, n)
        bad = NF.poison(x[0], pattern, atoms)[None]
        lab, ncomp, ncon = AR.contact_components(bad, box, aa, ca, ab, cb, cut, node_of, n_nodes)
        want = AR.contact_components(_far(x[0], atoms)[None], box, aa, ca, ab, cb, cut, node_of, n_nodes)
        np.testing.assert_array_equal(lab, want[0])
        np.testing.assert_array_equal(ncomp, want[1])
        np.testing.assert_array_equal(ncon, want[2])
        for a in atoms:
            assert lab[0, a] == a and (lab[0] == a).sum() == 1  # a component of its own
    assert clean[2][0] > 0


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_residence_design_clears_the_poisoned_frame_of_the_pair_only(pattern):
    """A central atom of group 0 poisoned in frame t*: its b_0 pairs lose frame t* of their presence pattern; the
    brute-force oracle on the poisoned coordinates gives the closed form of that."""
    F = 12
    pats = RD.patterns(F, seed=3)
    groups = [(pats["always"], 2, 3), (pats["periodic"], 1, 2)]
    d = RD.designed(groups, seed=5)
    t_star = 4
    assert groups[0][0][t_star]
    xi = d.xi.copy()
    xi[t_star] = NF.poison(xi[t_star], pattern, (0,))
    if pattern == "two_plus_inf":
        xi[t_star] = NF.poison(xi[t_star], pattern, (0, 1))  # both central atoms of group 0
    k = 2 if pattern == "two_plus_inf" else 1
    h = np.array([O.shell_indicator(xi[f].T, d.xj[f].T, d.box[f], RD.LO ** 2, RD.HI ** 2, False) for f in range(F)])
    p_cleared = groups[0][0].copy()
    p_cleared[t_star] = False
    want = d.counts - k * 3 * RD.acorr(groups[0][0]) + k * 3 * RD.acorr(p_cleared)
    np.testing.assert_array_equal(O.residence_counts(h), want)
    assert int(h.sum()) == d.n_records - 3 * k


# ------------------------------------------------------------------------------------------------ the dump reader
def test_native_and_pandas_readers_agree_on_non_finite_tokens(tmp_path):
    from mdproptools_amd import io as IO

    n = 8
    rng = np.random.default_rng(7005)
    path = str(tmp_path / "blown.dump")
    want = []
    with open(path, "wt") as fh:
        for step in range(3):
            x = rng.uniform(0, 10, (n, 3))
            tok = [["%.6f" % v for v in row] for row in x]
            val = np.array([[float(t) for t in row] for row in tok])
            for k, (text, v) in enumerate(NF.DUMP_TOKENS):
                a, ax = (k + step) % n, (k + step) % 3
                tok[a][ax], val[a, ax] = text, v
            fh.write("ITEM: TIMESTEP\n%d\nITEM: NUMBER OF ATOMS\n%d\nITEM: BOX BOUNDS pp pp pp\n0.0 10.0\n0.0 10.0\n"
                     "0.0 10.0\nITEM: ATOMS id type x y z\n" % (step, n))
            order = rng.permutation(n)
            fh.write("".join("%d %d %s\n" % (i + 1, 1 + i % 2, " ".join(tok[i])) for i in order))
            want.append(val.T)
    cols = ["id", "type", "x", "y", "z"]
    native = IO._native_file_frames(path, cols, "id", 1)
    pandas = IO._pandas_file_frames(path, cols, "id")
    assert len(native) == len(pandas) == 3
    for f in range(3):
        assert native[f][0] == pandas[f][0] == f
        assert NF.same_bits(native[f][4], pandas[f][4])
        assert NF.same_bits(native[f][4][2:], want[f])
        assert np.isnan(native[f][4]).sum() == 3 and np.isinf(native[f][4]).sum() == 3
