"""
mdhip_shell_residence (csrc/residence.hip) at its edges: mask word boundaries, trajectories up to the 65 535-frame cap
(lag tables beyond one LDS window), exact shell bounds and wrap edges, per-frame boxes, both kernel forms (SWAP), device
inputs, pair keys above 2^32, pair tables that overflow and are swept again, and the ResidenceTime drop-in.

Every check is an exact integer comparison (residence counts bit-exact), against the brute-force oracle
(oracle.cpu_ref.shell_indicator + residence_counts) where it is affordable and against the closed-form counts of
designed trajectories (tests/residence_design.py, checked against the oracle in test_residence_design_cpu.py) where not.
"""
import numpy as np
import pytest

import residence_design as RD
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

LO2, HI2 = RD.LO * RD.LO, RD.HI * RD.HI


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _check(B, d, same=False, want=None):
    """The kernel on a design (cross: xi / xj; same: one set with exclude_diagonal) against `want` (default: the
    design's closed form), counts AND n_records exactly."""
    counts, nrec = B.shell_residence(d.xi, d.xj, d.box, LO2, HI2, exclude_diagonal=same)
    want_c, want_n = want if want is not None else (d.counts, d.n_records)
    np.testing.assert_array_equal(counts.astype(np.int64), want_c)
    assert nrec == want_n
    return counts, nrec


def _oracle(xi, xj, box, lo2, hi2, same=False):
    F = xi.shape[0]
    h = np.array([O.shell_indicator(xi[f].T, xj[f].T, box[f], lo2, hi2, same) for f in range(F)])
    return O.residence_counts(h), int(h.sum())


def _edge_groups(F, seed, scale=1):
    p = RD.patterns(F, seed=seed)
    return [(p["always"], 2 * scale, 1), (p["run"], 1, 2 * scale), (p["periodic"], 3, 2), (p["random"], 2, 3),
            (p["ends"], 1, 1), (p["never"], 2, 2)]


# ------------------------------------------------------------------ mask words
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
def test_mask_word_boundaries(B, F):
    """Frame counts on either side of a 64-frame mask word, every pattern (a pair present only in the first and the
    last frame sets the first and the last bit of its mask), against the brute-force oracle and the closed form."""
    for same in (False, True):
        d = RD.designed(_edge_groups(F, seed=F), seed=F, same=same)
        want = RD.oracle_counts(d, same=same)
        np.testing.assert_array_equal(want[0], d.counts)
        _check(B, d, same, want)


# ------------------------------------------------------------------ long trajectories: lag windows
@pytest.mark.parametrize("F", [8200, 20100, 30000, 65535])
def test_long_trajectories(B, F):
    """8 200 frames: the first lag table above 64 KB of LDS; 20 100: the last that fits one 160 KB window (one
    launch, as for every shorter trajectory); 30 000 and 65 535 (the cap): several lag windows over 470 / 1024-word
    masks."""
    d = RD.designed(_edge_groups(F, seed=F), seed=F)
    _check(B, d)
    # the same-set form of the relation (one array, diagonal excluded), with different group sizes
    d = RD.designed(_edge_groups(F, seed=F + 1, scale=2)[:5], seed=F + 1, same=True)
    _check(B, d, same=True)


def test_host_refusals(B):
    """Refused on the host before any launch: more than 65 535 frames; exclude_diagonal with different set sizes."""
    from mdproptools_amd._lib import MdhipError

    x = np.zeros((65536, 3, 1))
    with pytest.raises(MdhipError, match="65535"):
        B.shell_residence(x, x, np.full((65536, 3), 10.0), LO2, HI2)
    p = RD.patterns(10, seed=1)
    d = RD.designed([(p["always"], 3, 1), (p["periodic"], 2, 2)], seed=1)
    assert d.xi.shape[2] != d.xj.shape[2]
    with pytest.raises(MdhipError, match="exclude_diagonal"):
        B.shell_residence(d.xi, d.xj, d.box, LO2, HI2, exclude_diagonal=True)
    # the context is still usable
    _check(B, d)


# ------------------------------------------------------------------ shell bounds and wrap, brute-force oracle
def _one_case_per_frame(disp, L, start=(0.0, 0.0, 0.0), central_shift=None):
    """One central atom and one shell atom per frame, the shell atom at central - disp[f] (the kernel and the
    reference subtract the shell atom from the central one); central_shift [F,3] then moves the central atoms by whole
    box lengths. -> xi [F,3,1], xj [F,3,1], box [F,3]."""
    disp = np.asarray(disp, dtype=np.float64)
    F = len(disp)
    xi = np.tile(np.asarray(start, dtype=np.float64), (F, 1))
    xj = xi - disp
    assert np.array_equal(xi - xj, disp)  # the differences are exact: the kernel sees disp itself
    if central_shift is not None:
        xi = xi + central_shift
    box = np.tile(np.asarray(L, dtype=np.float64), (F, 1))
    return np.ascontiguousarray(xi[:, :, None]), np.ascontiguousarray(xj[:, :, None]), box


def test_shell_bounds_exact(B):
    """rsq exactly on lo^2 is out, exactly on hi^2 is in (shell (3, 6]: 2^2 + 2^2 + 1^2 = 9, 4^2 + 4^2 + 2^2 = 36, all
    exact in binary), a component a few ulps either side, negative coordinates, central atoms whole boxes away."""
    L = np.array([32.0, 40.0, 48.0])
    e = 2.0 ** -26
    on_lo = [(2, 2, 1), (-2, 2, -1), (3, 0, 0), (0, -3, 0), (0, 0, 3)]
    on_hi = [(4, 4, 2), (-4, -4, 2), (6, 0, 0), (0, 6, 0), (0, 0, -6)]
    near = [(2, 2, 1 + e), (2, 2, 1 - e), (4, 4, 2 + e), (4, 4, 2 - e), (6 + e, 0, 0), (3 - e, 0, 0), (3 + e, 0, 0),
            (1.5, 1.5, 1.5), (5, 5, 5), (0, 0, 0)]
    base = on_lo + on_hi + near
    disp = np.array(base * 3, dtype=np.float64)
    F = len(disp)
    lo_idx = np.isin(np.arange(F) % len(base), np.arange(len(on_lo)))
    hi_idx = np.isin(np.arange(F) % len(base), len(on_lo) + np.arange(len(on_hi)))
    rng = np.random.default_rng(5)
    for start, shift in [((10.0, 10.0, 10.0), None), ((-7.5, -13.25, -0.5), None),
                         ((10.0, 10.0, 10.0), rng.integers(-1, 2, (F, 3)) * L)]:
        xi, xj, box = _one_case_per_frame(disp, L, start, shift)
        rsq = np.array([O.min_image_rsq(xi[f, :, 0], xj[f, :, 0], L) for f in range(F)])
        assert (rsq[lo_idx] == 9.0).all() and (rsq[hi_idx] == 36.0).all()  # the premise: exactly on the bounds
        want = _oracle(xi, xj, box, 9.0, 36.0)
        hits = (rsq > 9.0) & (rsq <= 36.0)
        assert want[1] == int(hits.sum()) and not hits[lo_idx].any() and hits[hi_idx].all()
        counts, nrec = B.shell_residence(xi, xj, box, 9.0, 36.0)
        np.testing.assert_array_equal(counts.astype(np.int64), want[0])
        assert nrec == want[1]


def test_wrap_edges(B):
    """Displacements of exactly +-L/2 and one ulp either side (the single wrap is strict: |d| > L/2), with lo^2 = (L/2)^2
    so that a missing or a non-strict wrap moves a count; displacements in (1.5 L, 2.5 L), which the reference's single
    shift leaves out of the shell although their minimum image is inside it."""
    L = np.array([12.0, 16.0, 20.0])
    cases = []
    for ax in range(3):
        h = L[ax] / 2
        for v in (h, -h, np.nextafter(h, 0), np.nextafter(h, 99), -np.nextafter(h, 0), -np.nextafter(h, 99)):
            d = [0.0, 0.0, 0.0]
            d[ax] = v
            cases.append(d)
    disp = np.array(cases * 2)
    xi, xj, box = _one_case_per_frame(disp, L, (0.0, 0.0, 0.0))
    for lo2, hi2 in [(36.0, 100.0), (0.0, 36.0), (64.0, 100.0), (0.0, 64.0), (100.0, 400.0), (0.0, 100.0)]:
        want = _oracle(xi, xj, box, lo2, hi2)
        counts, nrec = B.shell_residence(xi, xj, box, lo2, hi2)
        np.testing.assert_array_equal(counts.astype(np.int64), want[0])
        assert nrec == want[1]
    # beyond 1.5 L: the minimum image is 2 A away, the reference's single shift leaves L + ... : never counted
    far = []
    for ax in range(3):
        for k in (1.5 + 1 / 8, 2.0, 2.5 - 1 / 8):
            for sgn in (1, -1):
                d = [0.0, 0.0, 0.0]
                d[ax] = sgn * (k * L[ax] + (2.0 if k == 2.0 else 0.0))
                far.append(d)
    xi, xj, box = _one_case_per_frame(np.array(far), L, (1.0, -3.0, 5.0))
    want = _oracle(xi, xj, box, 0.0, 9.0)
    assert want[1] == 0  # the single shift leaves every one of them outside
    counts, nrec = B.shell_residence(xi, xj, box, 0.0, 9.0)
    np.testing.assert_array_equal(counts.astype(np.int64), want[0])
    assert nrec == 0
    # the same pairs one box length closer are inside: the kernel does see them
    near = np.array(far) - np.sign(np.array(far)) * L[None, :] * (np.abs(np.array(far)) > 0)
    xi, xj, box = _one_case_per_frame(near, L, (1.0, -3.0, 5.0))
    want = _oracle(xi, xj, box, 0.0, 9.0)
    assert want[1] == 6  # the 2 A images of the k = 2 cases
    counts, nrec = B.shell_residence(xi, xj, box, 0.0, 9.0)
    np.testing.assert_array_equal(counts.astype(np.int64), want[0])
    assert nrec == want[1]


def test_per_frame_box(B):
    """NPT: every frame wraps with its own box; frame 0's box is the largest (the pair table's estimate reads frame 0
    only, so it is too low). A pair sits L_f - 3 apart along x (in the shell (2, 4] only under its own frame's L), a
    decoy L_0 - 3 apart (in it only in frame 0 and wherever that frame's wrap happens to land inside)."""
    F = 90
    Lx = 40.0 - 0.25 * np.arange(F)  # exact, decreasing: frame 0 the largest
    box = np.stack([Lx, 30.0 - 0.125 * np.arange(F), np.full(F, 25.0)], axis=1)
    rng = np.random.default_rng(11)
    n_i, n_j = 24, 40
    xi = rng.uniform(0, 1, (1, 3, n_i)) * box[0][None, :, None] + np.cumsum(rng.normal(0, 0.2, (F, 3, n_i)), axis=0)
    xj = rng.uniform(0, 1, (1, 3, n_j)) * box[0][None, :, None] + np.cumsum(rng.normal(0, 0.2, (F, 3, n_j)), axis=0)
    xj[:, :, 0] = xi[:, :, 0] - np.stack([Lx - 3.0, np.zeros(F), np.zeros(F)], axis=1)
    xj[:, :, 1] = xi[:, :, 1] - np.stack([np.full(F, Lx[0] - 3.0), np.zeros(F), np.zeros(F)], axis=1)
    xi, xj = np.ascontiguousarray(xi), np.ascontiguousarray(xj)
    for lo, hi in [(2.0, 4.0), (0.0, 6.0)]:
        h = np.array([O.shell_indicator(xi[f].T, xj[f].T, box[f], lo * lo, hi * hi, False) for f in range(F)])
        if lo == 2.0:
            assert h[:, 0, 0].all() and h[0, 1, 1] and not h[1:, 1, 1].all()
        counts, nrec = B.shell_residence(xi, xj, box, lo * lo, hi * hi)
        np.testing.assert_array_equal(counts.astype(np.int64), O.residence_counts(h))
        assert nrec == int(h.sum())


# ------------------------------------------------------------------ symmetry: both kernel forms
def test_symmetry_both_kernel_forms(B):
    """h is symmetric in (i, j): shell_residence(xj, xi) == shell_residence(xi, xj) bit for bit, on shapes where
    either set is the larger one (the larger set goes on the lanes: both SWAP forms of shell_pairs_kernel run on the
    same data)."""
    F = 150
    p = RD.patterns(F, seed=2)
    for groups in ([(p["always"], 40, 3), (p["periodic"], 30, 2), (p["random"], 300, 1), (p["ends"], 5, 2)],
                   [(p["always"], 3, 40), (p["run"], 2, 300), (p["random"], 1, 7)]):
        d = RD.designed(groups, seed=2)
        a = _check(B, d)
        b = B.shell_residence(d.xj, d.xi, d.box, LO2, HI2)
        np.testing.assert_array_equal(b[0], a[0])
        assert b[1] == a[1]
    # random walkers in a dense box, against the oracle as well
    rng = np.random.default_rng(17)
    L = np.array([11.0, 12.0, 13.0])
    r = rng.uniform(0, 1, (1, 3, 340)) * L[None, :, None] + np.cumsum(rng.normal(0, 0.15, (F, 3, 340)), axis=0)
    xi, xj, box = np.ascontiguousarray(r[:, :, :40]), np.ascontiguousarray(r[:, :, 40:]), np.tile(L, (F, 1))
    want = _oracle(xi, xj, box, 1.0, 20.25)
    for x1, x2 in ((xi, xj), (xj, xi)):
        counts, nrec = B.shell_residence(x1, x2, box, 1.0, 20.25)
        np.testing.assert_array_equal(counts.astype(np.int64), want[0])
        assert nrec == want[1]


# ------------------------------------------------------------------ inputs
def test_device_inputs_and_aliasing(B):
    """Torch device tensors (both, or one of the two) give what host arrays give; `xi is xj` with exclude_diagonal
    gives what equal data in two separate arrays gives."""
    import torch

    F = 200
    d = RD.designed(_edge_groups(F, seed=4), seed=4)
    host = _check(B, d)
    ti = torch.from_numpy(d.xi).to("cuda")
    tj = torch.from_numpy(d.xj).to("cuda")
    for a, b in ((ti, tj), (ti, d.xj), (d.xi, tj)):
        counts, nrec = B.shell_residence(a, b, d.box, LO2, HI2)
        np.testing.assert_array_equal(counts, host[0])
        assert nrec == host[1]
    s = RD.designed(_edge_groups(F, seed=5), seed=5, same=True)
    one = _check(B, s, same=True)
    two = B.shell_residence(s.xi, s.xi.copy(), s.box, LO2, HI2, exclude_diagonal=True)
    np.testing.assert_array_equal(two[0], one[0])
    assert two[1] == one[1]
    ts = torch.from_numpy(s.xi).to("cuda")
    dev = B.shell_residence(ts, ts, s.box, LO2, HI2, exclude_diagonal=True)
    np.testing.assert_array_equal(dev[0], one[0])
    assert dev[1] == one[1]
    # the diagonal itself: with lo = 0 and rsq = 0 it is outside the shell anyway; with lo^2 < 0 only the flag drops it
    cnt, n = B.shell_residence(s.xi, s.xi, s.box, -1.0, HI2, exclude_diagonal=True)
    cnt2, n2 = B.shell_residence(s.xi, s.xi.copy(), s.box, -1.0, HI2, exclude_diagonal=False)
    n_atoms = s.xi.shape[2]
    assert n2 - n == n_atoms * F
    np.testing.assert_array_equal(cnt2.astype(np.int64) - cnt.astype(np.int64), n_atoms * (F - np.arange(F)))


# ------------------------------------------------------------------ 64-bit pair keys
def test_pair_keys_above_2_32(B):
    """68 921 central and 68 921 shell atoms (a 41^3 lattice, 3 A apart, box 123 A, shell (0.5, 1.5]): shell atom j
    sits 1 A from central atom j. Keys i * n_j + j reach 4.75e9. Shell atom m + 17 339 moves next to central atom
    m + 62 317 in frames 0 and 2: keys (m, m) and (m + 62 317, m + 17 339) differ by exactly 2^32, so a table that
    truncated keys would merge the two pairs."""
    n, F, m = 41 ** 3, 3, 1000
    assert 62317 * n + 17339 == 1 << 32
    g = np.stack(np.unravel_index(np.arange(n), (41, 41, 41))).astype(np.float64) * 3.0 + 1.5  # [3, n]
    xi = np.ascontiguousarray(np.broadcast_to(g, (F, 3, n)))
    xj = np.repeat((g + np.array([[1.0], [0.0], [0.0]]))[None], F, axis=0)
    i_s, j_s = m + 62317, m + 17339
    xj[[0, 2], :, j_s] = g[:, i_s] + np.array([0.0, 1.0, 0.0])
    xj = np.ascontiguousarray(xj)
    box = np.full((F, 3), 123.0)
    counts, nrec = B.shell_residence(xi, xj, box, 0.25, 2.25)
    # (n - 1) pairs (j, j) in all three frames, (j_s, j_s) in frame 1 only, (i_s, j_s) in frames 0 and 2
    want = (n - 1) * np.array([3, 2, 1]) + np.array([1, 0, 0]) + np.array([2, 0, 1])
    np.testing.assert_array_equal(counts.astype(np.int64), want)
    assert nrec == 3 * n
    # the oracle on the rows that hold every in-shell pair of the moved atoms
    rows = [m, j_s, i_s]
    h = np.array([O.shell_indicator(xi[f].T[rows], xj[f].T, box[f], 0.25, 2.25, False) for f in range(F)])
    assert h.sum() == 3 + 1 + 5 and h[:, 0, m].all() and h[[0, 2], 2, j_s].all() and h[1, 1, j_s]


# ------------------------------------------------------------------ pair tables that overflow: the re-sweep
def test_natural_overflow_resweep(B):
    """A clustered system, no option set: 1100 central and 1100 shell atoms all inside one shell for 200 frames in a
    1000 A box. The first table (2^20 slots from the shell's share of the box) cannot hold 1.21e6 pairs; the
    re-sweep is sized from the pairs (2^22 slots, 160 MiB), not from the 2.4e8 hits (2^29 slots, 20 GiB: refused)."""
    F = 200
    p = RD.patterns(F, seed=9)
    d = RD.designed([(p["always"], 1100, 1100), (p["periodic"], 3, 2), (p["ends"], 2, 2), (p["random"], 2, 3),
                     (p["run"], 1, 1)], seed=9, box=(1000.0, 1000.0, 1000.0))
    _check(B, d)


@pytest.mark.parametrize("same", [False, True])
def test_forced_overflow_resweep(B, same):
    """A 64-slot first table (the test option) for ~170 pairs over 16 000 frames (250-word masks): the re-sweep needs
    1024 slots; sized from the 2.4e6 hits it would ask for 2^23 slots x 2 KB = 16 GiB and be refused. The same-set
    form (one array, diagonal excluded) as well."""
    F = 16000
    p = RD.patterns(F, seed=12)
    d = RD.designed([(p["always"], 12, 12), (p["periodic"], 2, 3), (p["ends"], 2, 2), (p["random"], 3, 2),
                     (p["run"], 1, 2)], seed=12, same=same)
    ctx = B.default_context()
    ctx.set_option("residence_cap", 64)
    try:
        _check(B, d, same)
    finally:
        ctx.set_option("residence_cap", 0)
    _check(B, d, same)  # (no option: one sweep)


# ------------------------------------------------------------------ drop-in
def test_residence_time_dropin_npt_pseudo_types(B, tmp_path):
    """ResidenceTime.calc_auto_correlation on synthetic dumps with a box per frame and pseudo-types from num_mols /
    num_atoms_per_mol, a cross-type and a same-type relation: corr_df equals the oracle's autocorrelation of the
    oracle's indicator exactly (the host does the oracle's divisions in the oracle's order)."""
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical.residence_time import ResidenceTime

    num_mols, per_mol = [20, 30], [2, 1]  # pseudo-types 1, 2 (two-atom molecules) and 3 (one-atom molecules)
    n = 20 * 2 + 30
    ids = np.arange(1, n + 1)
    ltype = np.where(ids <= 40, 1, 2)
    F = 48
    rng = np.random.default_rng(23)
    Ls = np.stack([14.0 + 0.25 * (np.arange(F) % 5), 15.0 - 0.125 * (np.arange(F) % 3), np.full(F, 14.5)], axis=1)
    pos = rng.uniform(0, 14.0, (n, 3)) + np.cumsum(rng.normal(0, 0.3, (F, n, 3)), axis=0)
    pos = np.round(pos, 3)  # short decimals: the dump text parses back to these doubles exactly
    cols = ["id", "type", "x", "y", "z"]
    for f in range(F):
        tab = np.column_stack([ids, ltype, pos[f]])
        mio.write_dump(str(tmp_path / ("dump.nvt.%d.dump" % (1000 * f))), 1000 * f, [(0.0, L) for L in Ls[f]], cols, tab)
    r_cut = [[0.0, 4.0], [1.5, 5.0]]
    rt = ResidenceTime(r_cut, [[1, 3], [3, 3]], str(tmp_path / "dump.nvt.*.dump"), dt=2, num_mols=num_mols,
                       num_atoms_per_mol=per_mol, working_dir=str(tmp_path))
    rt.calc_auto_correlation()
    labels = O.calc_atom_type(ids, num_mols, per_mol)
    for (k, l), (lo, hi) in zip([(1, 3), (3, 3)], r_cut):
        sk, sl = np.flatnonzero(labels == k), np.flatnonzero(labels == l)
        h = np.array([O.shell_indicator(pos[f][sk], pos[f][sl], Ls[f], lo ** 2, hi ** 2, k == l) for f in range(F)])
        assert h[0].sum() > 0
        np.testing.assert_array_equal(rt.corr_df["%d-%d" % (k, l)].to_numpy(), O.residence_autocorr(h))
        counts, nrec = B.shell_residence(np.ascontiguousarray(pos[:, sk].transpose(0, 2, 1)),
                                         np.ascontiguousarray(pos[:, sl].transpose(0, 2, 1)), Ls, lo ** 2, hi ** 2,
                                         exclude_diagonal=k == l)
        np.testing.assert_array_equal(counts.astype(np.int64), O.residence_counts(h))
        assert nrec == int(h.sum())
