"""
tests/segment_exact.py checked without a GPU: against arithmetic done one Fraction step at a time (each step rounded by
float(), which rounds correctly), against the oracle and the golden within DESIGN §2's tolerances, and for teeth: on the
data the GPU tests use, the stated order gives other bits than np.add.reduceat, than fused products, and than a type
sum in one pass or by np.sum, so that bit-equality on the GPU pins the order.
"""
from fractions import Fraction as Q

import numpy as np
import pytest

import segment_exact as X
from conftest import sorted_frame
from oracle import cpu_ref as O


def _rd(x):
    return float(x)  # (Fraction -> float rounds to nearest even)


def com_steps(attr, mass, off, fused=False):
    """One Fraction per IEEE operation; fused=True adds each product unrounded (an fma)."""
    F, K, _ = attr.shape
    M = len(off) - 1
    out = np.zeros((F, K, M))
    for s in range(M):
        msum = 0.0
        for a in range(off[s], off[s + 1]):
            msum = _rd(Q(msum) + Q(mass[a]))
        for f in range(F):
            for k in range(K):
                acc = 0.0
                for a in range(off[s], off[s + 1]):
                    p = Q(attr[f, k, a]) * Q(mass[a])
                    acc = _rd(Q(acc) + (p if fused else Q(_rd(p))))
                out[f, k, s] = _rd(Q(acc) / Q(msum))
    return out


def type_sum_steps(tmp, seg_type, n_types):
    F = tmp.shape[0]
    out = np.zeros((3, n_types, F))
    for t, (lo, hi) in enumerate(zip(*X.type_runs(seg_type, n_types))):
        for f in range(F):
            for k in range(3):
                red = [0.0] * 256
                for i in range(hi - lo):
                    red[i % 256] = _rd(Q(red[i % 256]) + Q(tmp[f, k, lo + i]))
                w = 128
                while w:
                    for i in range(w):
                        red[i] = _rd(Q(red[i]) + Q(red[i + w]))
                    w //= 2
                out[k, t, f] = red[0]
    return out


def test_com_and_sums_equal_fraction_steps():
    rng = np.random.default_rng(3)
    for sizes in (np.array([1]), np.array([2, 1, 5]), rng.integers(1, 14, 25), np.array([40, 3, 1, 17])):
        off = X.offsets(sizes)
        m, q = X.gen_masses(rng, int(off[-1]))
        attr = X.gen_attr(rng, 2, 3, off)
        np.testing.assert_array_equal(X.com(attr, m, off), com_steps(attr, m, off))
        msum, qsum = X.seg_sums(m, q, off)
        for s in range(len(sizes)):
            mm = qq = 0.0
            for a in range(off[s], off[s + 1]):
                mm, qq = _rd(Q(mm) + Q(m[a])), _rd(Q(qq) + Q(q[a]))
            assert (msum[s], qsum[s]) == (mm, qq)


def test_flux_equals_fraction_steps():
    sizes, st, T = X.type_table()
    off = X.offsets(sizes)
    m, q = X.case_masses("types", off)
    vel = X.case_vel("types", off, 2)
    tmp = X.mol_flux(vel, m, q, off)
    vcom = com_steps(vel, m, off)
    _, qsum = X.seg_sums(m, q, off)
    qsi = np.array([_rd(Q(v) * Q(X.CHARGE_CONV)) for v in qsum])
    want = np.array([[[_rd(Q(_rd(Q(vcom[f, k, s]) * Q(X.VEL_CONV))) * Q(qsi[s])) for s in range(len(sizes))]
                      for k in range(3)] for f in range(2)])
    np.testing.assert_array_equal(tmp, want)
    np.testing.assert_array_equal(X.type_sum(tmp, st, T), type_sum_steps(tmp, st, T))
    np.testing.assert_array_equal(X.flux(vel, m, q, off, st, T), type_sum_steps(tmp, st, T))
    # the types hold 0, 1, 255, 256, 257, 0 and 600 molecules; the empty ones are 0
    assert sorted(np.bincount(st, minlength=T).tolist()) == [0, 0, 1, 255, 256, 257, 600]
    assert (X.flux(vel, m, q, off, st, T)[:, [0, 5]] == 0).all()


@pytest.mark.parametrize("name", sorted(X.segment_tables()))
def test_against_oracle(name):
    """COM rtol 1e-13 and charge flux rtol 1e-9, atol 1e-25 against the reference's arithmetic."""
    off = X.offsets(X.segment_tables()[name])
    m, q = X.case_masses(name, off)
    attr = X.case_attr(name, off, X.FRAMES, 3)
    vel = X.case_vel(name, off, X.FRAMES)
    st, T = X.seg_types(len(off) - 1)
    got, got_j = X.com(attr, m, off), X.flux(vel, m, q, off, st, T)
    msum, qsum = X.seg_sums(m, q, off)
    for f in range(X.FRAMES):
        ref, ref_m, ref_q = O.calc_com(attr[f].T, m, off, q)
        np.testing.assert_allclose(got[f].T, ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(msum, ref_m, rtol=1e-14)
        np.testing.assert_allclose(qsum, ref_q, rtol=1e-12, atol=1e-14)
        ref_j = O.charge_flux(vel[f].T, q, m, off, st + 1, T, X.VEL_CONV, X.CHARGE_CONV)
        np.testing.assert_allclose(got_j[:, :, f], ref_j, rtol=1e-9, atol=1e-25)


def test_against_golden(g_small):
    g = g_small
    cols = list(g["columns"])
    fr = np.stack([sorted_frame(f, cols.index("id")) for f in g["frames"]])
    pick = lambda names: np.ascontiguousarray(fr[:, :, [cols.index(c) for c in names]].transpose(0, 2, 1))  # noqa: E731
    _, _, off, seg_type = O.molecule_layout(g["num_mols"], g["num_atoms_per_mol"])
    amass = g["mass"][fr[0][:, cols.index("type")].astype(np.int64) - 1]
    ref = g["calc_com_xu"]
    np.testing.assert_allclose(X.com(pick(("xu", "yu", "zu")), amass, off)[0].T, ref[:, 2:5], rtol=1e-13)
    np.testing.assert_allclose(X.seg_sums(amass, None, off)[0], ref[:, 5], rtol=1e-14)
    j = X.flux(pick(("vx", "vy", "vz")), amass, fr[0][:, cols.index("q")], off, (seg_type - 1).astype(np.int32), 3,
               10 ** -10 / 10 ** -15, 1.602176634 * 10 ** -19)
    np.testing.assert_allclose(j, g["cond_j"], rtol=1e-9, atol=1e-25)


# ------------------------------------------------------------------------------------------------------------ teeth
def _gpu_cases():
    for name, sizes in sorted(X.segment_tables().items()):
        yield name, X.offsets(sizes)


@pytest.mark.parametrize("name", sorted(X.segment_tables()))
def test_teeth_reduceat_and_fused_products_differ(name):
    """On every table's GPU data the stated order differs somewhere from np.add.reduceat and from fused products."""
    off = X.offsets(X.segment_tables()[name])
    m, _ = X.case_masses(name, off)
    for K in X.N_ATTR:
        attr = X.case_attr(name, off, X.FRAMES, K)
        want = X.com(attr, m, off)
        alt = np.add.reduceat(attr * m, off[:-1], axis=2) / np.add.reduceat(m, off[:-1])
        assert (alt != want).any(), (name, K)
    # fused: on the first frames of the three-plane data (the Fraction loop is slow; small tables get every frame)
    attr = X.case_attr(name, off, X.FRAMES, 3)
    sub = attr[:1] if off[-1] > 100 else attr
    assert (com_steps(sub, m, off, fused=True) != X.com(sub, m, off)).any(), name
    vel = X.case_vel(name, off, X.FRAMES)
    alt = np.add.reduceat(vel * m, off[:-1], axis=2) / np.add.reduceat(m, off[:-1])
    assert (alt != X.com(vel, m, off)).any(), name


def _single_pass(tmp, seg_type, n_types):
    out = np.zeros((3, n_types, tmp.shape[0]))
    for t, (lo, hi) in enumerate(zip(*X.type_runs(seg_type, n_types))):
        acc = np.zeros(tmp.shape[:2])
        for s in range(lo, hi):
            acc = acc + tmp[:, :, s]
        out[:, t] = acc.T
    return out


def _np_sum(tmp, seg_type, n_types):
    lo, hi = X.type_runs(seg_type, n_types)
    return np.stack([np.sum(tmp[:, :, a:b], axis=2).T for a, b in zip(lo, hi)], axis=1)


def test_teeth_type_sum_order_differs():
    """The fixed tree of type_sum_kernel differs from one sequential pass and from np.sum on the flux data: on the type
    table in each type of 255 molecules or more, and on every segment table with a type of three molecules or more."""
    sizes, st, T = X.type_table()
    off = X.offsets(sizes)
    m, q = X.case_masses("types", off)
    tmp = X.mol_flux(X.case_vel("types", off, X.FRAMES), m, q, off)
    want = X.type_sum(tmp, st, T)
    for alt in (_single_pass(tmp, st, T), _np_sum(tmp, st, T)):
        np.testing.assert_allclose(alt, want, rtol=1e-9, atol=1e-25)
        for t in (2, 3, 4, 6):
            assert (alt[:, t] != want[:, t]).any(), t
    for name, off in _gpu_cases():
        M = len(off) - 1
        st, T = X.seg_types(M)
        if np.bincount(st).max() < 3:
            continue
        m, q = X.case_masses(name, off)
        tmp = X.mol_flux(X.case_vel(name, off, X.FRAMES), m, q, off)
        want = X.type_sum(tmp, st, T)
        for alt in (_single_pass(tmp, st, T), _np_sum(tmp, st, T)):
            assert (alt != want).any(), name


def test_teeth_edge_geometry_moves_counts():
    """The adversarial geometry of the molecular-histogram test: sites from np.add.reduceat's COM land in other bins
    and on the other side of a CN cutoff than sites from the stated order."""
    from oracle import cref as C

    g = X.edge_geometry()
    off = g["off"]
    sites = X.com(g["attr"], g["mass"], off)[0]
    alt = (np.add.reduceat(g["attr"] * g["mass"], off[:-1], axis=2) / np.add.reduceat(g["mass"], off[:-1]))[0]
    res = []
    for s in (sites, alt):
        part, ov = C.rdf_rect(g["xyz"][0], g["types"], s, g["site_types"], g["rel"], g["lengths"], g["r_cut"] ** 2,
                              g["ddr"], g["nbins"])
        cn = C.cn_rect(g["xyz"][0], g["types"], s, g["site_types"], g["rel"], g["lengths"],
                       [c * c for c in g["cn_cut"]])
        res.append((part, cn))
    assert (res[0][0] != res[1][0]).any() and (res[0][1] != res[1][1]).any()
