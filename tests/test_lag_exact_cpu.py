"""
The exact full-lag MSD reference (tests/lag_exact.py) on its own, without a GPU: its sums against brute-force Python
integers, its overflow guard, and its per-lag criterion for the spectral paths — met by a float64 numpy pipeline built the
way the library's is (centred series, padded length 2^m, 3 * 2^m or D * 6144 through residue classes, S1 from
extended-precision prefix sums, S1 - 2 S2) with room to spare, and missed by the same pipeline with one numeric fault
(one spectrum bin of one residue class off by 1e-9, one folded sample dropped).
"""

import numpy as np
import pytest

import lag_exact as X


def brute_sums(xi, max_lag, goff):
    F = xi.shape[0]
    out = np.zeros((max_lag + 1, len(goff) - 1, 3), dtype=object)
    for g in range(len(goff) - 1):
        for e in range(goff[g], goff[g + 1]):
            for a in range(3):
                s = [int(v) for v in xi[:, a, e]]
                for k in range(max_lag + 1):
                    out[k, g, a] += sum((s[t + k] - s[t]) ** 2 for t in range(F - k))
    return out


@pytest.mark.parametrize("F,max_lag,goff", [(2, 1, [0, 1]), (3, 2, [0, 2, 2, 3]), (3, 0, [0, 3]), (17, 16, [0, 1, 4, 4, 5]),
                                            (17, 9, [0, 5]), (40, 13, [0, 0, 2, 5])])
def test_exact_sums_equal_brute_force(F, max_lag, goff):
    rng = np.random.default_rng(F * 100 + max_lag)
    for name, gen in X.GENERATORS.items():
        xi = gen(rng, F, goff[-1] + 1)
        S = X.exact_sums(xi, max_lag, goff)
        assert S.dtype == np.int64 and S.shape == (max_lag + 1, len(goff) - 1, 3)
        assert (S == brute_sums(xi, max_lag, goff)).all(), name
        assert (S[0] == 0).all()


def test_exact_means_round_correctly():
    from fractions import Fraction

    rng = np.random.default_rng(3)
    xi = X.gen_white(rng, 23, 5, amp=1 << 20)
    goff = [0, 3, 3, 4]
    S = X.exact_sums(xi, 22, goff)
    for scale in (1.0, 0.5, 2.0**-33):
        by_sum, by_axes = X.exact_means(S, 23, goff, scale)
        u2 = Fraction(X.UNIT * scale) ** 2
        for k in range(23):
            for g, n in enumerate(np.diff(goff)):
                for a in range(4):
                    s = int(S[k, g].sum()) if a == 3 else int(S[k, g, a])
                    want = float(Fraction(s) * u2 / ((23 - k) * int(n))) if n else 0.0
                    assert by_sum[k, g, a] == want, (k, g, a)
        assert (by_axes[..., 3] == (by_axes[..., 0] + by_axes[..., 1]) + by_axes[..., 2]).all()
        assert (by_sum[..., :3] == by_axes[..., :3]).all() and (by_sum[:, 1] == 0).all()
    # sums past 2^53 go through Python's correctly rounded integer division
    big = np.array([[[(1 << 60) + 1, 3, (1 << 55) - 1]]], np.int64)
    m, _ = X.exact_means(np.concatenate([big, big]), 3, [0, 1])
    assert m[1, 0, 0] == ((1 << 60) + 1) / 2 * X.UNIT**2 and m[1, 0, 3] == ((1 << 60) + (1 << 55) + 3) / 2 * X.UNIT**2


def test_overflow_guard_refuses():
    xi = np.zeros((1000, 3, 4), np.int64)
    xi[::2, 0, :] = 1 << 28  # |x - x[0]| = 2^28: 4 * 1000 * 2^56 * 4 > 2^63
    with pytest.raises(AssertionError, match="overflow"):
        X.exact_sums(xi, 5, [0, 4])
    X.exact_sums(xi[:, :, :1][:10], 5, [0, 1])  # (a short one-entity slice of the same data fits)
    big = np.full((3, 3, 1), 1 << 30, np.int64)
    big[1] = -(1 << 30)
    with pytest.raises(AssertionError, match="overflow"):
        X.exact_sums(np.concatenate([big] * 800), 3, [0, 1])


def test_energy_is_exact():
    rng = np.random.default_rng(5)
    xi = X.gen_walk(rng, 101, 4)
    q = X.energy(xi, [0, 1, 4], 0.5)
    x = xi.astype(np.longdouble)
    c = x - x.mean(axis=0, keepdims=True)
    want = np.stack([(c[:, :, 0:1] ** 2).sum(axis=(0, 2)), (c[:, :, 1:4] ** 2).sum(axis=(0, 2))]) * (X.UNIT * 0.5) ** 2
    np.testing.assert_allclose(q, want.astype(np.float64), rtol=1e-15)


# ------------------------------------------------------------------------------ a float64 numpy spectral pipeline
W12_N = 6144


def _power_by_classes(x, D, fault=None):
    """|X_k|^2, k < L' = D * 6144, of the real series x (len <= L') through residue classes mod D:
    X[D j + r] = FFT_6144(y_r)[j], y_r[n] = w_L'^(r n) sum_q x[n + 6144 q] w_D^(r q) — the decomposition of msd_fft_w12r.h."""
    L = D * W12_N
    xp = np.zeros(L)
    xp[: len(x)] = x
    blocks = xp.reshape(D, W12_N)  # blocks[q, n] = x[n + 6144 q]
    n = np.arange(W12_N)
    P = np.empty(L)
    for r in range(D):
        wq = np.exp(-2j * np.pi * r * np.arange(D) / D)
        terms = blocks * wq[:, None]
        if fault and fault[0] == "drop" and fault[1] == r:
            terms[fault[3], fault[2]] = 0.0  # one sample of the fold of class r lost
        y = terms.sum(axis=0) * np.exp(-2j * np.pi * r * n / L)
        P[r::D] = np.abs(np.fft.fft(y)) ** 2
    return P


def fft_lag_msd(xi, max_lag, goff, L, classes=0, fault=None):
    """Means [K, G, 4] of the float64 pipeline at padded length L (classes = D: through residue classes, L = D * 6144).
    fault: ("bin", r) — the largest bin of class r (and its mirror) scaled by 1 + 1e-9; ("drop", r, n, q) — sample
    n + 6144 q left out of class r's fold."""
    x = X.to_float(xi)
    F, _, E = x.shape
    K, G = max_lag + 1, len(goff) - 1
    k = np.arange(K)
    out = np.zeros((K, G, 4))
    for g in range(G):
        n_g = goff[g + 1] - goff[g]
        if n_g == 0:
            continue
        for a in range(3):
            xs = x[:, a, goff[g]:goff[g + 1]]
            xc = xs - xs.mean(axis=0, keepdims=True)
            q = (xc.astype(np.longdouble) ** 2).sum(axis=1)
            pre = np.concatenate(([0], np.cumsum(q)))
            s1 = (pre[F] - pre[k]) + pre[F - k]
            if classes:
                P = sum(_power_by_classes(xc[:, e], classes, fault) for e in range(n_g))
                if fault and fault[0] == "bin":
                    r = fault[1]
                    j = int(np.argmax(P[r::classes][1:])) + 1
                    for b in {classes * j + r, (L - classes * j - r) % L}:
                        P[b] *= 1 + 1e-9
                s2 = np.fft.ifft(P).real[:K]
            else:
                P = (np.abs(np.fft.rfft(xc, L, axis=0)) ** 2).sum(axis=1)
                s2 = np.fft.irfft(P, L)[:K]
            v = (s1 - 2 * s2.astype(np.longdouble)).astype(np.float64)
            v[0] = 0.0
            out[:, g, a] = v / ((F - k) * n_g)
    out[..., 3] = (out[..., 0] + out[..., 1]) + out[..., 2]
    return out


def _case(name, F, E, seed):
    xi = X.GENERATORS[name](np.random.default_rng(seed), F, E)
    goff = [0, 1, E] if E > 1 else [0, 1]
    return xi, goff


@pytest.mark.parametrize("name", sorted(X.GENERATORS))
def test_numpy_pipeline_meets_the_criterion_with_room(name):
    """numpy's float64 transform stays within half the allowance on every generator at every padded-length form the library
    uses (2^m, 3 * 2^m, residue classes of 4 x 6144); measured 0.03-0.3 x EPS log2 L' 2 Q against the allowance's 8."""
    for F, max_lag, L, D in ((700, 699, 2048, 0), (3000, 2999, 6144, 0), (6145, 6144, 16384, 0), (7000, 6999, 24576, 4)):
        xi, goff = _case(name, F, 3, F)
        S = X.exact_sums(xi, max_lag, goff)
        Q = X.energy(xi, goff)
        got = fft_lag_msd(xi, max_lag, goff, L, classes=D)
        j = X.judge(got, S, Q, F, goff, L)
        assert j["frac"] <= 0.5 and j["ratio"] <= 1.0, (name, F, L, j)


@pytest.mark.parametrize("name", ["walk", "white", "spikes"])
def test_criterion_catches_one_numeric_fault(name):
    """One bin of one residue class off by 1e-9 relative, or one sample missing from one class's fold: the per-lag
    criterion fails although the relative error at most lags stays tiny (what a tolerance tied to min_k S would pass)."""
    F, L, D = 7000, 24576, 4
    xi, goff = _case(name, F, 2, 11)
    S = X.exact_sums(xi, F - 1, goff)
    Q = X.energy(xi, goff)
    clean = X.judge(fft_lag_msd(xi, F - 1, goff, L, classes=D), S, Q, F, goff, L)
    assert clean["frac"] <= 0.5, clean
    for fault in (("bin", 1), ("bin", 2), ("drop", 3, 500, 1), ("drop", 1, 6143, 0)):
        bad = X.judge(fft_lag_msd(xi, F - 1, goff, L, classes=D, fault=fault), S, Q, F, goff, L)
        assert bad["frac"] > 1.0, (name, fault, bad)
