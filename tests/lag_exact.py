"""
Exact host reference for the full-lag MSD (mdhip_lag_msd), no GPU and no torch.

Trajectories are integers `xi [F, 3, E]` (int64); the library is handed x = xi * 2^-10 (float64, exact) and a power-of-two
scale, so every MSD sum is an integer times u^2, u = 2^-10 * scale, and the means have one correctly rounded float64 value:

    S[k, g, a] = sum_{e in g} sum_{t < F - k} (xi[t + k, a, e] - xi[t, a, e])^2          (exact_sums, int64)
    mean[k, g, a] = round(S[k, g, a] * u^2 / ((F - k) * n_g))                            (exact_means)

exact_sums forms S as S1 - 2 S2 (prefix sums of the squares, np.correlate in int64) after subtracting an integer offset
per series, and asserts that no int64 sum can overflow. np.correlate costs O(F * max_lag) per series (0.3 s at F = 24 576,
full lag): keep the entity count small at long F.
"""
import math
from fractions import Fraction

import numpy as np

UNIT = 2.0**-10  # the library sees x = xi * UNIT
EPS = 2.0**-52  # (the library's eps_l = 4 * EPS * log2(L'))
I63 = 1 << 63
I53 = 1 << 53

# fold and region boundaries of the spectral paths (512-point sub-transforms, 1024-point short lengths, the 6144-point
# residue-class transforms and their folds at 12 288 and 24 576)
SPIKE_FRAMES = (0, 511, 512, 1023, 1024, 6143, 6144, 12287, 12288, 24575)


# ---------------------------------------------------------------------------------------------------------- generators
def _walk(rng, F, E, step):
    return np.cumsum(rng.integers(-step, step + 1, (F, 3, E)), axis=0, dtype=np.int64)


def gen_walk(rng, F, E, step=8, offset=1 << 18):
    """Integer random walk (steps uniform in [-step, step]) on a large per-series offset (|x| up to ~2^19 units for the
    default offset): what centring is for."""
    return _walk(rng, F, E, step) + rng.integers(-offset, offset + 1, (1, 3, E))


def gen_white(rng, F, E, amp=1024, offset=1 << 16):
    """Integer white noise: the same energy at every frequency, so every residue class of the spectrum carries its share."""
    return rng.integers(-amp, amp + 1, (F, 3, E)) + rng.integers(-offset, offset + 1, (1, 3, E))


def gen_periodic(rng, F, E, period, amp=512, step=4):
    """A walk with a high-frequency pattern on top: period 2 is the alternating sign (-1)^t, periods 3 and 7 a random
    integer pattern per series (energy at the Nyquist frequency and at L'/3, L'/7)."""
    t = np.arange(F)
    if period == 2:
        pat = np.where(t % 2 == 0, 1, -1)[:, None, None] * rng.integers(amp // 2, amp + 1, (1, 3, E))
    else:
        shape = rng.integers(-amp, amp + 1, (period, 3, E))
        pat = shape[t % period]
    return _walk(rng, F, E, step) + pat + rng.integers(-(1 << 12), (1 << 12) + 1, (1, 3, E))


def gen_spikes(rng, F, E, amp=1 << 14, step=2, frames=SPIKE_FRAMES):
    """A small walk with single-frame spikes on the fold and region boundaries below F, and on the last frame."""
    x = _walk(rng, F, E, step)
    for f in sorted({f for f in frames if f < F} | {F - 1}):
        x[f] += rng.choice([-1, 1], (3, E)) * rng.integers(amp // 2, amp + 1, (3, E))
    return x


def gen_ramp(rng, F, E, slope_max=3):
    """A linear ramp per series (x = c t + offset, c != 0): MSD(k) = c^2 k^2, ballistic."""
    c = rng.integers(1, slope_max + 1, (1, 3, E)) * rng.choice([-1, 1], (1, 3, E))
    return np.arange(F, dtype=np.int64)[:, None, None] * c + rng.integers(-(1 << 12), (1 << 12) + 1, (1, 3, E))


def gen_alias19(rng, F, E, amp=3072, step=20):
    """The period-19 motion of the sampled-mean test in integers (19 = F / 512 at F = 10 000: the stride of the sampled
    centre), on a slow walk."""
    t = np.arange(F)[:, None, None]
    osc = np.rint(amp * np.sin(2 * np.pi * t / 19.0 + rng.uniform(0, 2 * np.pi, (1, 3, E)))).astype(np.int64)
    return osc + _walk(rng, F, E, step)


GENERATORS = {
    "walk": gen_walk,
    "white": gen_white,
    "alt": lambda rng, F, E: gen_periodic(rng, F, E, 2),
    "p3": lambda rng, F, E: gen_periodic(rng, F, E, 3),
    "p7": lambda rng, F, E: gen_periodic(rng, F, E, 7),
    "spikes": gen_spikes,
    "ramp": gen_ramp,
    "alias19": gen_alias19,
}


def to_float(xi):
    """What the library is given: xi * 2^-10, exact in float64 for |xi| < 2^53."""
    assert np.abs(xi).max(initial=0) < I53
    return xi.astype(np.float64) * UNIT


# --------------------------------------------------------------------------------------------------------- exact sums
def _check_groups(goff, E):
    goff = [int(v) for v in goff]
    assert len(goff) >= 2 and goff[0] >= 0 and goff[-1] <= E and all(a <= b for a, b in zip(goff, goff[1:])), goff
    return goff


def overflow_margin(xi, goff):
    """The largest int64 magnitude exact_sums can meet (as a Python int), for the offsets it subtracts."""
    F = xi.shape[0]
    worst = 0
    for g in range(len(goff) - 1):
        n = goff[g + 1] - goff[g]
        if n == 0:
            continue
        y = xi[:, :, goff[g]:goff[g + 1]]
        m = int(np.abs(y - y[:1]).max())  # |x - x[0]| per series
        # per series: prefix sums and correlations <= F m^2, S1 <= 2 F m^2, S1 - 2 S2 within 4 F m^2; the group: n times that
        worst = max(worst, 4 * F * m * m * n)
    return worst


def exact_sums(xi, max_lag, goff):
    """S [max_lag + 1, G, 3] (int64): sum over the group's entities and the F - k origins of (x[t + k] - x[t])^2."""
    xi = np.asarray(xi)
    assert xi.dtype == np.int64 and xi.ndim == 3 and xi.shape[1] == 3, (xi.dtype, xi.shape)
    F, _, E = xi.shape
    goff = _check_groups(goff, E)
    assert 0 <= max_lag < max(F, 1), (max_lag, F)
    assert overflow_margin(xi, goff) < I63, "int64 sums could overflow: shrink the data or the groups"
    G, K = len(goff) - 1, max_lag + 1
    S = np.zeros((K, G, 3), np.int64)
    k = np.arange(K)
    for g in range(G):
        for e in range(goff[g], goff[g + 1]):
            for a in range(3):
                y = xi[:, a, e] - xi[0, a, e]
                P = np.concatenate(([0], np.cumsum(y * y)))  # P[j] = sum_{t < j} y_t^2
                s1 = (P[F] - P[k]) + P[F - k]
                # c[k] = sum_n y[n + k] y[n]: 'valid' against the series padded with K - 1 zeros: (K) x F products
                s2 = np.correlate(np.concatenate((y, np.zeros(K - 1, np.int64))), y, "valid")
                S[:, g, a] += s1 - 2 * s2
    return S


def sums_fit_double(S):
    """Every partial sum of every summation order is exact in float64: the three axes together stay below 2^53 units."""
    return int(S.sum(axis=2).max(initial=0)) < I53


def _div(S, cnt, u2):
    """round(S * u2 / cnt) for int arrays S, cnt (cnt > 0), u2 a power of two: float64 division where both are exact
    doubles (IEEE division rounds correctly), Python's correctly rounded int / int elsewhere."""
    S = np.asarray(S, np.int64)
    out = np.empty(S.shape)
    small = np.abs(S) < I53
    out[small] = S[small].astype(np.float64) / cnt[small].astype(np.float64)
    for i in zip(*np.nonzero(~small)):
        out[i] = int(S[i]) / int(cnt[i])
    return out * u2


def exact_means(S, F, goff, scale=1.0):
    """The correctly rounded means [K, G, 4] of the exact sums, in the library's units (u = 2^-10 * scale, scale a power of
    two). Returns (by_sum, by_axes): the total column as round((S0 + S1 + S2) / count) — how the difference kernels form
    it — and as (m0 + m1) + m2 of the rounded axis means — how lag_total_kernel and lag_ends_total_kernel do. Lags or
    groups without origins are 0."""
    m, e = math.frexp(scale)
    assert m == 0.5, "scale must be a power of two"
    u2 = (UNIT * scale) ** 2
    K, G, _ = S.shape
    n_g = np.diff(np.asarray(goff, np.int64))
    cnt = (F - np.arange(K, dtype=np.int64))[:, None] * n_g[None, :]
    by_sum = np.zeros((K, G, 4))
    ok = cnt > 0
    for a in range(3):
        by_sum[..., a][ok] = _div(S[..., a][ok], cnt[ok], u2)
    by_sum[..., 3][ok] = _div(S.sum(axis=2)[ok], cnt[ok], u2)
    by_axes = by_sum.copy()
    by_axes[..., 3] = (by_sum[..., 0] + by_sum[..., 1]) + by_sum[..., 2]
    return by_sum, by_axes


def energy(xi, goff, scale=1.0):
    """sum over the group's entities and frames of (x - mean_e)^2 per (group, axis): [G, 3] in the library's units."""
    F, _, E = xi.shape
    goff = _check_groups(goff, E)
    u2 = (UNIT * scale) ** 2
    out = np.zeros((len(goff) - 1, 3))
    for g in range(len(goff) - 1):
        for a in range(3):
            q = Fraction(0)
            for e in range(goff[g], goff[g + 1]):
                y = xi[:, a, e] - xi[0, a, e]
                s, s2 = int(y.sum()), int((y * y).sum())
                q += Fraction(F * s2 - s * s, F)
            out[g, a] = float(q) * u2
    return out


def eps_l(L):
    """The library's relative rounding scale of a spectral path of padded length L'."""
    return 4.0 * EPS * math.log2(L)


def judge(got, S, Q, F, goff, L, scale=1.0):
    """The per-lag criterion of a spectral path of padded length L' against the exact sums S [K, G, 3] and the exact
    energies Q [G, 3] (energy()): for every lag, group and axis

        |mean(k) * count(k) - S(k) u^2|  <=  2 * eps_l * 2 Q  +  4 EPS |S(k) u^2|           (eps_l = 4 EPS log2 L')

    — the library's own per-lag claim eps_l * 2 Q (lag_finish_dd_kernel), with a factor 2 for its sampled centre (the
    series are centred on the mean of ~512 sampled frames, not the exact one), and a few roundings of the mean itself; the
    total column against the sum of its axes' allowances. Returns a dict:
      frac   the largest error / allowance (<= 1: the criterion holds)
      ratio  the largest error / (EPS log2 L' 2 Q) over the axes: the path's measured error in units of its claim's scale
             (numpy's float64 transform measures 0.1-0.2; the allowance is 8)
      rel    the largest |mean - exact| / exact over the lags k >= 1 with S > 0 (what the reported bound must cover)
      loose  the largest eps_l 2 Q / min_k S(k) over the (group, axis) segments: the bound the library should report,
             give or take its centre"""
    K, G, _ = S.shape
    u2 = (UNIT * scale) ** 2
    n_g = np.diff(np.asarray(goff, np.int64)).astype(np.float64)
    cnt = (F - np.arange(K, dtype=np.float64))[:, None] * n_g[None, :]
    Su = S.astype(np.float64) * u2
    tot = np.concatenate([Su, Su.sum(axis=2, keepdims=True)], axis=2)
    err = np.abs(got * cnt[:, :, None] - tot)
    el = eps_l(L)
    allow_q = np.concatenate([2 * el * 2 * Q, (2 * el * 2 * Q).sum(axis=1, keepdims=True)], axis=1)  # [G, 4]
    allow = allow_q[None] + 4 * EPS * np.abs(tot)
    scale_q = EPS * math.log2(L) * 2 * Q  # [G, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(allow > 0, err / allow, np.where(err > 0, np.inf, 0.0))
        ratio = np.where(scale_q[None] > 0, err[..., :3] / scale_q[None], np.where(err[..., :3] > 0, np.inf, 0.0))
        exact = np.concatenate([Su, Su.sum(axis=2, keepdims=True)], axis=2) / np.where(cnt > 0, cnt, 1)[:, :, None]
        nz = (np.arange(K)[:, None, None] >= 1) & (tot > 0)
        rel = np.abs(got - exact)[nz] / exact[nz]
        Smin = np.where(S[1:] > 0, Su[1:], np.inf).min(axis=0) if K > 1 else np.full((G, 3), np.inf)
        loose = np.where(np.isfinite(Smin) & (Q > 0), el * 2 * Q / Smin, 0.0)
    return {"frac": float(frac.max(initial=0.0)), "ratio": float(ratio.max(initial=0.0)),
            "rel": float(rel.max(initial=0.0)), "loose": float(loose.max(initial=0.0))}
