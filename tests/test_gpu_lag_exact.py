"""
Full-lag MSD (mdhip_lag_msd) against EXACT integer sums at every lag, on every path (tests/lag_exact.py).

Trajectories are integers times 2^-10 with power-of-two scales, so each MSD sum has one exact value S(k). The difference
kernels must give the correctly rounded means bit for bit. Every spectral path is held, at every lag, to the library's own
per-lag claim with a factor 2 for its sampled centre:

    |mean(k) count(k) - S(k)| <= 2 eps_l 2 Q + 4 EPS |S(k)|,        eps_l = 4 EPS log2 L'  (L': the path's padded length)

with Q the exact energy of the (axis, group) segment — not the relative bound tied to min_k S(k) the other tests use, which
at middle lags allows hundreds of times more. The reported bound is checked from both sides against the exact sums.

Worst measured ratio max |err| / (EPS log2 L' 2 Q) per path on an MI355X (numpy's float64 transform: 0.03-0.3; the
allowance is 8; `-s` prints the table):
    msd_power_w1_kernel 0.19, msd_power_lds_kernel 0.39, msd_power_w12_kernel 0.24 (C4's 64-entity group included),
    msd_power_w12p_kernel 0.13, msd_power_w12r_kernel 0.11, msd_power_w12p_kernel + msd_power_w12o_kernel 0.12,
    lag_msd_fft 0.18. The file runs in about 40 s.

What it sees that the rest of the suite does not: the sums of msd_power_w12o_kernel<3> (D = 8), or of the odd class of
msd_power_w12p_kernel at D = 4, made 1e-10 too large in the upper half of the frequency band (a trial build, not kept) leave
every other GPU test passing — their random walks carry ~1/F of their energy there — and fail the criterion here by
200-900 x on white noise and spikes.
"""
import contextlib
import time

import numpy as np
import pytest

import lag_exact as X

pytestmark = pytest.mark.gpu

W1 = "msd_power_w1_kernel"
LDS = "msd_power_lds_kernel"
W12 = "msd_power_w12_kernel"
W12P = "msd_power_w12p_kernel"
W12R = "msd_power_w12r_kernel"
W12PO = "msd_power_w12p_kernel + msd_power_w12o_kernel"
BATCHED = "lag_msd_fft"
SCALES = (1.0, 0.5, 2.0**-33)
RATIOS = {}  # path -> (worst ratio, case)
TIMES = {}


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    yield backend
    print("\nworst max|err| / (EPS log2 L' 2 Q) per path:")
    for k, (r, case) in sorted(RATIOS.items()):
        print("  %-48s %.3f  (%s)" % (k, r, case))
    for k, t in TIMES.items():
        print("  time %-43s %.3f s" % (k, t))


@pytest.fixture(scope="module")
def ctx(B):
    return B.default_context()


RESTORE = {"lag_fft_kernel": 3}  # (the value that restores a key's default where -1 does not)


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, RESTORE.get(k, -1))
        ctx.set_option("lag_variant", -1)


class Case:
    """One trajectory and its exact reference, computed once for the longest lag range any of its calls asks for."""

    def __init__(self, gen, F, E, goff, max_lag=None, seed=0, xi=None):
        self.gen, self.F, self.goff = gen, F, list(goff)
        self.xi = xi if xi is not None else X.GENERATORS[gen](np.random.default_rng(seed * 7919 + F), F, E)
        self.max_lag = F - 1 if max_lag is None else max_lag
        self.r = X.to_float(self.xi)
        self.S = X.exact_sums(self.xi, self.max_lag, self.goff)
        self.Q1 = X.energy(self.xi, self.goff)  # (scale 1: Q scales with scale^2)

    def name(self, max_lag):
        return "%s F=%d max_lag=%d G=%d" % (self.gen, self.F, max_lag, len(self.goff) - 1)

    def means(self, max_lag, scale):
        return X.exact_means(self.S[: max_lag + 1], self.F, self.goff, scale)


def spectral(B, ctx, c, max_lag, scale, L, kernel, **opts):
    """One call on a spectral path (lag_variant 2 + opts): the kernel that answered, the per-lag criterion, the reported
    bound from both sides. Returns the means."""
    with options(ctx, **{"lag_variant": 2, **opts}):
        got = B.lag_msd(c.r, max_lag, c.goff, scale=scale)
        name, bound = ctx.last_kernel_name(), ctx.last_rel_bound()
    assert name == kernel, (c.name(max_lag), opts, name, kernel)
    S = c.S[: max_lag + 1]
    j = X.judge(got, S, c.Q1 * scale**2, c.F, c.goff, L, scale)
    where = "%s scale=%g %s" % (c.name(max_lag), scale, opts or "")
    if j["ratio"] > RATIOS.get(kernel, (-1.0,))[0]:
        RATIOS[kernel] = (j["ratio"], where)
    assert j["frac"] <= 1.0, (where, j)
    assert (got[0] == 0.0).all()
    # the reported bound covers the error against the exact sums at every lag (+ the rounding of a mean) ...
    assert j["rel"] <= bound + 2 * X.EPS, (where, j, bound)
    # ... and is not looser than the claim at the smallest exact sum, give or take the sampled centre
    assert bound <= 2 * j["loose"] * (1 + 1e-9), (where, j, bound)
    return got


def assert_exact(got, want, where):
    bad = np.argwhere(got != want)
    assert not len(bad), (where, len(bad), bad[:5].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:3]])


# ------------------------------------------------------------------------------------------- difference kernels
DIFF_CASES = [(2, 1, "walk"), (3, 2, "white"), (17, 16, "spikes"), (513, 512, "ramp"), (2100, 2099, "alt"),
              (4097, 4096, "white"), (8193, 8192, "spikes"), (12289, 12288, "p7"), (24577, 1500, "walk")]


@pytest.mark.parametrize("F,max_lag,gen", DIFF_CASES)
def test_difference_kernels_bit_exact(B, ctx, F, max_lag, gen):
    """lag_variant 1 (the series-resident lag_msd_lds_kernel while a series fits the LDS, here F <= 12 289) and 0 (the staged
    lag_msd_kernel, and lag_variant 1 beyond the LDS): every component equals the correctly rounded mean of the exact sum
    — the total column as round((S0 + S1 + S2) / count). These kernels are every other lag test's reference."""
    E = 5 if F < 20000 else 3
    goff = [0, 1, 1, E] if E == 5 else [0, 1, 3]
    c = Case(gen, F, E, goff, max_lag, seed=1)
    assert X.sums_fit_double(c.S), "the data must keep every sum exact in float64"
    for scale in SCALES:
        want, _ = c.means(max_lag, scale)
        for variant, kernel in ((1, "lag_msd_lds_kernel" if F <= 12289 else "lag_msd_kernel"), (0, "lag_msd_kernel")):
            with options(ctx, lag_variant=variant):
                got = B.lag_msd(c.r, max_lag, goff, scale=scale)
                assert ctx.last_kernel_name() == kernel and ctx.last_rel_bound() == 0.0, (F, variant, ctx.last_kernel_name())
            assert_exact(got, want, (F, variant, scale))


# ---------------------------------------------------------------------------------------------- one wave per series
# (F, max_lag, the kernel, padded length): both sides of F + max_lag = 1024, 2048 and of F = 1536
W1_SHAPES = [(2, 1, W1, 1024), (3, 2, W1, 1024), (512, 511, W1, 1024), (513, 511, W1, 1024), (513, 512, W1, 2048),
             (1024, 0, W1, 1024), (1024, 1, W1, 2048), (1025, 1023, W1, 2048), (1025, 1024, W1, 3072),
             (1535, 1534, W1, 3072), (1536, 512, W1, 2048), (1536, 513, W12, 12288), (1536, 1535, W12, 12288)]


def test_short_series_one_wave_per_series(B, ctx):
    """msd_power_w1_kernel (F <= 1536, F + max_lag <= 3072, at most 16 groups; padded length 1024, 2048, 3072) on both sides
    of every edge of its range, on white noise, spikes and walks; 17 groups take the block-wide kernel."""
    gens = ["white", "spikes", "walk", "p3", "alt", "ramp", "alias19", "p7"]
    for i, (F, max_lag, kernel, L) in enumerate(W1_SHAPES):
        E = 24
        c = Case(gens[i % len(gens)], F, E, [0, 1, 1, 9, E], max_lag, seed=2)
        spectral(B, ctx, c, max_lag, SCALES[i % 3], L, kernel)
    c = Case("white", 1000, 40, list(range(0, 33, 2)) + [40], seed=3)  # 17 groups
    spectral(B, ctx, c, 999, 1.0, 2048, LDS)
    spectral(B, ctx, Case("spikes", 1030, 16, list(range(17)), seed=3), 1029, 0.5, 3072, W1)  # 16 one-entity groups


# ------------------------------------------------------------------------------------------- fused LDS kernels
def test_fused_kernels_every_padded_length(B, ctx):
    """The block-wide kernels (lag_fft_kernel 0, 1, 2) at padded lengths 2^9 ... 2^14, with the one-wave and 12 288-point
    kernels switched off; odd entity counts, an empty and a one-entity group. (The three forms report the same kernel name:
    what is checked is that each option's result meets the criterion, not which form ran.)"""
    gens = ["white", "spikes", "walk", "alt", "p7", "alias19"]
    for i, (F, max_lag) in enumerate(((300, 211), (600, 424), (1500, 548), (2100, 1996), (5000, 3192), (9000, 7384))):
        L = 1 << int(np.ceil(np.log2(F + max_lag)))
        c = Case(gens[i], F, 21, [0, 1, 1, 21], max_lag, seed=4)
        for kern in (0, 1, 2):
            spectral(B, ctx, c, max_lag, SCALES[(i + kern) % 3], L, LDS, lag_w1=0, lag_w12_min_f=0, lag_fft_kernel=kern)


@pytest.mark.parametrize("F,gen", [(4097, "white"), (5120, "spikes"), (5121, "walk"), (8192, "white")])
def test_fused_kernels_sources_and_forms(B, ctx, F, gen):
    """lag_fft_kernel 0-3 x lag_direct 0/1/2 (a transposed copy, the trajectory read in place, tiles transposed inside the
    kernel; the name tells the 12 288-point kernel from the power-of-two ones, not the forms or sources apart) at the edges of the staging units (5120 / 5121) and of the 12 288-point kernel (F + max_lag <= 12 288), with 89
    entities (267 columns: off the 16-column tiles, enough for the clusters of 16) in ragged groups."""
    c = Case(gen, F, 89, [0, 5, 5, 48, 89], seed=5)
    for kern in (3, 2, 1, 0):
        w12 = kern == 3 and 2 * F - 1 <= 12288
        L = 12288 if w12 else 1 << int(np.ceil(np.log2(2 * F - 1)))
        for src in (0, 1, 2):
            spectral(B, ctx, c, F - 1, SCALES[(kern + src) % 3], L, W12 if w12 else LDS, lag_fft_kernel=kern, lag_direct=src)


# ------------------------------------------------------------------------------------------- residue classes
def test_residue_classes_d4(B, ctx):
    """16 384 < F + max_lag <= 24 576, F <= 12 288: msd_power_w12p_kernel (lag_residue 1) and msd_power_w12r_kernel (2),
    padded length 24 576; F + max_lag = 16 384 is still the fused kernel's. F = 12 289 is the D = 8 side."""
    for gen, F, lags in (("white", 8193, (8191, 8192)), ("spikes", 12288, (4096, 4097, 12287)), ("walk", 12288, (12287,))):
        c = Case(gen, F, 4, [0, 1, 4], seed=6)
        for i, max_lag in enumerate(lags):
            if F + max_lag <= 16384:
                spectral(B, ctx, c, max_lag, SCALES[i % 3], 16384, LDS)
                continue
            for residue, kernel in ((1, W12P), (2, W12R)):
                spectral(B, ctx, c, max_lag, SCALES[(i + residue) % 3], 24576, kernel, lag_residue=residue)
    c = Case("p3", 12289, 3, [0, 3], seed=6)
    spectral(B, ctx, c, 4095, 1.0, 16384, LDS)
    spectral(B, ctx, c, 4096, 0.5, 49152, W12PO)


def test_residue_classes_d8(B, ctx):
    """12 288 < F <= 24 576, F + max_lag <= 49 152: the fold-transposition, the even frequencies by the D = 4 kernel and the
    odd ones by msd_power_w12o_kernel<1|3>, padded length 49 152; F = 24 577 goes to the batched transforms."""
    for gen, F, E, max_lag in (("white", 12289, 3, 12288), ("spikes", 16000, 3, 15999), ("alt", 16000, 2, 9000),
                               ("spikes", 24576, 2, 24575), ("white", 24576, 1, 24575)):
        c = Case(gen, F, E, [0, 1, E] if E > 1 else [0, 1], max_lag, seed=7)
        spectral(B, ctx, c, max_lag, SCALES[F % 3], 49152, W12PO)
    c = Case("white", 24577, 1, [0, 1], 1000, seed=7)
    spectral(B, ctx, c, 1000, 1.0, 32768, BATCHED)


# ------------------------------------------------------------------------------------------- batched transforms
def test_batched_transforms(B, ctx):
    """Beyond the residue classes: padded length 2^m through the batched global transforms, F + max_lag = 49 153,
    65 536 and 65 537, lag_batched_fuse 0 (padded copy, half spectra), 1 (in-place first pass, |X|^2 from the packed
    transform), 2 (two passes, the second fused with |X|^2); a 70 000-frame call (2^17 points, which the transform plans as a
    radix-2^9 pass + a radix-2^8 pass — the plan is not visible from here: the name is lag_msd_fft for every form)."""
    for gen, F, lags in (("white", 24577, (24576,)), ("spikes", 40000, (25536, 25537))):
        c = Case(gen, F, 1, [0, 1], max(lags), seed=8)
        for max_lag in lags:
            L = 1 << int(np.ceil(np.log2(F + max_lag)))
            for fuse in (0, 1, 2):
                spectral(B, ctx, c, max_lag, SCALES[fuse], L, BATCHED, lag_batched_fuse=fuse)
    c = Case("walk", 70000, 2, [0, 1, 2], 3000, seed=8)
    spectral(B, ctx, c, 3000, 0.5, 131072, BATCHED, lag_variant=4)


# (radix, tile width) instance of fft_power_pass_kernel -> the smallest call that selects it: the second pass of the fused
# form (lag_batched_fuse=2) has radix 2^(logH - ceil(logH / 2)), H = L / 2. The calls above and in the other tests reach
# (5,4), (7,4) and (8,3) through L = 4096, 2^15 .. 2^18; these are the other four the library is built with.
FUSED_PASS_INSTANCES = [((6, 4), "white", 3000, 2000, 8192, {"lag_variant": 4}), ((9, 2), "spikes", (1 << 18) + 1, 8, 1 << 19, {}),
                        ((10, 1), "white", (1 << 20) + 1, 8, 1 << 21, {}), ((11, 1), "spikes", (1 << 22) + 1, 8, 1 << 23, {})]


@pytest.mark.parametrize("inst,gen,F,max_lag,L,opts", FUSED_PASS_INSTANCES, ids=["%d-%d" % c[0] for c in FUSED_PASS_INSTANCES])
def test_batched_transforms_fused_pass_instances(B, ctx, inst, gen, F, max_lag, L, opts):
    """One series per call, nine lags at the long lengths: exact sums at every lag for each instance of the fused second
    pass. The shape must still plan to the padded length that selects the instance (a change of the plan's rule fails here
    rather than emptying the case)."""
    opts = {"lag_batched_fuse": 2, **opts}
    plan = B.lag_plan(F, 1, max_lag, [0, 1], opts={"lag_variant": 2, **opts}, ctx=ctx)
    logH = L.bit_length() - 2
    assert (plan["kernel"], plan["L"]) == (BATCHED, L) and logH - (logH + 1) // 2 == inst[0], (plan, inst)
    c = Case(gen, F, 1, [0, 1], max_lag, seed=12)
    assert X.sums_fit_double(c.S), "the data must keep every sum exact in float64"
    spectral(B, ctx, c, max_lag, 1.0, L, BATCHED, **opts)


# ------------------------------------------------------------------------------------------- groups, batches, centring
def test_many_groups_every_path(B, ctx):
    """17 and 40 groups (ragged, empty, one-entity) on every path that takes more than 16: the 12 288-point kernel, the
    power-of-two LDS kernel, the residue classes D = 4 (lag_residue 1 and 2) and D = 8 (no cap on the group count), the batched
    transforms (lag_variant 4). The D = 4 call's own time (a repeated call, out of the judging) measured 5 ms with 17 groups
    and 13 ms with 40 at F = 9000, E = 40 (-s prints it)."""
    g17 = [0, 1, 1, 2, 5, 5, 9, 10, 14, 15, 20, 21, 27, 28, 30, 31, 39, 40]
    g40 = list(range(41))
    for goff in (g17, g40):
        c = Case("white", 2000, 40, goff, seed=9)
        spectral(B, ctx, c, 1999, 0.5, 12288, W12)
        spectral(B, ctx, c, 1999, 1.0, 4096, LDS, lag_w12_min_f=0)
        spectral(B, ctx, c, 1999, 1.0, 4096, BATCHED, lag_variant=4)
        c = Case("spikes", 9000, 40, goff, 7400, seed=9)
        spectral(B, ctx, c, 7400, 1.0, 24576, W12P)
        spectral(B, ctx, c, 7400, 0.5, 24576, W12R, lag_residue=2)
        with options(ctx, lag_variant=2):
            B.lag_msd(c.r, 7400, goff)
            t0 = time.perf_counter()
            B.lag_msd(c.r, 7400, goff)
            TIMES["residue D=4, %d groups, F=9000, E=40" % (len(goff) - 1)] = time.perf_counter() - t0
            assert ctx.last_kernel_name() == W12P
        c = Case("white", 13000, 40, goff, 4000, seed=9)
        spectral(B, ctx, c, 4000, 0.5, 49152, W12PO)


def test_batches_overlap_and_centre(B, ctx):
    """1 MB batches (groups straddle them), the CU-partitioned transposition (lag_overlap 2), and the centre on 512 / every /
    64 sampled frames (lag_mean_sample -1 / 0 / 64), on the residue-class and batched paths; the period-19 motion whose
    period is the sampling stride at F = 10 000."""
    c = Case("white", 12288, 8, [0, 3, 8], 12287, seed=10)
    for residue, kernel in ((1, W12P), (2, W12R)):
        for overlap in (2, 0):
            spectral(B, ctx, c, 12287, 0.5, 24576, kernel, lag_residue=residue, lag_batch_mb=1, lag_overlap=overlap)
    spectral(B, ctx, c, 12287, 1.0, 32768, BATCHED, lag_residue=0, lag_batch_mb=1)
    c = Case("spikes", 13000, 6, [0, 1, 4, 6], seed=10)
    spectral(B, ctx, c, 12999, 0.5, 49152, W12PO, lag_batch_mb=1, lag_overlap=2)
    c = Case("alias19", 10000, 6, [0, 6], seed=10)
    for sample in (-1, 0, 64):
        spectral(B, ctx, c, 9999, 1.0, 24576, W12P, lag_mean_sample=sample)
        spectral(B, ctx, c, 9999, 0.5, 32768, BATCHED, lag_residue=0, lag_mean_sample=sample)


# ------------------------------------------------------------------------------------------- device and async results
def test_device_and_async_results_equal_host(B, ctx):
    """One shape per path: the means into a device tensor (out=) and the asynchronous call with its device status word equal
    the host result bit for bit; the status word is the reported bound."""
    import torch

    for gen, F, E, max_lag, opts in (("white", 1000, 8, 999, {}), ("spikes", 1500, 8, 1499, {"lag_w1": 0}),
                                     ("walk", 5000, 20, 4999, {}), ("white", 8192, 20, 8191, {}),
                                     ("spikes", 12288, 3, 12287, {}), ("white", 12288, 3, 12287, {"lag_residue": 2}),
                                     ("alt", 16000, 3, 15999, {}), ("white", 24577, 1, 24576, {})):
        c = Case(gen, F, E, [0, 1, E], max_lag, seed=11)
        goff = c.goff
        with options(ctx, **{"lag_variant": 2, **opts}):
            host = B.lag_msd(c.r, max_lag, goff, scale=0.5)
            bound = ctx.last_rel_bound()
            dev_r = torch.from_numpy(c.r).cuda()
            out = torch.empty((max_lag + 1, len(goff) - 1, 4), dtype=torch.float64, device="cuda")
            B.lag_msd(dev_r, max_lag, goff, scale=0.5, out=out)
            torch.cuda.synchronize()
            assert_exact(out.cpu().numpy(), host, (F, opts, "out="))
            out2 = torch.full_like(out, -1.0)
            st = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
            B.lag_msd(dev_r, max_lag, goff, scale=0.5, out=out2, async_=True, status_out=st).wait()
            torch.cuda.synchronize()
            assert_exact(out2.cpu().numpy(), host, (F, opts, "async"))
            assert float(st.item()) == bound, (F, opts, float(st.item()), bound)


# ------------------------------------------------------------------------------------------- lag_variant 3 and lag_ends
def test_variant3_repairs_against_exact_sums(B, ctx):
    """lag_variant 3 with the bound missed at a few lags per end: the repaired rows (every lag whose exact sum lies well
    below the threshold the finish kernel applies) equal the correctly rounded means — total as (m0 + m1) + m2 — bit for bit;
    every row equals them or meets the reported bound (<= 1e-10) against the exact sums; lag_ends 0 gives the difference
    kernel's result, i.e. the exact means, bit for bit."""
    F, E, goff = 5000, 24, [0, 10, 24]
    t = np.arange(F)[:, None, None]
    for i, amp in enumerate((440, 830)):
        rng = np.random.default_rng(12 + i)
        xi = X._walk(rng, F, E, 8) + np.rint(amp * np.sin(2 * np.pi * t / F + rng.uniform(0, 6.28, (1, 3, E)))).astype(np.int64)
        c = Case("walk+slow", F, E, goff, xi=xi)
        by_sum, by_axes = c.means(F - 1, 1.0)
        with options(ctx, lag_variant=2):
            B.lag_msd(c.r, F - 1, goff)
            assert ctx.last_rel_bound() > 1e-10, (amp, ctx.last_rel_bound())  # (else the case tests nothing)
        with options(ctx, lag_variant=3):
            got = B.lag_msd(c.r, F - 1, goff)
            bound = ctx.last_rel_bound()
            assert "lag_low_lags_kernel" in ctx.last_kernel_name() and 0.0 < bound <= 1e-10, (ctx.last_kernel_name(), bound)
        # lags whose |S1 - 2 S2| is surely below eps_l 2 tot / 1e-10 (tot >= Q: the sampled centre only adds energy)
        thr = X.eps_l(12288) * 2 * c.Q1 / 1e-10  # [G, 3]
        low = (c.S.astype(np.float64) * X.UNIT**2 < 0.5 * thr[None]).any(axis=(1, 2))
        low[0] = False
        ks = np.nonzero(low)[0]
        must = [k for k in range(1, F) if (ks[ks < F // 2].size and k <= ks[ks < F // 2].max())
                or (ks[ks >= F // 2].size and k >= ks[ks >= F // 2].min())]
        assert must and len(must) <= 48, (amp, must)
        assert_exact(got[must], by_axes[must], (amp, "repaired rows"))
        same = (got == by_axes).all(axis=(1, 2))
        nz = by_sum > 0
        rel = np.where(nz, np.abs(got - by_sum) / np.where(nz, by_sum, 1.0), 0.0)
        assert (rel[~same] <= bound).all(), (amp, rel[~same].max(), bound)
        with options(ctx, lag_variant=3, lag_ends=0):
            whole = B.lag_msd(c.r, F - 1, goff)
            assert ctx.last_kernel_name().startswith("lag_msd_") and ctx.last_rel_bound() == 0.0
        assert_exact(whole, by_sum, (amp, "lag_ends 0"))


# ------------------------------------------------------------------------------------------- the benchmark's shape
def test_bench_shape_default_path(B, ctx):
    """C4 (50 000 entities x 5000 frames, an integer walk made on the device) through the default path: the 12 288-point
    kernel answers with a bound <= 1e-10, and a 64-entity group of the same call meets the per-lag criterion against exact
    sums and stays within the reported bound (from below only: the bound covers all 50 000 entities, not the group)."""
    import torch

    F, E = 5000, 50000
    g = torch.Generator(device="cuda").manual_seed(4)
    steps = torch.randint(-8, 9, (F, 3, E), dtype=torch.int32, device="cuda", generator=g)
    xi_d = torch.cumsum(steps, dim=0, dtype=torch.int32)
    del steps
    xi_d += torch.randint(-(1 << 18), 1 << 18, (1, 3, E), dtype=torch.int32, device="cuda", generator=g)
    r = xi_d.to(torch.float64) * X.UNIT
    head = xi_d[:, :, :64].to(torch.int64).cpu().numpy()
    del xi_d
    goff = [0, 64, E]
    with options(ctx, lag_variant=-1):
        got = B.lag_msd(r, F - 1, goff, scale=0.5)
        name, bound = ctx.last_kernel_name(), ctx.last_rel_bound()
    del r
    torch.cuda.empty_cache()
    assert name == W12 and 0.0 < bound <= 1e-10, (name, bound)
    S = X.exact_sums(head, F - 1, [0, 64])
    Q = X.energy(head, [0, 64]) * 0.25
    j = X.judge(got[:, :1], S, Q, F, [0, 64], 12288, 0.5)
    if j["ratio"] > RATIOS.get(W12, (-1.0,))[0]:
        RATIOS[W12] = (j["ratio"], "C4 group of 64")
    assert j["frac"] <= 1.0, j
    assert j["rel"] <= bound + 2 * X.EPS, (j, bound)
