"""
The shapes the full-lag MSD plan tests walk through (tests/test_abi_cpu.py: mdhip_lag_plan against what the parent
commit reports in last_kernel_name(); tests/test_gpu_lag_plan.py: the plan against a real call; tests/test_lag_plan_native_cpu.py: the
item tables under sanitizers).

A case is a dict: frames F, entities E, group offsets `go`, `max_lag`, option overrides `opts`. One case per branch of
lag_choose (csrc/lag_plan.h) and per template instance the launch code names, each at the smallest shape that reaches
it. Unless stated E = 96 (288 columns >= 16 x the 16 clusters of 256 CUs: staging is allowed), one group, full lag.
`plan(case, ...)` asks the library what it would launch; `run(case, B, ctx)` makes the call on a seeded random walk.
"""
import numpy as np

W1, POW2, W12, RESIDUE, BATCHED = range(5)  # info["path"]
FUSED = (POW2, W12)
RESTORE = {"lag_fft_kernel": 3}  # (the value that restores a key's default where -1 does not)


def _case(F, E=96, G=1, go=None, max_lag=None, **opts):
    go = np.linspace(0, E, G + 1).astype(np.int64) if go is None else np.asarray(go, np.int64)
    return dict(F=F, E=E, go=go, max_lag=F - 1 if max_lag is None else max_lag, opts=opts)


K0 = dict(lag_fft_kernel=0, lag_w1=0)  # the first fused kernel (QR instances), whatever the length
K1 = dict(lag_fft_kernel=1, lag_w1=0)  # the second (QR2 instances)
K2 = dict(lag_fft_kernel=2)            # the third at every length it serves (no 12 288-point kernel)

CASES = {
    # one wave per series: padded 1024 / 2048 / 3072, and where it is refused
    "w1_2": _case(2),
    "w1_300": _case(300),
    "w1_1024": _case(1024),
    "w1_1025": _case(1025),
    "w1_1535": _case(1535),
    "w1_ends_1536": _case(1536),  # the 12 288-point kernel's SHORT instance from here on
    "w1_off": _case(300, lag_w1=0),
    "w1_17_groups": _case(300, G=17),
    # the 12 288-point kernel: SHORT | QE 4 | 5 | 6, staged and over the transposed copy
    "w12_short_1600": _case(1600),
    "w12_short_3071": _case(3071),
    "w12_qe4_3072": _case(3072),
    "w12_qe5_4097": _case(4097),
    "w12_qe5_5000": _case(5000),
    "w12_qe5_5120": _case(5120),
    "w12_qe6_5121": _case(5121),
    "w12_qe6_6144": _case(6144),
    "w12_short_src0": _case(1600, lag_direct=0),
    "w12_qe4_src0": _case(3072, lag_direct=0),
    "w12_qe6_src0": _case(6144, lag_direct=0),
    "w12_min_f_0": _case(2100, lag_w12_min_f=0),
    # beyond it: the power-of-two kernel with m = 13, eight staging units
    "pow2_6145": _case(6145),
    "pow2_8192": _case(8192),
    # lag_fft_kernel 0 / 1 / 2 at one shape, and every instance of the three power-of-two kernels
    "k0_2100": _case(2100, **K0),
    "k1_2100": _case(2100, **K1),
    "k2_2100": _case(2100, **K2),
    "k0_qr1": _case(300, **K0),
    "k0_qr2": _case(600, **K0),
    "k0_qr4": _case(1600, **K0),
    "k0_qr10": _case(5000, **K0),
    "k0_qr12": _case(6000, **K0),
    "k0_qr16": _case(8192, **K0),
    "k0_qr24": _case(9000, max_lag=7000, **K0),
    "k0_qr32": _case(12500, max_lag=3000, **K0),
    "k1_qr2_1": _case(300, **K1),
    "k1_qr2_2": _case(1600, **K1),
    "k1_qr2_5": _case(4097, **K1),
    "k1_qr2_8": _case(8192, **K1),
    "k1_qr2_16": _case(9000, max_lag=7000, **K1),  # F > N: only with max_lag < F - 1
    "k2_jj1_qe4": _case(4000, **K2),
    "k2_jj1_qe8": _case(5000, max_lag=3000, **K2),
    "k2_units5_5120": _case(5120, **K2),
    "k2_units8_5121": _case(5121, **K2),
    "k2_jj2_qe8": _case(9000, max_lag=7000, **K2),  # 576 rows per member: beyond the ring, transposed
    "k2_src1": _case(4000, lag_direct=1, **K2),
    "k2_src1_m13": _case(8192, lag_direct=1, **K2),
    "k2_src0": _case(4000, lag_direct=0, **K2),
    # where the series come from
    "direct_0": _case(4097, lag_direct=0),
    "direct_1": _case(4097, lag_direct=1),
    "direct_2": _case(4097, lag_direct=2),
    "direct_3": _case(4097, lag_direct=3),
    "cols_240": _case(4097, E=80),  # fewer than 16 columns per cluster: not staged
    "empty_group": _case(4097, go=[0, 20, 40, 40, 60, 80, 96]),  # 15 non-empty segments of 18: one cluster each, one spare
    "segments_18": _case(4097, go=[0, 14, 28, 28, 42, 56, 70, 96]),  # 18 non-empty segments > 16 clusters: transposed
    # residue classes of a 4 x and an 8 x 6144-point transform
    "d4_8193": _case(8193),
    "d4_12288": _case(12288),
    "d8_12289": _case(12289),
    "d8_24576": _case(24576),
    "residue_0": _case(8193, lag_residue=0),
    "residue_2": _case(8193, lag_residue=2),
    "residue_3_batches": _case(8193, lag_batch_mb=7),
    "overlap_2": _case(8193, lag_overlap=2),
    # the batched transforms
    "batched_24577": _case(24577),
    "batched_fuse_0": _case(8193, lag_residue=0, lag_batched_fuse=0),
    "batched_fuse_1": _case(8193, lag_residue=0, lag_batched_fuse=1),
    "batched_3_batches": _case(8193, lag_residue=0, lag_batch_mb=32),
    "variant_4": _case(300, lag_variant=4),
}


def plan(case, cu_count=256, lds_bytes=163840, ctx=None, aligned=True):
    """mdhip_lag_plan for `case` -> dict(kernel=..., **INFO). `ctx`: a context whose options and device limits are used
    instead of the defaults, cu_count and lds_bytes (pass 0 for the two)."""
    from mdproptools_amd import backend

    return backend.lag_plan(case["F"], case["E"], case["max_lag"], case["go"], opts=case["opts"], ctx=ctx, cu_count=cu_count,
                            lds_bytes=lds_bytes, aligned=aligned)


def series(case, seed=5):
    """A random walk [F, 3, E] (host memory; the library stages it, 16-byte aligned)."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0.0, 0.1, (case["F"], 3, case["E"])), axis=0)


def run(case, B, ctx, seed=5):
    """The real call for `case`, asynchronous with a device result so that the status word can be read. The spectral
    result is accepted whatever its bound (lag_variant 2 unless the case sets the option: with 3 a missed bound lets the
    exact kernel answer and leave ITS name) -> dict(out, kernel, launches, bound, status, fallbacks)."""
    import torch

    opts = {"lag_variant": 2, **case["opts"]}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        n_fb = ctx.fallbacks()
        G = len(case["go"]) - 1
        out = torch.empty((case["max_lag"] + 1, G, 4), dtype=torch.float64, device="cuda")
        status = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        h = B.lag_msd(series(case, seed), case["max_lag"], case["go"], ctx=ctx, out=out, async_=True, status_out=status)
        h.wait()
        ctx.sync()
        return dict(out=out.cpu().numpy(), kernel=ctx.last_kernel_name(), launches=ctx.last_kernel_ms()[1],
                    bound=ctx.last_rel_bound(), status=float(status.cpu()[0]), fallbacks=ctx.fallbacks() - n_fb)
    finally:
        for k in opts:
            ctx.set_option(k, RESTORE.get(k, -1))
