"""
The call deck: one entry per public kernel entry of backend.py and size, plus entries chosen for the state a context
keeps between calls (tests/test_gpu_call_order.py runs them in many orders on one context; tests/test_call_deck_cpu.py
shows on the CPU that every entry tests something). Importable without a GPU and without torch.

An entry has
  make()                                   -> dict of numpy inputs, seeded: the same bytes every time
  call(B, ctx, inputs, device=False)       -> tuple of results of exactly ONE backend function, called with ctx=ctx
  reference(inputs)                        -> what the family's own plain restatement gives (imported, not rewritten)
  check(got, want)                         -> the criterion of the family's own test file: equality for integers and for
                                              exact-integer data, that file's derived bound otherwise
`staged` names the float64 inputs the library stages (host) or reads in place (device). `call` also takes `stage=`, an
object with put(array), out(shape, dtype), pre() and async_ (class Stage): how the stream tests hand over late inputs,
device result buffers and the asynchronous forms without a second copy of every call.

Sizes. small = the smallest shape the family's own file uses either side of a tile (17 centres, 65 entities, 257
atoms, ...); large = every staged input and every result array at least four times the bytes (frames, atoms, bins,
classes or jobs times four, the box grown to keep the density), nothing above 4 100 atoms x 12 frames or 70 000 samples
but the one cumtrapz entry of 1 000 001 samples.
"""
import numpy as np

import aggregates_ref
import angular_ref
import cluster_ref
import config_ref
import displacement_ref
import einstein_ref
import hbonds_ref
import hydration_ref
import lag_exact
import number_density_ref
import reorientation_ref
import residence_design
import sdf_ref
import segment_exact
import vanhove_ref
from nonfinite_cases import k1024
from oracle import cpu_ref, cref

K = {"small": 1, "large": 4}
XCORR_FFT, XCORR_DIRECT = 0, 1  # backend.XCORR_*


# ----------------------------------------------------------------------------------------------------- staging
class Stage:
    """How a call receives its arrays: as they are (host), or as CUDA tensors on the context's device. Results stay
    on the host (out() gives None) and calls are synchronous; the stream tests subclass this."""

    async_ = False

    def __init__(self, ctx=None, device=False):
        self.ctx, self.device = ctx, device

    def put(self, a):
        if not self.device:
            return a
        import torch

        return torch.as_tensor(np.ascontiguousarray(a), device="cuda:%d" % self.ctx.device)

    def out(self, shape, dtype="float64"):
        return None

    def pre(self):
        """Called immediately before the backend function."""


class Deferred:
    """An asynchronous call in flight: finish() completes it and gives the entry's result tuple. `outs`: the device
    result buffers of the call (the stream tests copy them back on their own stream)."""

    def __init__(self, pending, pack, outs=(), status=None):
        self.pending, self.pack, self.outs = pending, pack, tuple(o for o in outs if o is not None)
        self.status = status  # lag_msd: the device word that says whether the result on the stream is final

    def finish(self):
        return self.pack(self.pending.wait())


def _done(res, pack, outs=(), status=None):
    return Deferred(res, pack, outs, status) if hasattr(res, "wait") and hasattr(res, "ticket") else pack(res)


def host(v):
    """A result as numpy / int: device tensors come back, int64 bit patterns of counts are uint64 again."""
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
        return v.view(np.uint64) if v.dtype == np.int64 else v
    return v


def as_bytes(result):
    """The bytes of a result tuple (what call-order independence compares)."""
    out = []
    for v in result:
        v = host(v)
        out.append(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else v)
    return out


# ----------------------------------------------------------------------------------------------------- criteria
def same(got, want):
    """Equality of every member: integers and exact-integer data (NaN equals NaN, as the families' files hold it)."""
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = host(g), host(w)
        if isinstance(w, np.ndarray) or isinstance(g, np.ndarray):
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape, (k, g.shape, w.shape)
            if g.dtype.kind == "f" or w.dtype.kind == "f":
                assert np.array_equal(g.astype(np.float64), w.astype(np.float64), equal_nan=True), k
            else:
                assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), k
        else:
            assert g == w, (k, g, w)


def same_signed(got, want):
    """Equality that tells -0 from +0 (tests/reorientation_ref.py: same_bits)."""
    same(got, want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray) and w.dtype.kind == "f":
            assert reorientation_ref.same_bits(host(g), w), k


def same_bytes(got, want):
    """Every member bit for bit (the families that hold floating-point results to their bytes)."""
    same(got, want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray) and w.dtype.kind == "f":
            assert np.ascontiguousarray(host(g)).tobytes() == np.ascontiguousarray(w).tobytes(), k


class Entry:
    def __init__(self, name, fn, size, make, run, reference, check, staged, nontrivial, device=True, has_out=False,
                 tags=(), arrays=None, out_form=None):
        self.name, self.fn, self.size = name, fn, size
        # what the result is when the stage hands out device result buffers, from the host form's (default: the same)
        self.out_form = out_form or (lambda result: result)
        # the members of reference() that have a result's shape (default: every array of it)
        self.arrays = arrays or (lambda want: [w for w in want if isinstance(w, np.ndarray)])
        self.make, self._run, self.reference, self.check = make, run, reference, check
        self.staged, self.nontrivial, self.device, self.has_out, self.tags = staged, nontrivial, device, has_out, tags

    def call(self, B, ctx, inputs, device=False, stage=None):
        return self._run(B, ctx, inputs, stage or Stage(ctx, device))

    def __repr__(self):
        return "Entry(%s)" % self.name


DECK = {}


def _add(name, fn, size, make, run, reference, check, staged, nontrivial, **kw):
    assert name not in DECK, name
    DECK[name] = Entry(name, fn, size, make, run, reference, check, staged, nontrivial, **kw)


def _both(fn, build, **kw):
    """The small and the large variant of one family: build(k) -> (make, run, reference, check, staged, nontrivial)."""
    for size, k in K.items():
        _add("%s_%s" % (fn, size), fn, size, *build(k), **kw)


def _grown(L, k):
    """Box edges for k times the atoms at the same density, on a grid of 1/8."""
    return np.round(np.asarray(L, dtype=np.float64) * k ** (1.0 / 3.0) * 8.0) / 8.0


def _gas(seed, F, n, L):
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    return np.round(rng.uniform(0, 1, (F, 3, n)) * L[None, :, None], 3), np.tile(L, (F, 1))


def _hist_hits(k=0):
    return lambda want: np.asarray(want[k]).sum() > 0


# ================================================================================================ pair histograms
def _pair_make(n, F, L, seed, r_cut=12.0, ddr=0.2, nb=60):
    def make():
        from mdproptools_amd import synth

        rel = np.array(synth.ALL_PAIRS_4, dtype=np.int32)
        return dict(x=synth.rdf_frames(n, range(F), L, seed), ty=synth.rdf_types(n), box=np.full((F, 3), float(L)),
                    rel=rel, r_cut=r_cut, ddr=ddr, nb=nb, cuts=synth.cn_cutoffs(len(rel)),
                    sites=synth.rdf_frames(max(n // 4, 1), range(F), L, seed + 20),
                    sty=synth.rdf_types(max(n // 4, 1), 2))
    return make


def _ref_rdf(i):
    F = len(i["x"])
    res = [cref.rdf_pairs(i["x"][f], i["ty"], i["rel"], i["box"][f], i["r_cut"] ** 2, i["ddr"], i["nb"])
           for f in range(F)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), int(sum(r[2] for r in res))


def _ref_cn(i):
    return (np.stack([cref.cn_pairs(i["x"][f], i["ty"], i["rel"], i["box"][f], [c * c for c in i["cuts"]])
                      for f in range(len(i["x"]))]),)


def _pair_family(k, seed=30):
    return _pair_make(257 * k, 3 * k, float(_grown(30.0, k)), seed)


def _rdf(k):
    def run(B, ctx, i, X):
        x = X.put(i["x"])
        X.pre()
        return _done(B.rdf_loop(x, i["ty"], i["box"], i["rel"], i["r_cut"], i["ddr"], i["nb"], ctx=ctx,
                                async_=X.async_), tuple)
    return _pair_family(k), run, _ref_rdf, same, ("x",), _hist_hits(0)


def _rdf_cn(k):
    def run(B, ctx, i, X):
        x = X.put(i["x"])
        X.pre()
        return _done(B.rdf_cn_loop(x, i["ty"], i["box"], i["rel"], i["r_cut"], i["ddr"], i["nb"], i["cuts"], ctx=ctx,
                                   async_=X.async_), tuple)
    return _pair_family(k, 31), run, lambda i: _ref_rdf(i) + _ref_cn(i), same, ("x",), _hist_hits(3)


def _cn(k):
    def run(B, ctx, i, X):
        x = X.put(i["x"])
        o = X.out((len(i["rel"]),), "int64")
        X.pre()
        if o is not None:  # (a device buffer holds the frame sums)
            return _done(B.cn_loop(x, i["ty"], i["box"], i["rel"], i["cuts"], per_frame=False, ctx=ctx, out=o,
                                   async_=X.async_), lambda r: (host(r),), (o,))
        return _done(B.cn_loop(x, i["ty"], i["box"], i["rel"], i["cuts"], ctx=ctx, async_=X.async_), lambda r: (r,))
    return _pair_family(k, 32), run, _ref_cn, same, ("x",), _hist_hits(0)


def _rdf_mol(k):
    def run(B, ctx, i, X):
        x, s = X.put(i["x"]), X.put(i["sites"])
        X.pre()
        return tuple(B.rdf_mol_loop(x, i["ty"], s, i["sty"], i["box"], i["rel"][:3], i["r_cut"], i["ddr"], i["nb"],
                                    ctx=ctx))

    def ref(i):
        res = [cref.rdf_rect(i["x"][f], i["ty"], i["sites"][f], i["sty"], i["rel"][:3], i["box"][f], i["r_cut"] ** 2,
                             i["ddr"], i["nb"]) for f in range(len(i["x"]))]
        return np.stack([r[0] for r in res]), int(sum(r[1] for r in res))
    return _pair_family(k, 33), run, ref, same, ("x", "sites"), _hist_hits(0)


def _cn_mol(k):
    def run(B, ctx, i, X):
        x, s = X.put(i["x"]), X.put(i["sites"])
        X.pre()
        return (B.cn_mol_loop(x, i["ty"], s, i["sty"], i["box"], i["rel"][:3], i["cuts"][:3], ctx=ctx),)

    def ref(i):
        return (np.stack([cref.cn_rect(i["x"][f], i["ty"], i["sites"][f], i["sty"], i["rel"][:3], i["box"][f],
                                       [c * c for c in i["cuts"][:3]]) for f in range(len(i["x"]))]),)
    return _pair_family(k, 34), run, ref, same, ("x", "sites"), _hist_hits(0)


_both("rdf_loop", _rdf)
_both("rdf_cn_loop", _rdf_cn)
_both("cn_loop", _cn, has_out=True, out_form=lambda r: (r[0].sum(axis=0),))
_both("rdf_mol_loop", _rdf_mol)
_both("cn_mol_loop", _cn_mol)


def _unpack_words(i):
    R, nb = len(i["rel"]), i["nb"]

    def unpack(t):
        w = host(t).reshape(-1)
        return w[:nb].copy(), w[nb:(1 + R) * nb].reshape(R, nb).copy(), int(w[-1])
    return unpack


def _rdf_dev_run(B, ctx, i, X):
    import torch

    x = X.put(i["x"])
    words = (1 + len(i["rel"])) * i["nb"] + 1
    o = X.out((words,), "int64")
    if o is None:
        o = torch.zeros(words, dtype=torch.int64, device="cuda:%d" % ctx.device)
        torch.cuda.current_stream(o.device).synchronize()
    X.pre()
    return _done(B.rdf_loop_dev(x, i["ty"], i["box"], i["rel"], i["r_cut"], i["ddr"], i["nb"], o, ctx=ctx,
                                async_=X.async_), _unpack_words(i), (o,))


def _ref_rdf_sum(i):
    full, part, ov = _ref_rdf(i)
    return full.sum(axis=0), part.sum(axis=0), ov


_add("rdf_loop_dev", "rdf_loop_dev", "small", _pair_make(257, 3, 30.0, 35), _rdf_dev_run, _ref_rdf_sum, same, ("x",),
     _hist_hits(0), has_out=True)


def _culled_run(B, ctx, i, X):
    """2048 atoms in L = 40 with r_cut 9: eight full tiles, the culled sweep forced (rdf_cull = 1, restored after)."""
    x = X.put(i["x"])
    ctx.set_option("rdf_cull", 1)
    try:
        X.pre()
        return tuple(B.rdf_loop(x, i["ty"], i["box"], i["rel"], i["r_cut"], i["ddr"], i["nb"], ctx=ctx))
    finally:
        ctx.set_option("rdf_cull", -1)


_add("rdf_loop_culled", "rdf_loop", "state", _pair_make(2048, 2, 40.0, 36, r_cut=9.0, ddr=0.1, nb=90), _culled_run,
     _ref_rdf, same, ("x",), _hist_hits(0), tags=("pair",))


class InFlight(Stage):
    """The asynchronous form on the stage it wraps: the call is left in flight."""

    async_ = True

    def __init__(self, inner):
        self.inner = inner

    def put(self, a):
        return self.inner.put(a)

    def out(self, shape, dtype="float64"):
        return self.inner.out(shape, dtype)

    def pre(self):
        self.inner.pre()


def _in_flight(run):
    return lambda B, ctx, i, X: run(B, ctx, i, InFlight(X))


_add("rdf_loop_async", "rdf_loop", "state", _pair_make(300, 9, 30.0, 37), _in_flight(_rdf(1)[1]), _ref_rdf, same,
     ("x",), _hist_hits(0), tags=("pair", "in_flight"))
_add("rdf_cn_loop_async", "rdf_cn_loop", "state", _pair_make(2100, 4, 40.0, 38, r_cut=9.0, ddr=0.1, nb=90),
     _in_flight(_rdf_cn(1)[1]), lambda i: _ref_rdf(i) + _ref_cn(i), same, ("x",), _hist_hits(3),
     tags=("pair", "in_flight"))


# ================================================================================================ segments
def _seg_make(k):
    def make():
        sizes = np.tile(segment_exact.segment_tables()["ragged"], k)
        off = segment_exact.offsets(sizes)
        m, q = segment_exact.case_masses("ragged%d" % k, off)
        st, T = segment_exact.seg_types(len(sizes))
        F = 7 * k
        return dict(off=off, m=m, q=q, st=st, T=T, attr=segment_exact.case_attr("ragged%d" % k, off, F, 3),
                    vel=segment_exact.case_vel("ragged%d" % k, off, F))
    return make


def _segment_com(k):
    def run(B, ctx, i, X):
        a = X.put(i["attr"])
        o = X.out((len(i["attr"]), 3, len(i["off"]) - 1))
        X.pre()
        return _done(B.segment_com(a, i["m"], i["off"], atom_q=i["q"], out=o, ctx=ctx, async_=X.async_), tuple, (o,))

    def ref(i):
        return (segment_exact.com(i["attr"], i["m"], i["off"]),) + tuple(segment_exact.seg_sums(i["m"], i["q"], i["off"]))
    return _seg_make(k), run, ref, same, ("attr",), lambda w: np.abs(w[0]).sum() > 0


def _charge_flux(k):
    def run(B, ctx, i, X):
        v = X.put(i["vel"])
        o = X.out((3, i["T"], len(i["vel"])))
        X.pre()
        return _done(B.charge_flux(v, i["m"], i["q"], i["off"], i["st"], i["T"], segment_exact.VEL_CONV,
                                   segment_exact.CHARGE_CONV, ctx=ctx, out=o, async_=X.async_), lambda r: (r,), (o,))

    def ref(i):
        return (segment_exact.flux(i["vel"], i["m"], i["q"], i["off"], i["st"], i["T"]),)
    return _seg_make(k), run, ref, same, ("vel",), lambda w: np.abs(w[0]).sum() > 0


_both("segment_com", _segment_com, has_out=True)
_both("charge_flux", _charge_flux, has_out=True)


# ================================================================================================ MSD
def _msd_make(k, seed):
    def make():
        rng = np.random.default_rng(seed + k)
        F, E = 9 * k, 65 * k
        go = np.array([0, E // 3, E // 3, E], dtype=np.int64)
        pairs = np.column_stack([np.zeros(F, np.int32), np.arange(F, dtype=np.int32)])
        return dict(r=k1024(rng, (F, 3, E)), go=go, pairs=pairs)
    return make


def _msd_pairs(k):
    def run(B, ctx, i, X):
        r = X.put(i["r"])
        X.pre()
        return (B.msd_pairs(r, i["pairs"], i["go"], ctx=ctx),)
    return (_msd_make(k, 40), run, lambda i: (cref.msd_pairs(i["r"], i["pairs"], i["go"]),), same, ("r",),
            lambda w: w[0].sum() > 0)


def _msd_origin(k):
    def run(B, ctx, i, X):
        r, origin = X.put(i["r"]), X.put(np.ascontiguousarray(i["r"][0]))
        o = X.out((len(i["r"]), len(i["go"]) - 1, 4))
        X.pre()
        return _done(B.msd_origin(r, origin, i["go"], out=o, ctx=ctx, async_=X.async_), lambda r: (r,), (o,))
    return (_msd_make(k, 41), run, lambda i: (cref.msd_pairs(i["r"], i["pairs"], i["go"]),), same, ("r",),
            lambda w: w[0].sum() > 0)


def _windows_check(got, want):
    """tests/test_gpu_launch_limits.py: the window sums as means equal oracle.cpu_ref.msd_fixed_lag (exact data)."""
    sums, (ref, n) = host(got[0]), want
    assert np.array_equal(sums[:, :3] / (n - 1), ref[:, :3]) and np.array_equal(sums[:, 3] / n, ref[:, 3])


def _msd_windows(k):
    tao = 2

    def run(B, ctx, i, X):
        r = X.put(i["r"])
        o = X.out((i["r"].shape[2], 4))
        X.pre()
        return _done(B.msd_windows(r, tao, ctx=ctx, out=o, async_=X.async_), lambda r: (r,), (o,))

    def ref(i):
        return cpu_ref.msd_fixed_lag(i["r"].transpose(0, 2, 1), tao), len(i["r"][::tao])
    return _msd_make(k, 42), run, ref, _windows_check, ("r",), lambda w: w[0].sum() > 0


_both("msd_pairs", _msd_pairs)
_both("msd_origin", _msd_origin, has_out=True)
_both("msd_windows", _msd_windows, has_out=True, arrays=lambda w: [w[0]])


MI355X = dict(cu_count=256, lds_bytes=163840)  # the device limits the plan is asked with where there is no device


def lag_planned(i, opts=None):
    """What the library plans for a lag_msd entry on an MI355X (mdhip_lag_plan: no device needed)."""
    from mdproptools_amd import backend

    return backend.lag_plan(i["xi"].shape[0], i["xi"].shape[2], i["max_lag"], i["go"], opts=opts, **MI355X)


def lag_padded(i, opts=None):
    return lag_planned(i, opts)["L"]


def _lag_make(F, E, go, gen, seed):
    def make():
        xi = lag_exact.GENERATORS[gen](np.random.default_rng(seed * 7919 + F), F, E)
        return dict(xi=xi, r=lag_exact.to_float(xi), go=np.asarray(go, dtype=np.int64), max_lag=F - 1)
    return make


def _lag_ref(opts):
    def ref(i):
        F = i["xi"].shape[0]
        go = [int(v) for v in i["go"]]
        return (lag_exact.exact_sums(i["xi"], i["max_lag"], go), lag_exact.energy(i["xi"], go), F, go,
                lag_padded(i, opts))
    return ref


def _lag_check(got, want):
    """tests/test_gpu_lag_exact.py: the per-lag criterion of a spectral path against the exact integer sums (the exact
    kernels, should one answer instead, meet it with room to spare)."""
    S, Q, F, go, L = want
    j = lag_exact.judge(host(got[0]), S, Q, F, go, L)
    assert j["frac"] <= 1.0, j
    assert (host(got[0])[0] == 0.0).all()


def _lag_msd(k):
    F = 300 * k

    def run(B, ctx, i, X):
        r = X.put(i["r"])
        o = X.out((i["max_lag"] + 1, len(i["go"]) - 1, 4))
        st = X.out((1,)) if X.async_ and o is not None else None
        X.pre()
        return _done(B.lag_msd(r, i["max_lag"], i["go"], ctx=ctx, out=o, async_=X.async_, status_out=st),
                     lambda r: (r,), (o,), st)
    return (_lag_make(F, 5, [0, 1, 1, 5], "white", 3), run, _lag_ref(None), _lag_check, ("r",),
            lambda w: w[0].sum() > 0)


_both("lag_msd", _lag_msd, has_out=True, arrays=lambda w: [w[0]])

VARIANT4 = {"lag_variant": 4}
# the residue-class path in 1 MB batches with the CU-partitioned pair of streams (csrc/msd_fft.hip: the fork and join
# of lag_msd_fft_residue) at the smallest shape that plans it: 8193 frames of 3 entities, five batches
OVERLAP = {"lag_variant": 2, "lag_residue": 1, "lag_batch_mb": 1, "lag_overlap": 2}


def _lag_with(opts):
    def run(B, ctx, i, X):
        """lag_msd under options of the context, set here and restored (-1: the default) whatever happens."""
        r = X.put(i["r"])
        o = X.out((i["max_lag"] + 1, len(i["go"]) - 1, 4))
        st = X.out((1,)) if X.async_ and o is not None else None
        for key, v in opts.items():
            ctx.set_option(key, v)
        try:
            X.pre()
            return _done(B.lag_msd(r, i["max_lag"], i["go"], ctx=ctx, out=o, async_=X.async_, status_out=st),
                         lambda r: (r,), (o,), st)
        finally:
            for key in opts:
                ctx.set_option(key, -1)
    return run


# (the batched transforms of lag_variant 4 share the roots of unity with the xcorr FFT)
_add("lag_msd_variant4", "lag_msd", "state", _lag_make(1100, 12, [0, 5, 12], "walk", 4), _lag_with(VARIANT4),
     _lag_ref(VARIANT4), _lag_check, ("r",), lambda w: w[0].sum() > 0, tags=("twiddle",), arrays=lambda w: [w[0]])
_add("lag_msd_overlap", "lag_msd", "state", _lag_make(8193, 3, [0, 1, 3], "white", 5), _lag_with(OVERLAP),
     _lag_ref(OVERLAP), _lag_check, ("r",), lambda w: w[0].sum() > 0, has_out=True, tags=("overlap",),
     arrays=lambda w: [w[0]])


# ================================================================================================ xcorr, scan
def xcorr_padded(n):
    """The xcorr FFT path pads a series of n samples to the next power of two of 2 n - 1."""
    return 1 << (2 * n - 1).bit_length()


def _series_make(P, n, seed, amp=50):
    def make():
        rng = np.random.default_rng(seed)
        return dict(a=rng.integers(-amp, amp + 1, (P, n)).astype(np.float64),
                    b=rng.integers(-amp, amp + 1, (P, n)).astype(np.float64))
    return make


def _xcorr_ref(i):
    return (np.stack([cref.xcorr_direct(a, b) for a, b in zip(i["a"], i["b"])]), i["a"], i["b"])


def _xcorr_check_direct(got, want):
    same((got[0],), (want[0],))


def _xcorr_check_fft(got, want):
    """tests/test_gpu_launch_limits.py: integer samples, the lag sums within 1e-13 |a| |b| per series."""
    c, a, b = want
    n = a.shape[1]
    w = n - np.arange(n)
    bound = 1e-13 * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    assert (np.abs(host(got[0]) * w - c * w).max(axis=1) <= bound).all()


def _xcorr_run(method):
    def run(B, ctx, i, X):
        a, b = X.put(i["a"]), X.put(i["b"])
        o = X.out(i["a"].shape)
        X.pre()
        return _done(B.xcorr(a, b, method=method, ctx=ctx, out=o, async_=X.async_), lambda r: (r,), (o,))
    return run


def _nz(w):
    return np.abs(w[0]).sum() > 0


_add("xcorr_fft_small", "xcorr", "small", _series_make(3, 257, 50), _xcorr_run(XCORR_FFT), _xcorr_ref,
     _xcorr_check_fft, ("a", "b"), _nz, has_out=True, tags=("twiddle",), arrays=lambda w: [w[0]])
_add("xcorr_fft_large", "xcorr", "large", _series_make(3, 4097, 51), _xcorr_run(XCORR_FFT), _xcorr_ref,
     _xcorr_check_fft, ("a", "b"), _nz, has_out=True, tags=("twiddle",), arrays=lambda w: [w[0]])
_add("xcorr_fft_small_again", "xcorr", "state", _series_make(3, 257, 52), _xcorr_run(XCORR_FFT), _xcorr_ref,
     _xcorr_check_fft, ("a", "b"), _nz, has_out=True, tags=("twiddle",), arrays=lambda w: [w[0]])
_add("xcorr_direct_small", "xcorr", "small", _series_make(3, 257, 53), _xcorr_run(XCORR_DIRECT), _xcorr_ref,
     _xcorr_check_direct, ("a", "b"), _nz, has_out=True, arrays=lambda w: [w[0]])
_add("xcorr_direct_large", "xcorr", "large", _series_make(3, 1028, 54), _xcorr_run(XCORR_DIRECT), _xcorr_ref,
     _xcorr_check_direct, ("a", "b"), _nz, has_out=True, arrays=lambda w: [w[0]])

SCAN_TILE = 2048  # increments per tile of the one-pass scan (csrc/scan.hip: SC_BLOCK)


def scan_tiles(shape):
    S, n = shape
    return S * (-(-(n - 1) // SCAN_TILE))


def _cumtrapz(shape, seed, dx):
    def make():
        return dict(y=np.random.default_rng(seed).integers(-100, 101, shape).astype(np.float64))

    def run(B, ctx, i, X):
        y = X.put(i["y"])
        o = X.out((shape[0], shape[1] - 1))
        X.pre()
        return _done(B.cumtrapz(y, dx, ctx=ctx, out=o, async_=X.async_), lambda r: (r,), (o,))

    def ref(i):  # integer samples, dx a power of two: numpy's cumsum is exact, in any order
        return (np.cumsum(dx * (i["y"][:, 1:] + i["y"][:, :-1]) / 2.0, axis=1),)
    return make, run, ref, same, ("y",), _nz


_add("cumtrapz_small", "cumtrapz", "small", *_cumtrapz((3, 1250), 60, 0.5), has_out=True, tags=("scan",))
_add("cumtrapz_large", "cumtrapz", "large", *_cumtrapz((3, 5000), 61, 0.5), has_out=True, tags=("scan",))
_add("cumtrapz_70_series", "cumtrapz", "state", *_cumtrapz((70, 300), 62, 0.5), has_out=True, tags=("scan",))
_add("cumtrapz_two_launches", "cumtrapz", "state", *_cumtrapz((5, 1_000_001), 63, 2.0), has_out=True,
     tags=("scan",))


def _gk_check(got, want):
    """tests/test_gpu_launch_limits.py: the direct correlation of integer samples exactly, the integral of that very
    correlation and its mean to rounding."""
    acf, integ, mean = (host(g) for g in got)
    assert np.array_equal(acf, want[0])
    for s in range(len(acf)):
        np.testing.assert_allclose(integ[s], cpu_ref.cumtrapz(acf[s], 0.5), rtol=1e-13,
                                   atol=1e-13 * np.abs(acf[s]).max())
    np.testing.assert_allclose(mean, integ.mean(axis=0), rtol=1e-12)


def _green_kubo(k):
    def run(B, ctx, i, X):
        a = X.put(i["a"])
        X.pre()
        return _done(B.green_kubo(a, method=XCORR_DIRECT, dx=0.5, want_mean=True, ctx=ctx, async_=X.async_), tuple)

    def ref(i):
        return (np.stack([cref.xcorr_direct(a, a) for a in i["a"]]),)
    return _series_make(3, 257 * k, 64 + k, amp=100), run, ref, _gk_check, ("a",), _nz


_both("green_kubo", _green_kubo, has_out=True, tags=("scan",))


# ================================================================================================ residence
def _residence(k):
    def make():
        F = 65 * k
        p = residence_design.patterns(F, seed=F)
        groups = [(p["always"], 2, 1), (p["run"], 1, 2), (p["periodic"], 3, 2), (p["random"], 2, 3), (p["ends"], 1, 1),
                  (p["never"], 2, 2)]
        d = residence_design.designed(groups, seed=F)
        return dict(xi=d.xi, xj=d.xj, box=d.box)

    def run(B, ctx, i, X):
        xi, xj = X.put(i["xi"]), X.put(i["xj"])
        X.pre()
        lo, hi = residence_design.LO, residence_design.HI
        return tuple(B.shell_residence(xi, xj, i["box"], lo * lo, hi * hi, ctx=ctx))

    def ref(i):
        return tuple(residence_design.oracle_counts(residence_design.Design(i["xi"], i["xj"], i["box"], None, None)))
    return make, run, ref, same, ("xi", "xj"), _hist_hits(0)


_both("shell_residence", _residence)


# ================================================================================================ shell searches
def _clumps(seed, F, n_mols, L=16.0):
    """Molecules of 1-8 atoms as clumps on a 1/4 grid, some across a face (the system of tests/test_gpu_clusters.py and
    tests/test_gpu_configurations.py, types and classes included)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 9, n_mols)
    mol_of = np.repeat(np.arange(n_mols), sizes).astype(np.int32)
    seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    N = len(mol_of)
    base = rng.integers(0, 8, (F, 3, n_mols)).astype(np.float64) * (L / 8)
    xyz = np.mod(base[:, :, mol_of] + rng.integers(-3, 4, (F, 3, N)) / 4.0, L)
    mol_type = rng.integers(1, 4, n_mols).astype(np.int32)
    cls = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), N)
    centres = np.unique(np.concatenate(([0], 1 + rng.choice(N - 2, 15, replace=False), [N - 1]))).astype(np.int32)
    passes = rng.uniform(size=(F, n_mols)) < 0.7
    return dict(xyz=xyz, box=np.full((F, 3), L), mol_of=mol_of, seg_off=seg_off, mol_type=mol_type, cls=cls,
                centres=centres, passes=passes, force=rng.normal(0.0, 1.0, (F, 3, N)) * 10.0 ** rng.uniform(-3, 3, N))


def _pad_rows(rows, pad, dtype, width=None):
    """Ragged [F][C] lists as the padded array the library returns, K = max(width, the longest row)."""
    big = max([len(r) for fr in rows for r in fr] + [width or 1])
    out = np.full((len(rows), len(rows[0]), big), pad, dtype=dtype)
    for f, fr in enumerate(rows):
        for c, r in enumerate(fr):
            out[f, c, :len(r)] = r
    return out, np.array([[len(r) for r in fr] for fr in rows], dtype=np.int32)


_PAD = {"i": lambda t: -1, "u": lambda t: np.iinfo(t).max, "f": lambda t: np.nan}


def _rows_same(got, want):
    """The counts, the rows up to the restatement's width, and the library's padding beyond it (K = max(cap, largest
    row): the cap is not part of the answer)."""
    *g_rows, g_count = (host(v) for v in got)
    *w_rows, w_count = want
    assert np.array_equal(g_count, w_count)
    for g, w in zip(g_rows, w_rows):
        k = w.shape[2]
        assert g.shape[2] >= k and g.dtype == w.dtype
        same((g[:, :, :k],), (w,))
        same((g[:, :, k:],), (np.full(g[:, :, k:].shape, _PAD[g.dtype.kind](g.dtype), dtype=g.dtype),))


def _members_ref(r_cut):
    def ref(i):
        rows = [[cluster_ref.shell(i["xyz"][f], i["box"][f], p, i["mol_of"], r_cut ** 2) for p in i["centres"]]
                for f in range(len(i["xyz"]))]
        return _pad_rows(rows, -1, np.int32)
    return ref


def _shell_members(k, cap=None, r_cut=2.5):
    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.shell_members(x, i["box"], i["centres"], i["mol_of"], r_cut ** 2, ctx=ctx,
                                     **({} if cap is None else {"cap": cap})))
    return (lambda: _clumps(70, 3 * k, 150), run, _members_ref(r_cut), _rows_same, ("xyz",),
            lambda w: w[1].max() > 1)


def _shell_coordination(k):
    rs2, rc2 = 2.5 ** 2, 2.0 ** 2

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.shell_coordination(x, i["box"], i["centres"], i["mol_of"], i["seg_off"], i["mol_type"],
                                          i["cls"], rs2, rc2, passes=i["passes"], ctx=ctx))

    def ref(i):
        rows = config_ref.coordination_rows(i["xyz"], i["box"], i["centres"], i["mol_of"], i["seg_off"], i["mol_type"],
                                            i["cls"], rs2, rc2, i["passes"])
        mols, count = _pad_rows([[[m for m, _ in e] for e in fr] for fr in rows], -1, np.int32)
        words, _ = _pad_rows([[[w for _, w in e] for e in fr] for fr in rows], np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        return mols, words, count
    return (lambda: _clumps(72, 3 * k, 150), run, ref, _rows_same, ("xyz",), lambda w: w[2].max() > 1)


def _mol_kahan(k):
    def run(B, ctx, i, X):
        a = X.put(i["force"])
        X.pre()
        return (B.mol_kahan_sums(a, i["seg_off"], ctx=ctx),)

    def ref(i):
        return (np.stack([np.stack([cluster_ref.kahan_sums(i["force"][f, a], i["seg_off"]) for a in range(3)])
                          for f in range(len(i["force"]))]),)
    return lambda: _clumps(74, 3 * k, 150), run, ref, same_bytes, ("force",), _nz


_both("shell_members", _shell_members)
_both("shell_coordination", _shell_coordination)
_both("mol_kahan_sums", _mol_kahan)


def _waters(seed, F, n_ion, n_wat, L):
    """Ions, then O H1 H2 per water, on a grid of 0.001 (the system of tests/test_gpu_hydration.py without its planted
    atoms)."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    n = n_ion + 3 * n_wat
    xyz = np.round(rng.uniform(0, 1, (F, 3, n)) * L[None, :, None], 3)
    o = n_ion + 3 * np.arange(n_wat)
    for h in (1, 2):
        xyz[:, :, o + h] = np.round(xyz[:, :, o] + rng.normal(0, 0.6, (F, 3, n_wat)), 3)
    return dict(xyz=xyz, box=np.tile(L, (F, 1)), ions=np.arange(n_ion), wat=o)


def _hyd_frames(i):
    return [dict(xyz=i["xyz"][f], bounds=np.column_stack([np.zeros(3), i["box"][f]]), timestep=f)
            for f in range(len(i["xyz"]))]


HYD_R = 3.5


def _hydration_cosines(k, cap=None):
    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.hydration_cosines(x, i["box"], i["ions"], i["wat"], HYD_R ** 2, ctx=ctx,
                                         **({} if cap is None else {"cap": cap})))

    def ref(i):
        rows = [hydration_ref.frame_rows(fr, i["ions"], i["wat"], HYD_R) for fr in _hyd_frames(i)]
        idx, count = _pad_rows([[sel for sel, _ in fr] for fr in rows], -1, np.int32)
        cos, _ = _pad_rows([[c for _, c in fr] for fr in rows], np.nan, np.float64)
        return idx, cos, count

    def check(got, want):
        _rows_same(got, want)
        g, w, count = host(got[1]), want[1], want[2]
        for f, c in np.ndindex(count.shape):  # the cosines bit for bit, as tests/test_gpu_hydration.py holds them
            assert g[f, c, :count[f, c]].tobytes() == w[f, c, :count[f, c]].tobytes(), (f, c)
    return (lambda: _waters(76 + k, 2 * k, 17, 80, [16.0, 16.0, 6.0]), run, ref, check, ("xyz",),
            lambda w: w[2].max() > 1)


def _hydration_counts(k):
    nb = 100 * k

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.hydration_counts(x, i["box"], i["ions"], i["wat"], HYD_R ** 2, hydration_ref.COS_CUT, 2.0 / nb,
                                        nb, ctx=ctx))

    def ref(i):
        return tuple(hydration_ref.counts(_hyd_frames(i), 1, 2, HYD_R, [len(i["ions"]), len(i["wat"])], [1, 3],
                                          cos_bin_size=2.0 / nb))
    return (lambda: _waters(78 + k, 2 * k, 17 * k, 80 * k, _grown([16.0, 16.0, 6.0], k)), run, ref, same, ("xyz",),
            _hist_hits(2))


_both("hydration_cosines", _hydration_cosines)
_both("hydration_counts", _hydration_counts)


def _angle(k, cap=None, r_cut=3.0):
    trip = [(2, 1, 2), (2, 1, 3), (3, 1, 3), (3, 1, 2)][:k]

    def make():
        xyz, box = _gas(80 + k, 2 * k, 201 * k, _grown([12.0, 9.0, 6.0], k))
        return dict(xyz=xyz, box=box, types=np.arange(xyz.shape[2]) % 3 + 1,
                    rc2=np.full((len(trip), 2), r_cut ** 2), edges=angular_ref.cos_edges(1.0))

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.angle_hist(x, i["box"], i["types"], trip, i["rc2"], i["edges"], ctx=ctx,
                                  **({} if cap is None else {"cap": cap})))

    def ref(i):
        return tuple(angular_ref.angle_hist(i["xyz"], i["box"], i["types"], trip, i["rc2"], i["edges"]))
    return make, run, ref, same, ("xyz",), _hist_hits(0)


_both("angle_hist", _angle)

# the row-cap re-runs: a cap below the fullest row of the input (asserted on the CPU), so the library goes round again
_add("shell_members_capped", "shell_members", "state", *_shell_members(1, cap=2), tags=("capped",))
_add("hydration_cosines_capped", "hydration_cosines", "state", *_hydration_cosines(1, cap=4), tags=("capped",))
_add("angle_hist_capped", "angle_hist", "state", *_angle(1, cap=8), tags=("capped",))
CAPS = {"shell_members_capped": (2, 1), "hydration_cosines_capped": (4, 2), "angle_hist_capped": (8, 2)}


# ================================================================================================ SDF, aggregates, H-bonds
def _sdf_make(k):
    def make():
        n_mols = 17 * k
        n = 3 * n_mols + 150 * k
        xyz, box = _gas(82 + k, 2, n, _grown([9.0, 8.0, 7.0], k))
        o = 3 * np.arange(n_mols)
        cand = np.arange(3 * n_mols, n)
        return dict(xyz=xyz, box=box, o=o, cand=cand, cls=cand % (2 * k), S=2 * k, r_cut=3.0,
                    bin_size=0.5 if k == 1 else 0.3)
    return make


def _body_frames(k):
    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.body_frames(x, i["box"], i["o"], i["o"] + 1, i["o"] + 2, ctx=ctx))

    def ref(i):
        e, valid = sdf_ref.body_frames(i["xyz"], i["box"], i["o"], i["o"] + 1, i["o"] + 2)
        return e, valid, int((~valid).sum())

    def check(got, want):
        e, valid, bad = (host(g) for g in got)
        assert np.array_equal(valid, want[1]) and bad == want[2]
        assert reorientation_ref.same_bits(e[valid], np.asarray(want[0])[want[1]])
    return _sdf_make(k), run, ref, check, ("xyz",), lambda w: np.asarray(w[1]).any()


def _sdf_hist(k):
    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.sdf_hist(x, i["box"], i["o"], i["o"] + 1, i["o"] + 2, i["cand"], i["cls"], i["S"], i["r_cut"],
                                i["bin_size"], ctx=ctx))

    def ref(i):
        return tuple(sdf_ref.sdf_hist(i["xyz"], i["box"], i["o"], i["o"] + 1, i["o"] + 2, i["cand"], i["cls"], i["S"],
                                      i["r_cut"], i["bin_size"]))
    return _sdf_make(k), run, ref, same, ("xyz",), _hist_hits(0)


_both("body_frames", _body_frames)
_both("sdf_hist", _sdf_hist)


def _contact(k):
    def make():
        xyz, box = _gas(84 + k, 2 * k, 201 * k, _grown([12.0, 9.0, 6.0], k))
        aa, ca, ab, cb, cut = aggregates_ref.lists(np.arange(xyz.shape[2]) % 3 + 1, [(1, 2, 1.5), (2, 3, 1.25)])
        return dict(xyz=xyz, box=box, aa=aa, ca=ca, ab=ab, cb=cb, cut=cut, node_of=np.arange(xyz.shape[2]))

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.contact_components(x, i["box"], i["aa"], i["ca"], i["ab"], i["cb"], i["cut"], i["node_of"],
                                          len(i["node_of"]), ctx=ctx))

    def ref(i):
        return tuple(aggregates_ref.contact_components(i["xyz"], i["box"], i["aa"], i["ca"], i["ab"], i["cb"], i["cut"],
                                                       i["node_of"], len(i["node_of"])))
    return make, run, ref, same, ("xyz",), _hist_hits(2)


_both("contact_components", _contact)

R_DA = 3.5
COS150 = float(np.cos(np.radians(150.0)))


def _hb_make(k, F):
    def make():
        n_don, n_acc = 33 * k, 150 * k
        rng = np.random.default_rng(86 + k)
        L = _grown([9.0, 8.0, 7.0], k)
        n = 2 * n_don + n_acc
        xyz = np.round(rng.uniform(0, 1, (F, 3, n)) * L[None, :, None], 3)
        for d in range(n_don):  # one hydrogen 0.95 from its donor, wrapped on its own (tests/test_gpu_hbonds.py)
            u = rng.normal(size=(F, 3))
            u *= 0.95 / np.linalg.norm(u, axis=1)[:, None]
            xyz[:, :, n_don + d] = np.round(np.mod(xyz[:, :, d] + u, L[None]), 3)
        return dict(xyz=xyz, box=np.tile(L, (F, 1)), don=np.arange(n_don, dtype=np.int32),
                    dcl=(np.arange(n_don) % 2).astype(np.int32), h_off=np.arange(n_don + 1, dtype=np.int32),
                    h_atoms=(n_don + np.arange(n_don)).astype(np.int32),
                    acc=(2 * n_don + np.arange(n_acc)).astype(np.int32), acl=(np.arange(n_acc) % 2).astype(np.int32),
                    edges=angular_ref.cos_edges(2.0 / k))
    return make


def _hbond_counts(k):
    cos_cut = float(np.cos(np.radians(110.0)))

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.hbond_counts(x, i["box"], i["don"], i["dcl"], i["h_off"], i["h_atoms"], i["acc"], i["acl"],
                                    R_DA ** 2, cos_cut, cos_edges=i["edges"], n_dc=2, n_ac=2, ctx=ctx))

    def ref(i):
        return tuple(hbonds_ref.hbond_counts(i["xyz"], i["box"], i["don"], i["dcl"], i["h_off"], i["h_atoms"], i["acc"],
                                             i["acl"], R_DA ** 2, cos_cut, edges=i["edges"], n_dc=2, n_ac=2))
    return _hb_make(k, 2 * k), run, ref, same, ("xyz",), _hist_hits(0)


def _hbond_lifetime(k):
    cos_cut = float(np.cos(np.radians(110.0)))

    def run(B, ctx, i, X):
        x = X.put(i["xyz"])
        X.pre()
        return tuple(B.hbond_lifetime(x, i["box"], i["don"], i["h_off"], i["h_atoms"], i["acc"], R_DA ** 2, cos_cut,
                                      ctx=ctx))

    def ref(i):
        return tuple(hbonds_ref.hbond_lifetime(i["xyz"], i["box"], i["don"], i["h_off"], i["h_atoms"], i["acc"],
                                               R_DA ** 2, cos_cut))
    return _hb_make(1, 3 * k), run, ref, same, ("xyz",), _hist_hits(0)


_both("hbond_counts", _hbond_counts)
_both("hbond_lifetime", _hbond_lifetime)


# ================================================================================================ axis profile
def _axis_profile(k):
    W, D, NB, ROWS = 0.5, 12.0, 24 * k, 3

    def make():
        rng = np.random.default_rng(88 + k)
        F, n = 6 * k, 257
        x = np.round(rng.uniform(-10.0, 30.0, (F, n)), 3)
        row = rng.integers(-1, ROWS, (F, n))
        surf = np.zeros((F, n), dtype=bool)
        surf[:, :20] = True
        x[:, :20] = np.round(rng.uniform(1.0, 5.0, (F, 20)), 3)
        surf[3] = False  # a frame without a surface
        code = np.where(row < 0, 0x3FFF, row) | np.where(surf, 0x4000, 0)
        return dict(x=x, codes=code.astype(np.uint16))

    def run(B, ctx, i, X):
        x = X.put(i["x"])
        X.pre()
        return tuple(B.axis_profile(x, i["codes"], B.AP_REF_POS, W / k, D, NB, ROWS, ctx=ctx))

    def ref(i):
        return tuple(number_density_ref.axis_profile(i["x"], i["codes"], 0, W / k, D, NB, ROWS))

    def check(got, want):  # tests/test_gpu_number_density.py: the counts equal, the extents to their bytes
        same((got[0], got[2]), (want[0], want[2]))
        assert np.ascontiguousarray(host(got[1])).tobytes() == np.ascontiguousarray(want[1]).tobytes()
    return make, run, ref, check, ("x",), _hist_hits(0)


for _size, _k in K.items():
    _add("axis_profile_%s" % _size, "axis_profile", _size, *_axis_profile(_k))


# ================================================================================================ displacement, van Hove
def _walk_make(k, seed, E):
    def make():
        F = 23 * k
        x, box = displacement_ref.grid_walk(seed + k, F, E)
        return dict(x=x, box=box, off=displacement_ref.three_groups(E), F=F)
    return make


def _displacement(k):
    def jobs(F):
        if k == 1:
            return [(0, 1, 1), (2, F // 3, 4), (2, F - 1, 1)]
        return [(g, lag, s) for g in (0, 2) for lag in (1, F // 3, F - 1) for s in (1, 4)]

    def run(B, ctx, i, X):
        x = X.put(i["x"])
        X.pre()
        return tuple(B.displacement_hist(x, i["box"], i["off"], jobs(i["F"]), 0.5, 12, ctx=ctx))

    def ref(i):
        return tuple(displacement_ref.displacement_hist(i["x"], i["box"], i["off"], jobs(i["F"]), 0.5, 12))

    def check(got, want):  # tests/test_gpu_displacement.py
        same(got[:3] + (got[4],), want[:3] + (want[4],))
        assert displacement_ref.moments_close(host(got[3]), want[3], want[2])
    return (_walk_make(k, 90, 65), run, ref, check, ("x",),
            lambda w: np.asarray(w[0]).sum() > 0 and np.asarray(w[1]).sum() > 0)


def _van_hove(k):
    def jobs(F):
        pairs = ((0, 0), (0, 2), (2, 0)) if k == 1 else ((0, 0), (2, 2), (0, 2), (2, 0), (0, 1), (1, 2))
        return [(a, b, lag, 1) for a, b in pairs for lag in ((1,) if k == 1 else (0, F - 1))]

    def run(B, ctx, i, X):
        x = X.put(i["x"])
        X.pre()
        return tuple(B.van_hove_distinct(x, i["box"], i["off"], jobs(i["F"]), 0.25, 24, ctx=ctx))

    def ref(i):
        return tuple(vanhove_ref.van_hove_distinct(i["x"], i["box"], i["off"], jobs(i["F"]), 0.25, 24))
    return (_walk_make(k, 92, 65), run, ref, same, ("x",),
            lambda w: np.asarray(w[0]).sum() > 0 and np.asarray(w[1]).sum() > 0)


_both("displacement_hist", _displacement)
_both("van_hove_distinct", _van_hove)


# ================================================================================================ collective, reorientation
def _collective(k):
    def make():
        r, w = einstein_ref.int_walk(94 + k, 129 * k, 65)
        return dict(r=r, w=w, off=np.array([0, 20, 20, 65], dtype=np.int64))

    def run(B, ctx, i, X):
        r = X.put(i["r"])
        o = X.out((len(i["off"]) - 1, 3, len(i["r"])))
        X.pre()
        return (B.collective_displacement(r, i["w"], i["off"], scale=1.0, out=o, ctx=ctx),)
    return (make, run, lambda i: (einstein_ref.collective(i["r"], i["w"], 1.0, i["off"])[0],), same, ("r",), _nz)


def _cross_msd(k):
    def make():
        return dict(P=einstein_ref.int_series(96 + k, 3, 129 * k))

    def run(B, ctx, i, X):
        P = X.put(i["P"])
        n = i["P"].shape[2]
        o = X.out((n, 3, 3))
        X.pre()
        return (B.cross_msd(P, n - 1, out=o, ctx=ctx),)

    def ref(i):
        sums, cnt = einstein_ref.cross_msd_exact_int(i["P"], i["P"].shape[2] - 1)
        return (sums / cnt[:, None, None].astype(np.float64),)
    return make, run, ref, same, ("P",), _nz


def _axis_vectors(k):
    terms = [[(1, -1.0), (3, 1.0)], [(2, 1.0)], [(1, 0.5), (2, -0.25)], [(3, 1.0)]][:k]

    def make():
        rng = np.random.default_rng(98 + k)
        F, mols, per = 65 * k, 17, 4
        L = 9.0 + rng.random((F, 3))
        centre = rng.random((F, 3, mols, 1)) * L[:, :, None, None]
        x = centre + rng.normal(0.0, 0.7, size=(F, 3, mols, per))
        return dict(x=np.ascontiguousarray(np.mod(x, L[:, :, None, None]).reshape(F, 3, mols * per)), box=L,
                    a0=np.zeros(k, dtype=np.int64), mols=[mols] * k, length=[per] * k)

    def run(B, ctx, i, X):
        x = X.put(i["x"])
        o = X.out((sum(i["mols"]), 3, len(i["x"])))
        X.pre()
        return tuple(B.axis_vectors(x, i["box"], i["a0"], i["mols"], i["length"], terms, out=o, ctx=ctx))

    def ref(i):
        return tuple(reorientation_ref.axis_vectors(i["x"], i["box"], i["a0"], i["mols"], i["length"], terms))
    return make, run, ref, same_signed, ("x",), _nz


def _orient_corr(k):
    def make():
        n = 129 * k
        return dict(U=reorientation_ref.axis_series(np.random.default_rng(100 + k), 17, n),
                    off=np.array([0, 5, 5, 17], dtype=np.int64), max_lag=n - 1)

    def run(B, ctx, i, X):
        U = X.put(i["U"])
        o = X.out((i["max_lag"] + 1, len(i["off"]) - 1, 2))
        X.pre()
        return (B.orient_corr(U, i["off"], i["max_lag"], out=o, ctx=ctx),)
    return (make, run, lambda i: (reorientation_ref.orient_sums_int(i["U"], i["off"], i["max_lag"]),), same, ("U",),
            _nz)


_both("collective_displacement", _collective, has_out=True)
_both("cross_msd", _cross_msd, has_out=True)
_both("axis_vectors", _axis_vectors, has_out=True)
_both("orient_corr", _orient_corr, has_out=True)


# ================================================================================================ refused calls
def _refused_einval(B, ctx, i, X):
    """mdhip_cross_msd with 17 groups (tests/test_gpu_einstein.py: test_invalid_arguments_are_refused_by_the_library):
    MDHIP_EINVAL before anything is written."""
    from mdproptools_amd._lib import MdhipError

    try:
        B.cross_msd(i["P"], 3, ctx=ctx)
    except MdhipError as e:
        assert e.code == -1, e
        return ()
    raise AssertionError("17 groups were not refused")


def _refused_python(B, ctx, i, X):
    """van_hove_distinct without a box: refused by the wrapper (ValueError) before the library is entered."""
    try:
        B.van_hove_distinct(i["P"], None, [0, 8], [(0, 0, 0, 1)], 0.25, 4, ctx=ctx)
    except ValueError:
        return ()
    raise AssertionError("a missing box was not refused")


for _name, _run in (("refused_einval", _refused_einval), ("refused_python", _refused_python)):
    _add(_name, "refused", "state", lambda: dict(P=np.zeros((17, 3, 8))), _run, lambda i: (), same, (), None,
         device=False, tags=("refused",))


# ================================================================================================ the order
# State entries sit where the state they exercise is live: the three transform lengths and the batched MSD transforms in
# a row; the scan's one-launch, 70-series and two-launch calls with a Green-Kubo chain between them; each row-cap re-run
# followed by the small variant of another shell-search consumer; the two asynchronous pair calls left in flight with an
# exclusive call of a newer family and a cumtrapz directly behind them; a refused call between two entries, twice.
_add("cumtrapz_behind_pairs", "cumtrapz", "state", *_cumtrapz((3, 1250), 65, 0.5), has_out=True, tags=("scan",))
_HEAD = [
    "rdf_loop_small", "msd_origin_small", "shell_residence_small", "van_hove_distinct_large", "green_kubo_large",
    "xcorr_fft_small", "xcorr_fft_large", "xcorr_fft_small_again", "lag_msd_variant4",
    "cumtrapz_large", "cumtrapz_70_series", "green_kubo_small", "cumtrapz_two_launches", "cumtrapz_small",
    "shell_members_capped", "hydration_counts_small", "hydration_cosines_capped", "shell_coordination_small",
    "angle_hist_capped", "shell_members_small",
    "rdf_loop_culled", "rdf_cn_loop_small",
    "rdf_loop_async", "rdf_cn_loop_async", "van_hove_distinct_small", "sdf_hist_small", "orient_corr_small",
    "cumtrapz_behind_pairs",
    "refused_einval", "cross_msd_small", "refused_python", "displacement_hist_small",
]
ORDER = _HEAD + [n for n in DECK if n not in _HEAD]
assert sorted(ORDER) == sorted(DECK)

PUBLIC = ("rdf_loop", "rdf_cn_loop", "cn_loop", "rdf_mol_loop", "cn_mol_loop", "segment_com", "charge_flux", "msd_pairs",
          "msd_origin", "msd_windows", "lag_msd", "xcorr", "cumtrapz", "green_kubo", "shell_residence", "shell_members",
          "shell_coordination", "mol_kahan_sums", "hydration_cosines", "hydration_counts", "angle_hist", "body_frames",
          "sdf_hist", "contact_components", "hbond_counts", "hbond_lifetime", "axis_profile", "displacement_hist",
          "van_hove_distinct", "collective_displacement", "cross_msd", "axis_vectors", "orient_corr")


def entries(order=None):
    return [DECK[n] for n in (ORDER if order is None else order)]
