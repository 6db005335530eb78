"""
Call-order independence: the deck of tests/call_deck.py, every public kernel entry of backend.py small and large, on
ONE context in many orders, on a caller's stream, on two contexts at once and over context turnover. Every family's own
file calls it on a context that has run nothing else; a context is not stateless between calls, and what it keeps is
exercised here by these entries:

  WS_FFT_TW (roots of unity, rebuilt when fft_tw_logL / fft_tw_ptr change; shared by the xcorr FFT path and the batched
      full-lag MSD transforms)          xcorr_fft_small (L 1024), xcorr_fft_large (L 16384), xcorr_fft_small_again,
                                        lag_msd_variant4 (L 4096), in a row
  WS_SCAN (two sets of totals, stall word, carries at an offset of max(n_series, 64); scan_capacity, scan_parity flip
      per launch)                       cumtrapz_large (one launch: the parity flips), cumtrapz_70_series (the carries
                                        move), green_kubo_small, cumtrapz_two_launches (parity unchanged), cumtrapz_small,
                                        cumtrapz_behind_pairs
  the shared workspace slots (WS_XYZ_I, WS_OUT, WS_MISC, WS_AUX0..3, WS_PART, WS_HIST: never shrunk, never cleared)
                                        every family small after large and large after small: the orders large_small
                                        and small_large, the listed order, its reverse and the two shuffles
  the row-cap re-run of the shell-search consumers
                                        shell_members_capped, hydration_cosines_capped, angle_hist_capped, each followed
                                        by the small variant of another consumer
  lanes (pair_flip, lane1_busy, excl_busy, events), stage_used / stage_flip, the H2D ring's cursor and events
                                        rdf_loop_small (dense), rdf_loop_culled, rdf_cn_loop_small (one sweep),
                                        rdf_loop_async + rdf_cn_loop_async left in flight with van_hove_distinct_small,
                                        sdf_hist_small, orient_corr_small and cumtrapz_behind_pairs directly behind
  the deferred error / the completion of a call on behalf of a later one; the last_* registers
                                        refused_einval, refused_python (the next entry is unaffected); the in-flight
                                        pair calls are completed by the calls behind them; last_kernel_name() is that of
                                        the call just made, after every call
  the pinned-block free list and the process-wide PinnedPool, the cached default context
                                        cumtrapz_two_launches (a 40 MB result) dropped and asked for again by the next
                                        context in test_context_turnover; green_kubo_large, xcorr_fft_large;
                                        test_the_default_context_after_whatever_ran_before
  mdhip_set_stream, as_input / _dev_out without their host synchronisation, the CU-masked part streams of
      msd_fft.hip, the copy stream, the re-runs in completion steps
                                        test_on_a_callers_stream (every entry, inputs arriving late on the stream),
                                        lag_msd_overlap (the fork and join), test_current_stream_is_not_the_contexts

`alone[name]` is each entry on a fresh Context(0) that has run nothing else, checked once against the restatement with
the family's own criterion; everything else is compared with `alone` by bytes.
"""
import gc
import random
from types import SimpleNamespace

import numpy as np
import pytest

import call_deck as D

pytestmark = pytest.mark.gpu

SHUFFLE_SEEDS = (20261019, 977)
REWRITTEN_AT_COMPLETION = ("rdf_loop_dev",)
LAG_BOUND_OK = 1e-10  # csrc/msd.hip: the bound up to which the spectral full-lag result is kept
DELAY_MATMULS = 12  # 4096 x 4096 float32 products ahead of every late input (a few milliseconds on an MI355X)


@pytest.fixture(scope="module")
def env():
    import torch

    from mdproptools_amd import backend
    from mdproptools_amd._lib import Context

    inputs = {name: D.DECK[name].make() for name in D.ORDER}
    return SimpleNamespace(B=backend, torch=torch, Context=Context, inputs=inputs)


def _finished(r):
    r = r.finish() if isinstance(r, D.Deferred) else r
    return tuple(D.host(v) for v in r)


def _alone_run(env, name):
    ctx = env.Context(0)
    try:
        r = _finished(D.DECK[name].call(env.B, ctx, env.inputs[name]))
        return SimpleNamespace(result=r, bytes=D.as_bytes(r), fallbacks=ctx.fallbacks(), kernel=ctx.last_kernel_name())
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def alone(env):
    return {name: _alone_run(env, name) for name in D.ORDER}


def test_alone_results_match_the_restatements(env, alone):
    """The anchor: every entry, alone on a fresh context, against its family's restatement with that family's criterion."""
    bad = []
    for name in D.ORDER:
        e = D.DECK[name]
        try:
            e.check(alone[name].result, e.reference(env.inputs[name]))
        except AssertionError as err:
            bad.append("%s: %s" % (name, str(err)[:300]))
    assert not bad, "\n".join(bad)


def test_two_fresh_contexts_agree_in_bytes(env, alone):
    """Byte equality with `alone` means something only if `alone` is reproducible: a second fresh context per entry."""
    differ = [name for name in D.ORDER if _alone_run(env, name).bytes != alone[name].bytes]
    assert not differ, differ


def _differences(name, got, want_bytes):
    got = D.as_bytes(got)
    if len(got) != len(want_bytes):
        return ["%s: %d results, alone %d" % (name, len(got), len(want_bytes))]
    return ["%s[%d] differs from the call alone" % (name, k) for k, (g, w) in enumerate(zip(got, want_bytes)) if g != w]


def run_sequence(env, ctx, names, alone, device=False):
    """The entries `names` on `ctx`, in-flight entries completed at the end -> the list of disagreements with `alone`."""
    bad, flying, want_fallbacks = [], [], ctx.fallbacks()
    for name in names:
        e = D.DECK[name]
        r = e.call(env.B, ctx, env.inputs[name], device=device and e.device)
        want_fallbacks += alone[name].fallbacks
        if isinstance(r, D.Deferred):
            flying.append((name, r))
            continue
        bad += _differences(name, r, alone[name].bytes)
        if "refused" not in e.tags and ctx.last_kernel_name() != alone[name].kernel:
            bad.append("%s: last_kernel_name() %r, alone %r" % (name, ctx.last_kernel_name(), alone[name].kernel))
    for name, d in flying:
        bad += _differences(name, d.finish(), alone[name].bytes)
    assert ctx.pending() == 0
    assert ctx.fallbacks() == want_fallbacks
    return bad


def _orders():
    listed = list(D.ORDER)
    large = [n for n in listed if D.DECK[n].size == "large"]
    small = [n for n in listed if D.DECK[n].size == "small"]
    state = [n for n in listed if D.DECK[n].size == "state"]
    out = {"listed": listed, "reversed": listed[::-1], "large_small": large + state + small,
           "small_large": small + state + large}
    for seed in SHUFFLE_SEEDS:
        order = list(listed)
        random.Random(seed).shuffle(order)
        out["shuffle_%d" % seed] = order
    return out


ORDERS = _orders()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_context_any_order(env, alone, order, form):
    ctx = env.Context(0)
    try:
        bad = run_sequence(env, ctx, ORDERS[order], alone, device=form == "device")
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_the_default_context_after_whatever_ran_before(env, alone):
    """The process-wide default context: in a run of the whole suite it has served every other test file by now."""
    ctx = env.B.default_context()
    bad = run_sequence(env, ctx, D.ORDER, alone)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- a caller's stream
class Late(D.Stage):
    """Inputs that arrive LATE on the stream `S`: the tensor is allocated and filled with NaN, a chain of large products
    is queued, then the real input as a non-blocking copy from page-locked memory; pre() asserts that the copy has not
    happened when the library is called. Result buffers (where the entry takes one) are NaN-filled device tensors and
    the call is asynchronous."""

    def __init__(self, env, ctx, S, pinned, use_out):
        self.torch, self.ctx, self.S, self.pinned = env.torch, ctx, S, pinned
        self.use_out = self.async_ = use_out
        self.dev = "cuda:%d" % ctx.device
        self.events, self.keep = [], []
        self.spin = env.torch.full((4096, 4096), 1.0 / 4096, dtype=env.torch.float32, device=self.dev)

    def put(self, a):
        torch = self.torch
        src = self.pinned.get(id(a))
        if src is None:
            src = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
        t = torch.full(tuple(a.shape), float("nan"), dtype=torch.float64, device=self.dev)
        x = self.spin
        for _ in range(DELAY_MATMULS):
            x = x @ self.spin
        t.copy_(src, non_blocking=True)
        produced = torch.cuda.Event()
        produced.record(self.S)
        self.events.append(produced)
        self.keep.append(src)
        return t

    def out(self, shape, dtype="float64"):
        if not self.use_out:
            return None
        torch = self.torch
        if dtype == "int64":
            return torch.full(tuple(shape), -1, dtype=torch.int64, device=self.dev)
        return torch.full(tuple(shape), float("nan"), dtype=torch.float64, device=self.dev)

    def pre(self):
        assert self.events, "no device input"
        assert not any(ev.query() for ev in self.events), "the input had arrived before the call: lengthen the delay"


def _pinned_inputs(env, names):
    pinned = {}
    for name in names:
        for k in D.DECK[name].staged:
            a = env.inputs[name][k]
            pinned[id(a)] = env.torch.from_numpy(a).pin_memory()
    return pinned


def _late_sequence(env, ctx, S, names, alone, consume=True):
    """`names` with late inputs on the current stream S, no host synchronisation until the end -> disagreements.
    `consume`: S is the context's stream too, so a copy queued on it behind a call is ordered behind that call."""
    torch = env.torch
    pinned = _pinned_inputs(env, names)
    bad, flying, late = [], [], 0
    for name in names:
        e = D.DECK[name]
        if not e.device:
            bad += _differences(name, e.call(env.B, ctx, env.inputs[name]), alone[name].bytes)
            continue
        stage = Late(env, ctx, S, pinned, e.has_out)
        r = e.call(env.B, ctx, env.inputs[name], stage=stage)
        late += len(stage.events)
        want = D.as_bytes(e.out_form(alone[name].result)) if e.has_out else alone[name].bytes
        if isinstance(r, D.Deferred):
            copies = []
            for o in (r.outs + (() if r.status is None else (r.status,))) if consume else ():
                # the consumer: a non-blocking copy to page-locked memory, on S, behind the call
                h = torch.empty(o.shape, dtype=o.dtype, pin_memory=True)
                h.copy_(o, non_blocking=True)
                copies.append((h, o))
            flying.append((name, r, want, copies, stage))
        else:
            bad += _differences(name, r, want)
    S.synchronize()
    ctx.wait()
    for name, d, want, copies, _stage in flying:
        bad += _differences(name, d.finish(), want)
        # What the consumer on S saw. include/mdhip.h: a device result is FINAL when the call has completed — "a rare
        # internal re-run may rewrite it at completion". Two entry points do so by design and say so: lag_msd through
        # its status word on the stream (the spectral path's bound: beyond 1e-10 the completion step answers from the
        # difference form; +inf: the transposition did not complete), the device-resident pair sums for frames that did
        # not run as one scalar-j pass (their host class histograms are added at completion, csrc/pair_hist.hip:
        # mdhip_rdf_atomic_dev). Everywhere else the copy queued behind the call must hold the final bytes.
        if name in REWRITTEN_AT_COMPLETION or not consume:
            continue
        if d.status is not None:
            status = float(copies[-1][0].numpy()[0])
            forced = "overlap" in D.DECK[name].tags  # (lag_variant 2: the spectral result stands whatever its bound)
            if np.isnan(status) or status > (np.finfo(np.float64).max if forced else LAG_BOUND_OK):
                continue
        for h, o in copies[:len(d.outs)]:
            if h.numpy().tobytes() != o.cpu().numpy().tobytes():
                bad.append("%s: the copy queued behind the call did not see its result" % name)
    assert ctx.pending() == 0
    assert late > 0
    return bad


def test_on_a_callers_stream(env, alone):
    torch = env.torch
    ctx = env.Context(0)
    try:
        S = torch.cuda.Stream()
        ctx.set_stream(S.cuda_stream)
        with torch.cuda.stream(S):
            bad = _late_sequence(env, ctx, S, D.ORDER, alone)
        ctx.set_stream(None)
        bad += run_sequence(env, ctx, D.ORDER[:5], alone)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_current_stream_is_not_the_contexts(env, alone):
    """The context launches on S, torch's current stream is another one (the default stream) and the inputs arrive
    late on THAT: the wrappers must wait for it themselves."""
    torch = env.torch
    ctx = env.Context(0)
    try:
        S = torch.cuda.Stream()
        ctx.set_stream(S.cuda_stream)
        names = [n for n in D.ORDER if D.DECK[n].device][:12] + ["lag_msd_small", "segment_com_small", "cn_loop_small"]
        bad = _late_sequence(env, ctx, torch.cuda.current_stream(), names, alone, consume=False)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_the_overlap_entry_forks_and_joins_on_this_device(env, alone):
    """lag_msd_overlap is planned with the CU-partitioned streams on the device the tests run on (tests/
    test_call_deck_cpu.py shows it for the limits of an MI355X): the residue-class path, at least three batches."""
    i = env.inputs["lag_msd_overlap"]
    ctx = env.Context(0)
    try:
        for k, v in D.OVERLAP.items():
            ctx.set_option(k, v)
        plan = env.B.lag_plan(i["xi"].shape[0], i["xi"].shape[2], i["max_lag"], i["go"], ctx=ctx)
    finally:
        ctx.close()
    assert plan["path"] == 3 and plan["n_batches"] >= 3, plan
    assert alone["lag_msd_overlap"].kernel == plan["kernel"]


# ---------------------------------------------------------------------------------------------- two contexts, turnover
def test_two_contexts_alternate_and_swap(env, alone):
    a, b = env.Context(0), env.Context(0)
    try:
        bad, flying = [], []
        for ctx, pair in ((a, "rdf_loop_async"), (b, "rdf_cn_loop_async")):  # in flight on both before either waits
            for name in (pair, "cumtrapz_small"):
                stage = D.InFlight(D.Stage(ctx, False))
                r = D.DECK[name].call(env.B, ctx, env.inputs[name], stage=stage)
                assert isinstance(r, D.Deferred)
                flying.append((name, r))
        assert a.pending() > 0 and b.pending() > 0
        for name, d in flying:
            bad += _differences(name, d.finish(), alone[name].bytes)
        for first, second in ((a, b), (b, a)):
            names = list(D.ORDER)
            bad += run_sequence(env, first, names[0::2], alone)
            bad += run_sequence(env, second, names[1::2], alone)
    finally:
        a.close()
        b.close()
    assert not bad, "\n".join(bad)


def test_context_turnover(env, alone):
    """Ten contexts, five entries each, closed; between them a 40 MB page-locked result is dropped and asked for again
    by the next context: the pool hands the same block out again."""
    from mdproptools_amd import _lib

    names = [n for n in D.ORDER if "in_flight" not in D.DECK[n].tags and n != "cumtrapz_two_launches"]
    big = "cumtrapz_two_launches"
    assert alone[big].result[0].nbytes >= _lib.PIN_RESULTS_FROM
    bad, blocks = [], []
    for k in range(10):
        ctx = env.Context(0)
        try:
            bad += run_sequence(env, ctx, [names[(5 * k + j) % len(names)] for j in range(5)], alone)
            r = D.DECK[big].call(env.B, ctx, env.inputs[big])
            bad += _differences(big, r, alone[big].bytes)
            blocks.append(r[0].ctypes.data)
            del r
            gc.collect()
        finally:
            ctx.close()
    assert len(set(blocks)) < len(blocks), "no page-locked block was handed out twice"
    assert not bad, "\n".join(bad)
