"""
Two pair-histogram calls on the device at once (ctx.h "Lanes"): consecutive asynchronous atom-atom
calls alternate between two compute streams, each with a workspace set of its own. Whatever is in flight beside a call,
and in whatever order the calls are waited for, every result is — bit for bit — what the C oracle counts
(oracle.cref.rdf_pairs / cn_pairs) and what the same call gives when it is made synchronously.

Shapes: the base shape is n = 300 (two tiles, the second partial), F = 9 (one XCD gets two frames), L = 30, r_cut = 12,
4 types, all 10 pairs; n = 2 000 grows the workspace. Frames of that size take the dense kernels, which complete inside
the entry point, so every scenario also runs at n = 2 100 in L = 40 with r_cut 9 (9 tiles, the last one partial: the
culled scalar-j sweep, whose host half is deferred — the calls that really are on the device together; the kernel name
is asserted). The overflow guard needs more wave items than the resident grid has waves before halving a batch can
help: the shape of test_overflow_guard_splits_the_batch (96 frames of 6 000 atoms, L = 42, r_cut 12), here 4 distinct
frames repeated 24 times (the oracle counts 4).
"""
import numpy as np
import pytest

from oracle import cref as C

pytestmark = pytest.mark.gpu

NB_SMALL, NB_BIG = 240, 90


class Case:
    """One data set with its oracle results (per frame) — computed once, never modified."""

    def __init__(self, synth, n, F, L, r_cut, ddr, nb, seed, cuboid=False):
        self.n, self.F, self.r_cut, self.ddr, self.nb = n, F, r_cut, ddr, nb
        self.x = synth.rdf_frames(n, range(F), L - 1.0 if cuboid else L, seed)  # (inside the shortest edge)
        rng = np.random.default_rng(seed)
        self.ty = rng.integers(1, 5, n).astype(np.int32) if cuboid else synth.rdf_types(n)
        self.box = np.tile(np.array([L, L - 1.0, L + 0.5]) if cuboid else np.full(3, float(L)), (F, 1))
        self.rel = np.array(synth.ALL_PAIRS_4)
        self.cuts = synth.cn_cutoffs(len(self.rel))
        self.full = np.empty((F, nb), np.uint64)
        self.part = np.empty((F, len(self.rel), nb), np.uint64)
        self.cn = np.empty((F, len(self.rel)), np.uint64)
        for f in range(F):
            self.full[f], self.part[f], _ = C.rdf_pairs(self.x[f], self.ty, self.rel, self.box[f], r_cut * r_cut, ddr, nb)
            self.cn[f] = C.cn_pairs(self.x[f], self.ty, self.rel, self.box[f], [c * c for c in self.cuts])
        for a in (self.x, self.ty, self.box, self.full, self.part, self.cn):
            a.setflags(write=False)
        self.dev = None

    def sub(self, F):
        """The first F frames as a case of their own (views)."""
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.F, c.x, c.box, c.full, c.part, c.cn = F, self.x[:F], self.box[:F], self.full[:F], self.part[:F], self.cn[:F]
        c.dev = None if self.dev is None else self.dev[:F]
        return c

    def want_rdf(self, per_frame):
        return (self.full, self.part) if per_frame else (self.full.sum(axis=0), self.part.sum(axis=0))

    def want_cn(self, per_frame):
        return self.cn if per_frame else self.cn.sum(axis=0)


@pytest.fixture(scope="module")
def env():
    import torch

    from mdproptools_amd import backend, synth
    from mdproptools_amd._lib import Context

    small = [Case(synth, 300, 9, 30.0 + k, 12.0, 0.05, NB_SMALL, 70 + k, cuboid=k > 0) for k in range(3)]
    grown = Case(synth, 2000, 9, 30.0, 12.0, 0.05, NB_SMALL, 75)
    big = [Case(synth, 2100, 9, 40.0 + k, 9.0, 0.1, NB_BIG, 80 + k, cuboid=k > 0) for k in range(3)]
    for c in small + [grown] + big:
        c.dev = torch.tensor(c.x, device="cuda")
    ctx = Context(0)
    yield backend, torch, ctx, small, grown, big
    ctx.close()


def rdf(B, ctx, c, per_frame=False, x=None, async_=True):
    return B.rdf_loop(c.dev if x is None else x, c.ty, c.box, c.rel, c.r_cut, c.ddr, c.nb, per_frame=per_frame, ctx=ctx,
                      async_=async_)


def cn(B, ctx, c, per_frame=False, async_=True):
    return B.cn_loop(c.dev, c.ty, c.box, c.rel, c.cuts, per_frame=per_frame, ctx=ctx, async_=async_)


def rdf_cn(B, ctx, c, per_frame=False, async_=True):
    return B.rdf_cn_loop(c.dev, c.ty, c.box, c.rel, c.r_cut, c.ddr, c.nb, c.cuts, per_frame=per_frame, ctx=ctx, async_=async_)


def check_rdf(got, c, per_frame, sync=None):
    full, part = c.want_rdf(per_frame)
    np.testing.assert_array_equal(got[0], full)
    np.testing.assert_array_equal(got[1], part)
    if sync is not None:
        np.testing.assert_array_equal(got[0], sync[0])
        np.testing.assert_array_equal(got[1], sync[1])
        assert got[2] == sync[2]


def sets(env):
    """(label, three cases, must the sweep be the deferred scalar-j kernel)"""
    _B, _torch, _ctx, small, _grown, big = env
    return (("base", small, False), ("culled", big, True))


@pytest.mark.parametrize("order", ["issue", "reverse"])
def test_three_different_calls_in_flight(env, order):
    B, _torch, ctx, *_ = env
    for label, cases, culled in sets(env):
        sync = [rdf(B, ctx, c, async_=False) for c in cases]
        hs = [rdf(B, ctx, c) for c in cases]
        if culled:
            assert ctx.pending() == 3, label
        seq = list(range(3)) if order == "issue" else [2, 1, 0]
        got = {k: hs[k].wait() for k in seq}
        assert ctx.pending() == 0
        for k, c in enumerate(cases):
            check_rdf(got[k], c, False, sync[k])
            if culled:
                assert "pair_hist_sj_kernel" in hs[k].stats()[3] and hs[k].stats()[2] == 1, label


def test_workspace_grows_under_a_live_call(env):
    B, _torch, ctx, small, grown, big = env
    from mdproptools_amd._lib import Context

    # n = 300 followed by n = 2 000, then the same with frames whose sweeps are deferred: a fresh context, so that every
    # buffer of the second and third call is allocated (first use of a lane) or re-allocated (the same lane again) while
    # the call before is in flight
    c2 = Context(0)
    try:
        pairs = [(small[0], grown), (big[0].sub(2), big[1])]
        for a, b in pairs:
            ha, hb = rdf(B, c2, a), rdf(B, c2, b)
            hc = rdf(B, c2, b, per_frame=True)  # the lane of `a` again, with larger buffers
            check_rdf(ha.wait(), a, False, rdf(B, ctx, a, async_=False))
            check_rdf(hb.wait(), b, False, rdf(B, ctx, b, async_=False))
            check_rdf(hc.wait(), b, True, rdf(B, ctx, b, per_frame=True, async_=False))
    finally:
        c2.close()


def test_one_and_nine_frames_alternate(env):
    B, _torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        seq = [cases[k % 3].sub(1) if k % 2 == 0 else cases[k % 3] for k in range(6)]
        sync = [rdf(B, ctx, c, async_=False) for c in seq]
        hs = [rdf(B, ctx, c) for c in seq]
        for h, c, r in zip(hs, seq, sync):
            check_rdf(h.wait(), c, False, r)


def test_frame_summed_and_per_frame_interleaved(env):
    B, _torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        plan = [(cases[k % 3], k % 2 == 1) for k in range(6)]
        sync = [rdf(B, ctx, c, per_frame=pf, async_=False) for c, pf in plan]
        hs = [rdf(B, ctx, c, per_frame=pf) for c, pf in plan]
        for h, (c, pf), r in zip(hs, plan, sync):
            check_rdf(h.wait(), c, pf, r)


def test_cn_and_one_sweep_between_two_rdf_calls(env):
    B, _torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        for pf in (False, True):
            sync_rdf = [rdf(B, ctx, cases[k], pf, async_=False) for k in (0, 1)]
            sync_cn = cn(B, ctx, cases[1], pf, async_=False)
            sync_both = rdf_cn(B, ctx, cases[2], pf, async_=False)
            h0 = rdf(B, ctx, cases[0], pf)
            h1 = cn(B, ctx, cases[1], pf)
            h2 = rdf_cn(B, ctx, cases[2], pf)
            h3 = rdf(B, ctx, cases[1], pf)
            got = [h.wait() for h in (h0, h1, h2, h3)]
            check_rdf(got[0], cases[0], pf, sync_rdf[0])
            np.testing.assert_array_equal(got[1], cases[1].want_cn(pf))
            np.testing.assert_array_equal(got[1], sync_cn)
            check_rdf(got[2][:3], cases[2], pf, sync_both[:3])
            np.testing.assert_array_equal(got[2][3], cases[2].want_cn(pf))
            check_rdf(got[3], cases[1], pf, sync_rdf[1])


def test_guard_split_with_another_call_in_flight(env):
    """A launch that raises the overflow guard is run again in halves from its completion step — on its own lane, while
    the call issued after it is still in flight on the other one (and the other way round)."""
    B, torch, ctx, _small, _grown, big = env
    from mdproptools_amd import synth
    from mdproptools_amd._lib import Context

    base, reps = Case(synth, 6000, 4, 42.0, 12.0, 0.05, NB_SMALL, 90), 24
    a = base.sub(4)
    a.F, a.x, a.box = 4 * reps, np.tile(base.x, (reps, 1, 1)), np.tile(base.box, (reps, 1))
    a.full, a.part = np.tile(base.full, (reps, 1)), np.tile(base.part, (reps, 1, 1))
    a.dev = torch.tensor(a.x, device="cuda")
    b = big[1]
    sync_a, sync_b = rdf(B, ctx, a, async_=False), rdf(B, ctx, b, async_=False)  # (no guard lowered on this context)
    c2 = Context(0)
    try:
        split = False
        for guard in (1024, 512, 256, 128, 64, 32):
            c2.set_option("rdf_guard", guard)
            try:
                h0 = rdf(B, c2, a)
                h1 = rdf(B, c2, b)
                h2 = rdf(B, c2, a)
                g0, g1, g2 = h0.wait(), h1.wait(), h2.wait()
            except Exception as e:  # a threshold even one frame exceeds: the clean error, delivered by a wait
                print("guard %d: %s" % (guard, e))
                assert "overflow the 32-bit" in str(e)
                break
            print("guard %d: launches %s" % (guard, [h.stats()[2] for h in (h0, h1, h2)]))
            check_rdf(g0, a, False, sync_a)
            check_rdf(g1, b, False, sync_b)
            check_rdf(g2, a, False, sync_a)
            if max(h.stats()[2] for h in (h0, h1, h2)) > 1:  # a re-run needed more than one launch
                split = True
                break
        assert split, "no threshold made a call re-run its batch"
    finally:
        c2.close()


def test_sync_and_non_pair_calls_behind_two_async_pair_calls(env):
    B, torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        h0, h1 = rdf(B, ctx, cases[0]), rdf(B, ctx, cases[1])
        s = rdf(B, ctx, cases[2], async_=False)  # completes everything before it, then itself
        assert ctx.pending() == 0
        check_rdf(s, cases[2], False)
        check_rdf(h0.wait(), cases[0], False)
        check_rdf(h1.wait(), cases[1], False)
        # a non-pair call: frame-pair displacement sums of the same coordinates
        h0, h1 = rdf(B, ctx, cases[0]), rdf(B, ctx, cases[1])
        c = cases[0]
        pairs = np.array([[0, c.F - 1], [1, 3]], dtype=np.int32)
        sums = B.msd_pairs(c.dev, pairs, [0, c.n], ctx=ctx)
        assert ctx.pending() == 0
        d = c.x[pairs[:, 1]] - c.x[pairs[:, 0]]  # [P, 3, n]
        want = np.concatenate([(d * d).sum(axis=2), (d * d).sum(axis=(1, 2))[:, None]], axis=1)
        np.testing.assert_allclose(np.asarray(sums).reshape(len(pairs), 4), want, rtol=1e-12)
        check_rdf(h0.wait(), cases[0], False)
        check_rdf(h1.wait(), cases[1], False)


def test_host_and_device_inputs_mixed(env):
    B, torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        pinned = torch.empty(cases[1].x.shape, dtype=torch.float64, pin_memory=True)
        pinned.numpy()[...] = cases[1].x
        pageable = np.array(cases[2].x)
        # device | pinned | pageable | device | pinned (its lane's staging buffer again) | pageable
        srcs = [(cases[0], None), (cases[1], pinned.numpy()), (cases[2], pageable), (cases[0], None),
                (cases[1], pinned.numpy()), (cases[2], pageable)]
        sync = {id(c): (rdf(B, ctx, c, async_=False), rdf(B, ctx, c, per_frame=True, async_=False)) for c in cases}
        hs = [rdf(B, ctx, c, x=x) for c, x in srcs]
        for h, (c, _x) in zip(hs, srcs):
            check_rdf(h.wait(), c, False, sync[id(c)][0])
        hs = [rdf(B, ctx, c, per_frame=True, x=x) for c, x in srcs[1:4]]
        for h, (c, _x) in zip(hs, srcs[1:4]):
            check_rdf(h.wait(), c, True, sync[id(c)][1])


def test_device_resident_sums_alternate(env):
    """The sums left in the caller's device buffers (derive_rdf_kernel adds into them): four calls in flight, each with
    a buffer of its own, on alternating lanes."""
    B, torch, ctx, *_ = env
    for _label, cases, _culled in sets(env):
        seq = [cases[k % 3] for k in range(4)]
        sync = [rdf(B, ctx, c, async_=False) for c in seq]
        words = (1 + len(seq[0].rel)) * seq[0].nb + 1
        outs = [torch.full((words,), -1, dtype=torch.int64, device="cuda") for _ in seq]
        hs = [B.rdf_loop_dev(c.dev, c.ty, c.box, c.rel, c.r_cut, c.ddr, c.nb, o, ctx=ctx, async_=True) for c, o in zip(seq, outs)]
        for h, c, r in zip(reversed(hs), reversed(seq), reversed(sync)):
            flat = h.wait().cpu().numpy().view(np.uint64)
            got = (flat[:c.nb], flat[c.nb:-1].reshape(len(c.rel), c.nb), int(flat[-1]))
            check_rdf(got, c, False, r)
