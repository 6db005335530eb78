"""
Host-resident pair input past one staging chunk, on every route it takes to the device (csrc/pair_hist.hip:
pair_hist_run / stage_batch_async / batch_parts and the asynchronous whole-trajectory copy of run_job;
csrc/mdhip_ctx.hip: mdhip_h2d_any, the page-locked ring of 2 halves x 4 chunks of 8 MiB filled by the four helper
threads of csrc/copy_pool.h), and the options no other test sets: h2d_overlap, h2d_ring, rdf_inflight, fft_logc.

A wrong event, offset or chunk reuse on these routes does not fault: it gives plausible histograms from stale or torn
frames. So every host-resident call here is
  - preceded by the same call on a DECOY trajectory of the same shape (another seed) on the same context: workspace,
    ring and staging buffers hold wrong data, and a skipped or late copy changes the result;
  - compared, per frame and frame-summed, bit for bit (integers, assert_array_equal) with the same call on a
    device-resident copy of the data, and with the C oracle (oracle.cref) on the first and last frame of every batch
    and on every frame whose bytes contain an 8 MiB chunk boundary of its batch's copy — at least 8 frames, all
    frames for n <= 1500. Batches and chunk boundaries are derived here from the shapes (batch_parts restated), and
    the number of batches is held against the launch count of the call and of mdhip_pair_plan.

The shapes are the smallest that reach each edge: a copy of exactly 3 chunks and one of 9 that cycles a half of the
ring twice (n = 8192, F = 512); a last chunk of 40 bytes, which leaves three of the four helpers without work, and three
batches alternating the two copy events (n = 1329, rdf_batch 263, F = 526); one batch below 32 frames, under and over a
chunk; atoms x sites with both copies of a batch in one half; six asynchronous calls whose whole trajectory (2 chunks
and a quarter) goes through the ring.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 1 << 23          # bytes per chunk of the ring (mdhip_h2d_any)
RING_CHUNKS = 4          # chunks per half (mdhip_ctx::H2D_RING_CHUNKS)
TILE = 256               # atoms per tile (pair_common.h)
MORTON_CELLS = 32768
R_CUT, BIN, NBINS = 9.0, 0.05, 180
_WORKERS = min(16, os.cpu_count() or 1)


# ---- the arithmetic of the staging code, restated ---------------------------------------------------------------------

def batch_parts(F, ni, staged, cu_count, rdf_batch=0):
    """pair_hist.hip batch_parts: [(first frame, frames)]."""
    nT = (ni + TILE - 1) // TILE
    per_frame_b = 54.0 * ni + 4.0 * MORTON_CELLS + 2.0 * nT * nT + 1024.0
    batch = min(max(int(2147483648.0 / per_frame_b), 1), 32768)
    if batch > cu_count > 0:
        batch = batch // cu_count * cu_count
    if rdf_batch > 0:
        batch = rdf_batch
    parts, f0 = [], 0
    if staged and F >= 32:
        b0 = min(max(8, (F // 4) // 8 * 8), batch)
        parts.append((0, b0))
        f0 = b0
    while f0 < F:
        parts.append((f0, min(batch, F - f0)))
        f0 += batch
    return parts


def chunks_of(n_bytes):
    """Bytes of every chunk of one copy through the ring."""
    return [min(CHUNK, n_bytes - o) for o in range(0, n_bytes, CHUNK)]


def boundary_frames(parts, frame_bytes):
    """Frames whose byte range holds a chunk boundary of the copy of their batch (a boundary between two frames: both)."""
    out = set()
    for f0, nf in parts:
        for b in range(CHUNK, nf * frame_bytes, CHUNK):
            out.add(f0 + b // frame_bytes)
            if b % frame_bytes == 0:
                out.add(f0 + b // frame_bytes - 1)
    return out


def oracle_frames(F, n, parts, frame_bytes):
    """The frames held against the C oracle: ends of every batch, chunk boundaries of every copy (`frame_bytes`: one
    entry per array copied), filled up to 8 with evenly spaced ones; every frame for n <= 1500."""
    if n <= 1500:
        return list(range(F))
    fr = set()
    for f0, nf in parts:
        fr.update((f0, f0 + nf - 1))
    for fb in frame_bytes:
        fr |= boundary_frames(parts, fb)
    for f in np.linspace(0, F - 1, 8).astype(int):
        if len(fr) >= min(8, F):
            break
        fr.add(int(f))
    return sorted(fr)


# ---- shapes, data, references ------------------------------------------------------------------------------------------

class Shape:
    """Atoms (and sites) of one case: positions of seed `seed`, the decoy's of seed + 1000."""

    def __init__(self, name, n, F, L, seed, m=0, rdf_batch=0):
        from mdproptools_amd import synth

        self.name, self.n, self.F, self.L, self.seed, self.m, self.rdf_batch = name, n, F, float(L), seed, m, rdf_batch
        self.types = synth.rdf_types(n)
        self.box = np.full((F, 3), self.L)
        if m:
            self.site_types = synth.rdf_types(m, 2)
            self.rel = np.array([(1, 1), (2, 2), (3, 1), (4, 2)], dtype=np.int32)
        else:
            self.rel = np.array(synth.ALL_PAIRS_4, dtype=np.int32)
        self.cuts = synth.cn_cutoffs(len(self.rel))
        self._data = {}

    def frames(self, decoy=False, sites=False):
        key = (decoy, sites)
        if key not in self._data:
            rng = np.random.default_rng([self.seed + (1000 if decoy else 0), int(sites)])
            self._data[key] = rng.random((self.F, 3, self.m if sites else self.n)) * self.L
            self._data[key].flags.writeable = False  # shared by the tests of this module: nobody changes it
        return self._data[key]

    def parts(self, staged, cu_count, rdf_batch=None):
        return batch_parts(self.F, self.n, staged, cu_count, self.rdf_batch if rdf_batch is None else rdf_batch)

    def plan_case(self, op, per_frame, dev=False):
        import pair_plan_cases as P

        plan_op = {"rdf": "rdf", "cn": "cn", "rdf_cn": "rdf_cn", "rdf_sites": "rdf_sites", "cn_sites": "cn_sites"}[op]
        return P._case(plan_op, self.F, self.n, self.L, self.types, self.rel, R_CUT, BIN, NBINS, cuts=self.cuts,
                       per_frame=per_frame, m=self.m, site_types=self.site_types if self.m else None, dev=dev)


def call(B, ctx, shape, op, x, per_frame, sites=None, async_=False):
    """The pair call `op` on coordinates `x` (host array or device tensor) -> its arrays as a tuple (or the handle)."""
    s = shape
    if op == "rdf":
        r = B.rdf_loop(x, s.types, s.box, s.rel, R_CUT, BIN, NBINS, per_frame=per_frame, ctx=ctx, async_=async_)
    elif op == "cn":
        r = B.cn_loop(x, s.types, s.box, s.rel, s.cuts, per_frame=per_frame, ctx=ctx, async_=async_)
    elif op == "rdf_cn":
        r = B.rdf_cn_loop(x, s.types, s.box, s.rel, R_CUT, BIN, NBINS, s.cuts, per_frame=per_frame, ctx=ctx, async_=async_)
    elif op == "rdf_sites":
        r = B.rdf_mol_loop(x, s.types, sites, s.site_types, s.box, s.rel, R_CUT, BIN, NBINS, per_frame=per_frame, ctx=ctx)
    else:
        r = B.cn_mol_loop(x, s.types, sites, s.site_types, s.box, s.rel, s.cuts, per_frame=per_frame, ctx=ctx)
    return r if async_ else as_arrays(r)


def as_arrays(r):
    """A call's result as a tuple of arrays (the overflow count, a Python int, as a one-element array)."""
    if isinstance(r, np.ndarray):
        return (r,)
    return tuple(np.array([v], dtype=np.uint64) if isinstance(v, int) else v for v in r)


def oracle_frame(shape, op, x_f, s_f=None):
    """One frame through the C oracle -> the arrays of `call` for that frame, None where the oracle has no per-frame
    figure to compare (the overflow count of a call is one number for all its frames)."""
    from oracle import cref as C

    s, Lv = shape, [shape.L] * 3
    rc2, cuts2 = R_CUT * R_CUT, [c * c for c in shape.cuts]
    if op in ("rdf", "rdf_cn"):
        full, part, _ = C.rdf_pairs(x_f, s.types, s.rel, Lv, rc2, BIN, NBINS)
        return (full, part, None) + ((C.cn_pairs(x_f, s.types, s.rel, Lv, cuts2),) if op == "rdf_cn" else ())
    if op == "cn":
        return (C.cn_pairs(x_f, s.types, s.rel, Lv, cuts2),)
    if op == "rdf_sites":
        part, _ = C.rdf_rect(x_f, s.types, s_f, s.site_types, s.rel, Lv, rc2, BIN, NBINS)
        return (part, None)
    return (C.cn_rect(x_f, s.types, s_f, s.site_types, s.rel, Lv, cuts2),)


class References:
    """Per (shape, op): the call on device-resident copies, per frame and frame-summed, and the oracle's frames. Made
    once (a context of its own) and shared by the tests; nothing changes them afterwards."""

    def __init__(self, B, torch):
        from mdproptools_amd._lib import Context

        self.B, self.torch, self.ctx, self.made = B, torch, Context(0), {}
        self.cu_count = torch.cuda.get_device_properties(0).multi_processor_count

    def close(self):
        self.ctx.close()

    def get(self, shape, op, frames):
        key = (shape.name, op)
        if key not in self.made:
            x = to_device(self.torch, shape.frames())
            st = to_device(self.torch, shape.frames(sites=True)) if shape.m else None
            dev = {pf: call(self.B, self.ctx, shape, op, x, pf, sites=st) for pf in (True, False)}
            del x, st
            for a in dev[True] + dev[False]:
                a.flags.writeable = False
            self.made[key] = dict(dev=dev, oracle={})
        ref = self.made[key]
        todo = [f for f in frames if f not in ref["oracle"]]
        if todo:
            xs, ss = shape.frames(), shape.frames(sites=True) if shape.m else None
            with ThreadPoolExecutor(_WORKERS) as pool:  # (the oracle's C calls release the interpreter lock)
                res = list(pool.map(lambda f: oracle_frame(shape, op, xs[f], None if ss is None else ss[f]), todo))
            ref["oracle"].update(zip(todo, res))
        return ref


def check(got_pf, got_sum, ref, frames, what):
    """A host-resident call's per-frame and frame-summed arrays against the device-resident call and the oracle."""
    dev_pf, dev_sum = ref["dev"][True], ref["dev"][False]
    assert len(got_pf) == len(dev_pf) and len(got_sum) == len(dev_sum)
    for k, (g, d) in enumerate(zip(got_pf, dev_pf)):
        np.testing.assert_array_equal(g, d, err_msg="%s: per frame, array %d, against device-resident input" % (what, k))
    for k, (g, d) in enumerate(zip(got_sum, dev_sum)):
        np.testing.assert_array_equal(g, d, err_msg="%s: frame-summed, array %d, against device-resident input" % (what, k))
    assert len(frames) >= min(8, len(got_pf[0]))
    for f in frames:
        for k, want in enumerate(ref["oracle"][f]):
            if want is not None:
                np.testing.assert_array_equal(got_pf[k][f], want, err_msg="%s: frame %d, array %d, against the oracle" % (what, f, k))
    if len(frames) == len(got_pf[0]):  # every frame went through the oracle: the sums too
        for k, want in enumerate(ref["oracle"][frames[0]]):
            if want is not None:
                total = np.sum([ref["oracle"][f][k] for f in frames], axis=0, dtype=np.uint64)
                np.testing.assert_array_equal(got_sum[k], total, err_msg="%s: frame sum, array %d, against the oracle" % (what, k))


@pytest.fixture(scope="module")
def env():
    import torch

    from mdproptools_amd import backend
    from oracle import cref

    cref.build()
    refs = References(backend, torch)
    yield backend, torch, refs
    refs.close()


_SHAPES = {}


def shape_of(name):
    """The cases of this module (positions are made on first use and shared)."""
    if name not in _SHAPES:
        _SHAPES[name] = {
            "ring_wrap": lambda: Shape("ring_wrap", 8192, 512, 60.0, 11),            # 3 chunks, then 9
            "tail_40": lambda: Shape("tail_40", 1329, 526, 26.0, 12, rdf_batch=263),  # one chunk + 40 bytes
            "short_6mb": lambda: Shape("short_6mb", 8192, 31, 60.0, 13),
            "short_9mb": lambda: Shape("short_9mb", 12000, 31, 68.0, 14),
            "sites": lambda: Shape("sites", 8192, 160, 60.0, 15, m=2731),
        }[name]()
    return _SHAPES[name]


def to_device(torch, x):
    return torch.from_numpy(np.array(x)).cuda()  # (a writable copy: torch does not take read-only arrays)


def pinned_copy(torch, x):
    t = torch.empty(x.shape, dtype=torch.float64, pin_memory=True)
    t.numpy()[...] = x
    return t.numpy()


def expect_launches(ctx, shape, op, per_frame, parts, x_on_host):
    """The launch count of the call just made = batches x passes per batch; mdhip_pair_plan, which counts the batches of
    batch_parts itself, says the same (it is told where the atoms are, not where the sites are: with the atoms on the
    device it plans unstaged batches, so its total is held against the call's only when the atoms are on the host)."""
    import pair_plan_cases as P

    plan = P.plan(shape.plan_case(op, per_frame, dev=not x_on_host), 0, 0, ctx=ctx)
    if plan["status"] == P.TWO_SWEEPS:  # RDF and CN as two sweeps (the dense kernels): the call reports the second one
        plan = P.plan(shape.plan_case("cn", per_frame, dev=not x_on_host), 0, 0, ctx=ctx)
    assert plan["status"] == 0 and plan["n_pass"] >= 1, plan
    assert ctx.last_kernel_ms()[1] == len(parts) * plan["n_pass"], (shape.name, op, ctx.last_kernel_ms(), parts, plan)
    if x_on_host:
        assert plan["launches"] == len(parts) * plan["n_pass"], (shape.name, op, plan, parts)
        assert ctx.last_kernel_name() == plan["kernel"], (ctx.last_kernel_name(), plan)


def run_host_case(B, refs, ctx, shape, op, x_host, what, staged=True, sites_host=None, sites_dev=None, x_dev=None):
    """Decoy call, then the call under test, per frame and frame-summed; both against the references. `x_host` /
    `sites_host`: the host-resident inputs (None: that input is the device tensor x_dev / sites_dev). `staged`: whether
    the call stages its host-resident frames batch by batch (h2d_overlap). Returns the batches."""
    parts = shape.parts(staged, refs.cu_count)
    fb = ([24 * shape.n] if x_host is not None else []) + ([24 * shape.m] if sites_host is not None else [])
    frames = oracle_frames(shape.F, shape.n, shape.parts(True, refs.cu_count), fb)
    ref = refs.get(shape, op, frames)
    got = {}
    for per_frame in (True, False):
        call(B, ctx, shape, op, shape.frames(decoy=True) if x_host is not None else x_dev, per_frame,
             sites=shape.frames(decoy=True, sites=True) if sites_host is not None else sites_dev)
        got[per_frame] = call(B, ctx, shape, op, x_host if x_host is not None else x_dev, per_frame,
                              sites=sites_host if sites_host is not None else sites_dev)
        expect_launches(ctx, shape, op, per_frame, parts, x_host is not None)
    check(got[True], got[False], ref, frames, what)
    return parts


# ---- 1. exact chunks and a ring wrap inside one copy -------------------------------------------------------------------

@pytest.mark.parametrize("op", ["rdf", "cn", "rdf_cn"])
def test_exact_chunks_and_a_ring_wrap_in_one_copy(env, op):
    """n = 8192, F = 512: batches (0, 128) and (128, 384); the first copy is exactly 3 chunks, the second 9 chunks: it
    cycles the 4 chunks of its half twice, so a chunk is refilled while an earlier DMA may still read it. The culled
    scalar-j sweep runs (32 tiles)."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    s = shape_of("ring_wrap")
    parts = s.parts(True, refs.cu_count)
    assert parts == [(0, 128), (128, 384)]
    sizes = [chunks_of(nf * 24 * s.n) for _, nf in parts]
    assert sizes[0] == [CHUNK] * 3 and sizes[1] == [CHUNK] * 9 and len(sizes[1]) > 2 * RING_CHUNKS
    ctx = Context(0)
    try:
        assert run_host_case(B, refs, ctx, s, op, s.frames(), "ring_wrap " + op) == parts
        assert "pair_hist_sj_kernel" in ctx.last_kernel_name(), ctx.last_kernel_name()
    finally:
        ctx.close()


# ---- 2. a 40-byte last chunk and more than two batches -----------------------------------------------------------------

@pytest.mark.parametrize("op", ["rdf", "cn", "rdf_cn"])
def test_a_40_byte_last_chunk_and_three_batches(env, op):
    """n = 1329, rdf_batch 263, F = 526: batches (0, 128), (128, 263), (391, 135) alternate the copy events 0, 1, 0; the
    middle copy is one chunk and 40 bytes, of which the first helper thread gets all and the other three nothing. The
    dense kernels run; every frame goes through the oracle."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    s = shape_of("tail_40")
    parts = s.parts(True, refs.cu_count)
    assert parts == [(0, 128), (128, 263), (391, 135)]
    assert chunks_of(263 * 24 * s.n) == [CHUNK, 40]
    per = ((40 + 3) // 4 + 63) & ~63  # CopyPool::copy: bytes per helper
    assert [min(40, per * (k + 1)) - min(40, per * k) for k in range(4)] == [40, 0, 0, 0]
    ctx = Context(0)
    try:
        ctx.set_option("rdf_batch", 263)
        assert run_host_case(B, refs, ctx, s, op, s.frames(), "tail_40 " + op) == parts
        assert "sj_kernel" not in ctx.last_kernel_name(), ctx.last_kernel_name()  # (fewer than 8 tiles: no culled sweep)
    finally:
        ctx.set_option("rdf_batch", 0)
        ctx.close()


# ---- 3. one batch, fewer than 32 frames --------------------------------------------------------------------------------

@pytest.mark.parametrize("name, n_chunks", [("short_6mb", 1), ("short_9mb", 2)])
def test_one_batch_below_32_frames(env, name, n_chunks):
    """F = 31: no shorter first batch; 8192 atoms stay under one chunk, 12 000 atoms take a chunk and a partial one."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    s = shape_of(name)
    parts = s.parts(True, refs.cu_count)
    assert parts == [(0, 31)] and len(chunks_of(31 * 24 * s.n)) == n_chunks
    ctx = Context(0)
    try:
        for op in ("rdf", "cn"):
            run_host_case(B, refs, ctx, s, op, s.frames(), "%s %s" % (name, op))
    finally:
        ctx.close()


# ---- 4. atoms x sites: both copies of a batch through one half ---------------------------------------------------------

@pytest.mark.parametrize("mix", ["both_host", "sites_host", "atoms_host"])
def test_atoms_and_sites_share_a_half_of_the_ring(env, mix):
    """8192 atoms x 2731 sites (65 544 bytes per frame: no multiple of 64), F = 160: batches (0, 40) and (40, 120); the
    atoms and the sites of a batch go through the same half one after the other, and the second batch's atoms (22.5 MiB)
    plus sites (7.5 MiB) take all four chunks of it. Three residency mixes."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    s = shape_of("sites")
    parts = s.parts(True, refs.cu_count)
    assert parts == [(0, 40), (40, 120)] and (24 * s.m) % 64 != 0
    # the second batch's atoms (3 chunks) and sites (1) take every chunk of its half, which the decoy call before it has
    # used as well: each chunk is written again behind the event of the copy that last read it
    assert len(chunks_of(120 * 24 * s.n)) + len(chunks_of(120 * 24 * s.m)) == RING_CHUNKS
    x_dev = to_device(torch, s.frames()) if mix == "sites_host" else None
    s_dev = to_device(torch, s.frames(sites=True)) if mix == "atoms_host" else None
    ctx = Context(0)
    try:
        for op in ("rdf_sites", "cn_sites"):
            run_host_case(B, refs, ctx, s, op, None if mix == "sites_host" else s.frames(), "sites %s %s" % (mix, op),
                          sites_host=None if mix == "atoms_host" else s.frames(sites=True), sites_dev=s_dev, x_dev=x_dev)
    finally:
        ctx.close()


# ---- 5. asynchronous calls: the whole trajectory through the ring ------------------------------------------------------

def test_async_calls_copy_whole_trajectories_through_the_ring(env):
    """n = 8192, F = 96: 18 MiB per call = 2 chunks and a quarter, copied whole into the staging buffer the call before
    does not use. Six calls on different data, page-locked and pageable sources in turn, four in flight, a synchronous
    call in the middle, waited for in reverse order — after the same sequence on six decoy trajectories."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    n, F, L = 8192, 96, 60.0
    assert chunks_of(F * 24 * n) == [CHUNK, CHUNK, CHUNK // 4]
    shapes = [Shape("async%d" % k, n, F, L, 50 + k) for k in range(6)]
    assert batch_parts(F, n, False, refs.cu_count) == [(0, F)]  # (an asynchronous call stages its frames whole)
    frames = oracle_frames(F, n, [(0, F)], [24 * n])
    assert len(frames) >= 8 and {0, F - 1, CHUNK // (24 * n), 2 * CHUNK // (24 * n)} <= set(frames)
    ref = [refs.get(s, "rdf", frames) for s in shapes]

    def sources(decoy):
        return [pinned_copy(torch, s.frames(decoy)) if k % 2 == 0 else s.frames(decoy) for k, s in enumerate(shapes)]

    ctx = Context(0)
    try:
        got = {}
        for per_frame in (True, False):
            for decoy in (True, False):
                hosts = sources(decoy)
                hs = [call(B, ctx, s, "rdf", x, per_frame, async_=True) for s, x in zip(shapes[:4], hosts[:4])]
                assert ctx.pending() == 4
                mid = call(B, ctx, shapes[4], "rdf", hosts[4], not per_frame)  # synchronous: drains what is in flight
                assert ctx.pending() == 0
                hs += [call(B, ctx, s, "rdf", x, per_frame, async_=True) for s, x in zip(shapes[4:], hosts[4:])]
                res = [None] * 6
                for k in reversed(range(6)):
                    res[k] = as_arrays(hs[k].wait())
                    assert "pair_hist_sj_kernel" in hs[k].stats()[3] and hs[k].stats()[2] == 1, hs[k].stats()
                if not decoy:
                    got[per_frame] = res
                    got[("mid", not per_frame)] = mid
        for k in range(6):
            check(got[True][k], got[False][k], ref[k], frames, "async call %d" % k)
        check(got[("mid", True)], got[("mid", False)], ref[4], frames, "the synchronous call in the middle")
    finally:
        ctx.close()


# ---- 6. sources and options ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ring_wrap", "tail_40"])
@pytest.mark.parametrize("overlap, ring", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_every_source_under_every_copy_option(env, name, overlap, ring):
    """h2d_overlap x h2d_ring on the shapes of tests 1 (RDF) and 2 (RDF, CN, RDF + CN), each with a pageable C-contiguous source, a page-locked
    one, a pageable view that starts one double into a larger buffer (8-byte but not 16-byte aligned) and a read-only
    array: the same arrays every time."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    s = shape_of(name)
    x = s.frames()
    assert not x.flags.writeable  # the read-only source

    def source(kind):
        if kind == "pageable":
            return x.copy()
        if kind == "page-locked":
            return pinned_copy(torch, x)
        if kind == "read-only":
            return x
        buf = np.empty(x.size + 1)
        assert buf.ctypes.data % 16 == 0  # (numpy aligns its buffers: the view starts 8 bytes past a 16-byte boundary)
        view = buf[1:].reshape(x.shape)
        view[...] = x
        assert view.ctypes.data % 16 == 8 and view.flags.c_contiguous
        return view

    ctx = Context(0)
    try:
        ctx.set_option("h2d_overlap", overlap)
        ctx.set_option("h2d_ring", ring)
        if s.rdf_batch:
            ctx.set_option("rdf_batch", s.rdf_batch)
        want = s.parts(bool(overlap), refs.cu_count)
        assert len(want) == ((3 if s.rdf_batch else 2) if overlap else (2 if s.rdf_batch else 1))
        for kind in ("pageable", "page-locked", "view", "read-only"):
            src = source(kind)
            for op in ("rdf",) if name == "ring_wrap" else ("rdf", "cn", "rdf_cn"):
                what = "%s %s %s overlap %d ring %d" % (name, op, kind, overlap, ring)
                assert run_host_case(B, refs, ctx, s, op, src, what, staged=bool(overlap)) == want
    finally:
        ctx.set_option("h2d_overlap", 1)
        ctx.set_option("h2d_ring", 1)
        ctx.set_option("rdf_batch", 0)
        ctx.close()


# ---- 7. rdf_inflight ----------------------------------------------------------------------------------------------------

def test_rdf_inflight_blocks_per_frame(env):
    """rdf_inflight sets the blocks per frame of the per-frame scalar-j launch (pair_hist.hip, launch of a pass): 1, 2,
    4, 16 and a value beyond any frame count, at frame counts around the 8 frames dealt to the XCDs. n = 2100 in a 40 A
    box, r_cut 9: the culled sweep. Every frame against the oracle, bit for bit."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    counts = (1, 7, 8, 9, 17, 65)
    s = Shape("inflight", 2100, max(counts), 40.0, 21)
    ref = refs.get(s, "rdf", list(range(s.F)))
    x = to_device(torch, s.frames())
    ctx = Context(0)
    try:
        for value in (1, 2, 4, 16, 10 ** 6):
            ctx.set_option("rdf_inflight", value)
            for F in counts:
                full, part, ov = B.rdf_loop(x[:F], s.types, s.box[:F], s.rel, R_CUT, BIN, NBINS, per_frame=True, ctx=ctx)
                assert "pair_hist_sj_kernel" in ctx.last_kernel_name(), ctx.last_kernel_name()
                for f in range(F):
                    np.testing.assert_array_equal(full[f], ref["oracle"][f][0], err_msg="rdf_inflight %d F %d frame %d" % (value, F, f))
                    np.testing.assert_array_equal(part[f], ref["oracle"][f][1], err_msg="rdf_inflight %d F %d frame %d" % (value, F, f))
    finally:
        ctx.set_option("rdf_inflight", 1)
        ctx.close()


# ---- 8. fft_logc --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 257, 4097, 70_000])
def test_fft_logc_tile_widths(env, n):
    """fft_logc is the tile width (log2 columns) of fft_pass_kernel, the radix-4 network (fft_pow2.hip, launch_pass):
    every value from below to above its range [0, 6] (clamped), with fft_net8 0 so that this network runs at every radix,
    crossed with the largest radix fft_logr 4, 6, 10. Cross- and autocorrelation of 3 series against numpy's FFT of the
    zero-padded series within 1e-13 |a| |b|: reference and bound of test_gpu_parity's test_xcorr_fft_all_pass_plans."""
    B, torch, refs = env
    from mdproptools_amd._lib import Context

    rng = np.random.default_rng(n)
    a = rng.standard_normal((3, n)) * np.array([1.0, 1e3, 1e-4])[:, None]
    b = rng.standard_normal((3, n)) + 0.5
    L = 2
    while L < 2 * n:
        L *= 2
    w = n - np.arange(n)

    def ref(x, y):
        return np.fft.irfft(np.fft.rfft(x, L) * np.conj(np.fft.rfft(y, L)), L)[..., :n]

    ref_ab, ref_aa = ref(a, b), ref(a, a)
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    ctx = Context(0)
    try:
        ctx.set_option("fft_net8", 0)
        for logr in (4, 6, 10):
            ctx.set_option("fft_logr", logr)
            for logc in (-1, 0, 1, 2, 3, 4, 5, 6, 9):
                ctx.set_option("fft_logc", logc)
                got = B.xcorr(a, b, method=B.XCORR_FFT, ctx=ctx)
                assert (np.abs(got * w - ref_ab).max(axis=1) <= 1e-13 * na * nb).all(), (n, logr, logc)
                auto = B.xcorr(a, method=B.XCORR_FFT, ctx=ctx)
                assert (np.abs(auto * w - ref_aa).max(axis=1) <= 1e-13 * na * na).all(), (n, logr, logc)
    finally:
        ctx.set_option("fft_logc", 3)
        ctx.set_option("fft_logr", 10)
        ctx.set_option("fft_net8", 1)
        ctx.close()
