"""
numpy-facing wrappers over the C-ABI, one per reference kernel (the drop-in seam).

Argument meaning follows the reference's private functions
(/root/reference/mdproptools/structural/rdf_cn.py:72-162,
dynamical/diffusion.py:207-238, dynamical/conductivity.py:97-114,216-232,
dynamical/viscosity.py:86-153); layouts are the SoA planes of include/mdhip.h.
Coordinates may be host ndarrays, CUDA/HIP torch tensors (float64, contiguous)
or `_lib.DevPtr` — device-resident inputs are used in place.

Everything here runs on the GPU through libmdhip.so; there is no CPU path.

`async_=True` (where offered) issues the call through its *_async entry point: the device work is queued on the
context's stream and a `_lib.Pending` handle comes back at once; `handle.wait()` completes the call (and every call
issued before it) and returns what the synchronous form returns. Calls issued back to back run back to back on the
GPU, with no host round trip in between.
"""

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Pending, as_input, default_context, ptr, result_array

XCORR_FFT = 0
XCORR_DIRECT = 1


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dev_out(out, shape, dtype="torch.float64", ctx=None):
    """Checks a device result buffer (`out=`): contiguous CUDA tensor of `shape` and `dtype` on the context's device;
    whatever torch still has queued on that tensor's stream (its allocation's fill, say) is waited for, since the
    context writes it from a stream of its own. Returns its address."""
    if not (getattr(out, "is_cuda", False) and out.is_contiguous() and str(out.dtype) == dtype
            and tuple(out.shape) == tuple(shape)):
        raise ValueError("out must be a contiguous %s CUDA tensor of shape %s" % (dtype, tuple(shape)))
    if ctx is not None:
        if out.device.index is not None and out.device.index != ctx.device:
            raise ValueError("out lives on cuda:%d but the mdhip context is bound to device %d"
                             % (out.device.index, ctx.device))
        import torch

        cur = torch.cuda.current_stream(out.device)
        if getattr(ctx, "_stream", None) != cur.cuda_stream:
            cur.synchronize()
    return C.c_void_p(out.data_ptr())


def _shape3(x, name):
    shp = tuple(x.shape)
    if len(shp) != 3 or shp[1] != 3:
        raise ValueError("%s must have shape [n_frames, 3, n]" % name)
    return shp


def _xyz_box(xyz, box, ctx):
    """What the calls on xyz [F,3,N] and box [F,3] open with: -> (the context, F, N, box float64 [F,3], coordinate
    pointer, on_device, keepalive)."""
    ctx = ctx or default_context()
    F, _, N = _shape3(xyz, "xyz")
    return (ctx, F, N, _f64(box).reshape(F, 3)) + as_input(xyz, ctx)


def _mol_of(mol_of, N):
    """mol_of [N] as the library reads it."""
    mol = _i32(mol_of).ravel()
    if len(mol) != N:
        raise ValueError("mol_of must hold one molecule index per atom")
    return mol


def _pair_inputs(xyz, types, box, relation_matrix, ctx, check_types=True):
    """What every atom-atom pair call marshals: (F, N, coordinate pointer, on_device, keepalive, types int32, their
    frame stride (0: one [N] row shared by the frames), box [F,3], relations int32 [R,2])."""
    F, _, N = _shape3(xyz, "xyz")
    xp, on_dev, keep = as_input(xyz, ctx)
    ty = _i32(types)
    stride = 0 if ty.ndim == 1 else N
    if check_types and ty.size != (N if stride == 0 else F * N):
        raise ValueError("types must have shape [N] or [F, N]")
    return F, N, xp, on_dev, keep, ty, stride, _f64(box).reshape(F, 3), _i32(relation_matrix).reshape(-1, 2)


def _dest(out, shape, ctx, dtype=np.float64, dev_dtype="torch.float64", pinned=False):
    """Where a call writes its result: (result, pointer, on_device flag) — a fresh host array of `shape` (zeroed, or
    from `result_array`: page-locked when large) without `out`, else `out`, a device tensor validated by _dev_out."""
    if out is not None:
        return out, _dev_out(out, shape, dev_dtype, ctx), 1
    res = result_array(shape, dtype, device=ctx.device) if pinned else np.zeros(shape, dtype=dtype)
    return res, ptr(res, np.ctypeslib.as_ctypes_type(dtype)), 0


def _group_jobs(F, E, box, group_off, jobs, cols, group_cols, bin_size, n_bins, max_bins, max_text):
    """What the histogram calls over jobs on contiguous entity groups check first: -> (box float64 [F,3] or None,
    group_off int64 [G+1], G, jobs int32 [J, width], n_bins). `cols` names a job's columns, the first `group_cols` of
    which are groups."""
    bx = None
    if box is not None:
        bx = _f64(box)
        if bx.shape != (F, 3):
            raise ValueError("box must have shape [n_frames, 3]")
    off = _i64(group_off)
    if off.ndim != 1 or off.size < 1 or off[0] < 0 or off[-1] > E or np.any(np.diff(off) < 0):
        raise ValueError("group_off must be ascending offsets [n_groups + 1] within [0, n_ent]")
    G = off.size - 1
    width = cols.count(",") + 1
    jb = np.asarray(jobs)
    if jb.size and (jb.ndim != 2 or jb.shape[1] != width):
        raise ValueError("jobs must have shape [n_jobs, %d]: %s" % (width, cols))
    jb = _i32(jb).reshape(-1, width)
    if len(jb) and (jb[:, :group_cols].min() < 0 or jb[:, :group_cols].max() >= G):
        raise ValueError("a job names a group outside [0, %d)" % G)
    n_bins = int(n_bins)
    if not 1 <= n_bins <= max_bins:
        raise ValueError("n_bins must be in [1, %s]" % max_text)
    if not (float(bin_size) > 0.0 and np.isfinite(bin_size)):
        raise ValueError("bin_size must be positive and finite")
    return bx, off, G, jb, n_bins


def _check_cols(cols, n, what):
    """A host destination of per-entity columns: float64 [4, n] whose rows are contiguous (they may be rows of a larger
    C-ordered block). Returns (its address, the row stride in doubles)."""
    if not (isinstance(cols, np.ndarray) and cols.dtype == np.float64 and cols.shape == (4, n)
            and (n == 0 or (cols.strides[1] == 8 and cols.strides[0] % 8 == 0 and cols.strides[0] >= 8 * n))):
        raise ValueError("cols must be a float64 array [4, %s] with contiguous rows" % what)
    return C.c_void_p(cols.ctypes.data), cols.strides[0] // 8


def cutoff_sq(r_cut):
    """r_cut**2 as the jitted reference evaluates it: one multiply (numba lowers `x ** 2` with a
    literal exponent to x*x; rdf_cn.py:66). CPython's float pow differs in ~0.1% of inputs."""
    r = float(r_cut)
    return r * r


def rdf_loop(xyz, types, box, relation_matrix, r_cut, ddr, nbins, per_frame=True, ctx=None, edges=None, async_=False):
    """
    `_rdf_loop` (rdf_cn.py:72-97) for every frame of xyz [F,3,N].

    Returns (rdf_full uint64 [F,nbins], rdf_part uint64 [F,R,nbins], overflow) — or the frame sums
    [nbins] / [R,nbins] when per_frame is False.
    """
    ctx = ctx or default_context()
    F, N, xp, on_dev, keep, ty, stride, bx, rel = _pair_inputs(xyz, types, box, relation_matrix, ctx)
    R = len(rel)
    lead = (F,) if per_frame else ()
    full = np.zeros(lead + (nbins,), dtype=np.uint64)
    part = np.zeros(lead + (R, nbins), dtype=np.uint64)
    ov = C.c_uint64(0)
    ed = None if edges is None else _f64(edges)
    fn = ctx.lib.mdhip_rdf_atomic_async if async_ else ctx.lib.mdhip_rdf_atomic
    ctx.check(fn(
        ctx.h, F, N, xp, on_dev, ptr(ty, C.c_int32), stride, ptr(bx), R, ptr(rel, C.c_int32),
        cutoff_sq(r_cut), float(ddr), int(nbins), None if ed is None else ptr(ed), int(bool(per_frame)),
        ptr(full, C.c_uint64), ptr(part, C.c_uint64), C.byref(ov)))
    if async_:
        return Pending(ctx, (full, part, ov), keep=(keep, ty, bx, rel, ed), finish=lambda r: (r[0], r[1], int(r[2].value)))
    return full, part, int(ov.value)


def rdf_loop_dev(xyz, types, box, relation_matrix, r_cut, ddr, nbins, out, ctx=None, async_=False):
    """
    Frame-summed `_rdf_loop` with the sums left on the device: `out` = contiguous int64 CUDA tensor of
    (1 + R) * nbins + 1 words (rdf_full | rdf_part | overflow; the bit patterns are the uint64 counts), overwritten.
    Used by the multi-GPU layer so that the all-reduce reads the buffer the kernels wrote.
    """
    ctx = ctx or default_context()
    F, N, xp, on_dev, keep, ty, stride, bx, rel = _pair_inputs(xyz, types, box, relation_matrix, ctx)
    words = (1 + len(rel)) * int(nbins) + 1
    if not (getattr(out, "is_cuda", False) and out.is_contiguous() and str(out.dtype) == "torch.int64"
            and out.numel() == words):
        raise ValueError("out must be a contiguous int64 CUDA tensor of %d words" % words)
    op = _dev_out(out, out.shape, "torch.int64", ctx)
    fn = ctx.lib.mdhip_rdf_atomic_dev_async if async_ else ctx.lib.mdhip_rdf_atomic_dev
    ctx.check(fn(
        ctx.h, F, N, xp, on_dev, ptr(ty, C.c_int32), stride, ptr(bx), len(rel), ptr(rel, C.c_int32),
        cutoff_sq(r_cut), float(ddr), int(nbins), None, op))
    if async_:
        return Pending(ctx, out, keep=(keep, ty, bx, rel))
    return out


def rdf_cn_loop(xyz, types, box, relation_matrix, r_cut, ddr, nbins, cn_cut_list, per_frame=True, ctx=None,
                async_=False):
    """
    `_rdf_loop` and `_cn_loop` (rdf_cn.py:72-119) from ONE sweep over the pairs: returns
    (rdf_full, rdf_part, overflow, cn) — the integers of rdf_loop(...) and cn_loop(..., cn_cut_list).
    """
    ctx = ctx or default_context()
    F, N, xp, on_dev, keep, ty, stride, bx, rel = _pair_inputs(xyz, types, box, relation_matrix, ctx)
    R = len(rel)
    rc2 = _f64([cutoff_sq(r) for r in cn_cut_list])
    if len(rc2) != R:
        raise ValueError("one coordination cutoff per relation is required")
    lead = (F,) if per_frame else ()
    full = np.zeros(lead + (nbins,), dtype=np.uint64)
    part = np.zeros(lead + (R, nbins), dtype=np.uint64)
    cn = np.zeros(lead + (R,), dtype=np.uint64)
    ov = C.c_uint64(0)
    fn = ctx.lib.mdhip_rdf_cn_atomic_async if async_ else ctx.lib.mdhip_rdf_cn_atomic
    ctx.check(fn(
        ctx.h, F, N, xp, on_dev, ptr(ty, C.c_int32), stride, ptr(bx), R, ptr(rel, C.c_int32),
        cutoff_sq(r_cut), float(ddr), int(nbins), None, ptr(rc2), int(bool(per_frame)),
        ptr(full, C.c_uint64), ptr(part, C.c_uint64), C.byref(ov), ptr(cn, C.c_uint64)))
    if async_:
        return Pending(ctx, (full, part, ov, cn), keep=(keep, ty, bx, rel, rc2),
                       finish=lambda r: (r[0], r[1], int(r[2].value), r[3]))
    return full, part, int(ov.value), cn


def cn_loop(xyz, types, box, relation_matrix, r_cut_list, per_frame=True, ctx=None, out=None, async_=False):
    """`_cn_loop` (rdf_cn.py:100-119): raw counts uint64 [F,R] (or [R]). `out` (frame-summed only): an int64 CUDA
    tensor [R] that receives the counts on the device (their bit patterns; the multi-GPU layer all-reduces it)."""
    ctx = ctx or default_context()
    # (the shape of `types` is not checked here, and the library cannot: it sees a pointer and a stride)
    F, N, xp, on_dev, keep, ty, stride, bx, rel = _pair_inputs(xyz, types, box, relation_matrix, ctx, check_types=False)
    rc2 = _f64([cutoff_sq(r) for r in r_cut_list])
    if len(rc2) != len(rel):
        raise ValueError("one cutoff per relation is required")
    if out is not None and per_frame:
        raise ValueError("a device result buffer holds the frame-summed counts: pass per_frame=False")
    per_frame = int(bool(per_frame))
    cn, op, dev = _dest(out, ((F,) if per_frame else ()) + (len(rel),), ctx, np.uint64, "torch.int64")
    args = (ctx.h, F, N, xp, on_dev, ptr(ty, C.c_int32), stride, ptr(bx), len(rel), ptr(rel, C.c_int32), ptr(rc2))
    if async_:
        ctx.check(ctx.lib.mdhip_cn_atomic_async(*args, per_frame, op, dev))
        return Pending(ctx, cn, keep=(keep, ty, bx, rel, rc2))
    if dev:
        ctx.check(ctx.lib.mdhip_cn_atomic_dev(*args, op))
    else:
        ctx.check(ctx.lib.mdhip_cn_atomic(*args, per_frame, op))
    return cn


def rdf_mol_loop(xyz, types, sites, site_types, box, relation_matrix, r_cut, ddr, nbins, per_frame=True,
                 ctx=None):
    """`_rdf_mol_loop` (rdf_cn.py:122-141): atoms [F,3,N] x sites [F,3,M] -> (rdf_part, overflow)."""
    ctx = ctx or default_context()
    F, _, N = _shape3(xyz, "xyz")
    F2, _, M = _shape3(sites, "sites")
    if F2 != F:
        raise ValueError("xyz and sites must have the same number of frames")
    xp, x_dev, k1 = as_input(xyz, ctx)
    sp, s_dev, k2 = as_input(sites, ctx)
    ty, st = _i32(types), _i32(site_types)
    bx = _f64(box).reshape(F, 3)
    rel = _i32(relation_matrix).reshape(-1, 2)
    part = np.zeros(((F,) if per_frame else ()) + (len(rel), nbins), dtype=np.uint64)
    ov = C.c_uint64(0)
    ctx.check(ctx.lib.mdhip_rdf_sites(
        ctx.h, F, N, xp, x_dev, ptr(ty, C.c_int32), M, sp, s_dev, ptr(st, C.c_int32), ptr(bx), len(rel),
        ptr(rel, C.c_int32), cutoff_sq(r_cut), float(ddr), int(nbins), None, int(bool(per_frame)),
        ptr(part, C.c_uint64), C.byref(ov)))
    return part, int(ov.value)


def cn_mol_loop(xyz, types, sites, site_types, box, relation_matrix, r_cut_list, per_frame=True, ctx=None):
    """`_cn_mol_loop` (rdf_cn.py:144-162)."""
    ctx = ctx or default_context()
    F, _, N = _shape3(xyz, "xyz")
    _, _, M = _shape3(sites, "sites")
    xp, x_dev, k1 = as_input(xyz, ctx)
    sp, s_dev, k2 = as_input(sites, ctx)
    ty, st = _i32(types), _i32(site_types)
    bx = _f64(box).reshape(F, 3)
    rel = _i32(relation_matrix).reshape(-1, 2)
    rc2 = _f64([cutoff_sq(r) for r in r_cut_list])
    cn = np.zeros(((F,) if per_frame else ()) + (len(rel),), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_cn_sites(
        ctx.h, F, N, xp, x_dev, ptr(ty, C.c_int32), M, sp, s_dev, ptr(st, C.c_int32), ptr(bx), len(rel),
        ptr(rel, C.c_int32), ptr(rc2), int(bool(per_frame)), ptr(cn, C.c_uint64)))
    return cn


def segment_com(attr, atom_mass, seg_off, atom_q=None, out=None, ctx=None, async_=False):
    """
    `calc_com` / `_define_mol_cols` arithmetic (com_mols.py:58-60, rdf_cn.py:233-238):
    attr [F,K,N] -> com [F,K,M], plus seg_mass [M] and seg_q [M] (None without atom_q).
    `out` may be a device tensor [F,K,M] to keep the result on the GPU.
    """
    ctx = ctx or default_context()
    shp = tuple(attr.shape)
    if len(shp) != 3:
        raise ValueError("attr must have shape [n_frames, n_attr, n_atoms]")
    F, K, N = shp
    ap, a_dev, keep = as_input(attr, ctx)
    m = _f64(atom_mass)
    off = _i64(seg_off)
    M = len(off) - 1
    q = None if atom_q is None else _f64(atom_q)
    seg_mass = np.zeros(M)
    seg_q = None if q is None else np.zeros(M)
    if out is None:
        res = result_array((F, K, M), device=ctx.device)
        op, o_dev = C.c_void_p(res.ctypes.data), 0
    else:
        res = out
        op, o_dev, _k = as_input(out, ctx)
    fn = ctx.lib.mdhip_segment_com_async if async_ else ctx.lib.mdhip_segment_com
    ctx.check(fn(
        ctx.h, F, N, K, ap, a_dev, ptr(m), None if q is None else ptr(q), M, ptr(off, C.c_int64), op,
        o_dev, ptr(seg_mass), None if seg_q is None else ptr(seg_q)))
    if async_:
        return Pending(ctx, (res, seg_mass, seg_q), keep=(keep, m, off, q))
    return res, seg_mass, seg_q


def msd_pairs(r, pairs, group_off, scale=1.0, per_entity=False, ctx=None, out=None):
    """
    Frame-pair displacement sums (diffusion.py:212-218): r [F,3,E], pairs [P,2] ->
    sums [P,G,4] (+ per-entity rows [P,E,4] when requested). `out`: a float64 CUDA tensor [P,G,4] that receives the
    sums on the device (no per-entity rows then).
    """
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, on_dev, keep = as_input(r, ctx)
    pr = _i32(pairs).reshape(-1, 2)
    go = _i64(group_off)
    G = len(go) - 1
    if out is not None:
        if per_entity:
            raise ValueError("per-entity rows are not available with a device result buffer")
        ctx.check(ctx.lib.mdhip_msd_pairs_dev(
            ctx.h, F, E, rp, on_dev, float(scale), len(pr), ptr(pr, C.c_int32), G, ptr(go, C.c_int64),
            _dev_out(out, (len(pr), G, 4))))
        return out
    sums = np.zeros((len(pr), G, 4))
    pe = np.zeros((len(pr), E, 4)) if per_entity else None
    ctx.check(ctx.lib.mdhip_msd_pairs(
        ctx.h, F, E, rp, on_dev, float(scale), len(pr), ptr(pr, C.c_int32), G, ptr(go, C.c_int64),
        ptr(sums), None if pe is None else C.c_void_p(pe.ctypes.data), 0))
    return (sums, pe) if per_entity else sums


def msd_origin(r, origin, group_off, scale=1.0, cols=None, out=None, ctx=None, async_=False):
    """
    Single-origin MSD of a FRAME SHARD (diffusion.py:212-218 with the frames dealt to one process per GPU): every
    frame of r [F,3,E] against `origin` [3,E] (host array or CUDA tensor — the time-0 frame, broadcast by its owner).
    Returns sums [F,G,4]: a host array, or `out` (float64 CUDA tensor [F,G,4]) when given. `cols`: the per-entity
    columns dx2, dy2, dz2, msd, each [F*E] — a host float64 array [4, F*E] with contiguous rows or a CUDA tensor.
    """
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, on_dev, keep = as_input(r, ctx)
    if tuple(origin.shape) != (3, E):
        raise ValueError("origin must have shape [3, n_ent]")
    op, o_dev, keep2 = as_input(origin, ctx)
    go = _i64(group_off)
    G = len(go) - 1
    if out is None:
        sums = np.zeros((F, G, 4))
        sp, s_dev = C.c_void_p(sums.ctypes.data), 0
    else:
        sums, sp, s_dev = out, _dev_out(out, (F, G, 4), ctx=ctx), 1
    cp, c_dev, stride = None, 0, 0
    if cols is not None:
        if getattr(cols, "is_cuda", False):
            cp, c_dev, stride = _dev_out(cols, (4, F * E), ctx=ctx), 1, F * E
        else:
            cp, stride = _check_cols(cols, F * E, "n_frames * n_ent")
            stride = stride if F * E else 0
    fn = ctx.lib.mdhip_msd_origin_async if async_ else ctx.lib.mdhip_msd_origin
    ctx.check(fn(ctx.h, F, E, rp, on_dev, op, o_dev, float(scale), G, ptr(go, C.c_int64), sp, s_dev, cp, stride, c_dev))
    if async_:
        return Pending(ctx, sums, keep=(keep, keep2, go, cols))
    return sums


def msd_pairs_cols(r, pairs, group_off, cols, scale=1.0, ctx=None):
    """
    `msd_pairs` with the per-entity values written as the four COLUMNS dx2, dy2, dz2, msd of `cols` — a host float64
    array [4, P*E] whose rows are contiguous (they may be rows of a larger C-ordered block: the block a DataFrame
    wraps without copying). Returns sums [P,G,4].
    """
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, on_dev, keep = as_input(r, ctx)
    pr = _i32(pairs).reshape(-1, 2)
    go = _i64(group_off)
    G = len(go) - 1
    cp, stride = _check_cols(cols, len(pr) * E, "n_pairs * n_ent")
    sums = np.zeros((len(pr), G, 4))
    ctx.check(ctx.lib.mdhip_msd_pairs_cols(
        ctx.h, F, E, rp, on_dev, float(scale), len(pr), ptr(pr, C.c_int32), G, ptr(go, C.c_int64),
        ptr(sums), cp, stride, 0))
    return sums


def msd_windows(r, tao, scale=1.0, ctx=None, out=None, async_=False):
    """Fixed-lag window sums per entity (diffusion.py:225-237): r [F,3,E] -> [E,4] (`out`: float64 CUDA tensor [E,4])."""
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, on_dev, keep = as_input(r, ctx)
    res, op, dev = _dest(out, (E, 4), ctx)
    args = (ctx.h, F, E, rp, on_dev, float(scale), int(tao), op)
    if async_:
        ctx.check(ctx.lib.mdhip_msd_windows_async(*args, dev))
        return Pending(ctx, res, keep=keep)
    ctx.check((ctx.lib.mdhip_msd_windows_dev if dev else ctx.lib.mdhip_msd_windows)(*args))
    return res


def lag_msd(r, max_lag, group_off, scale=1.0, ctx=None, out=None, async_=False, status_out=None):
    """Full lag average (superset): r [F,3,E] -> [max_lag+1, G, 4] (`out`: float64 CUDA tensor of that shape).
    `status_out` (asynchronous call with a device result only): a float64 CUDA tensor whose first element receives the
    call's status on the device, behind its kernels (mdhip_lag_msd_status_dev: the spectral path's error bound, +inf
    when its result will be rewritten at completion, 0 for the exact path)."""
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, on_dev, keep = as_input(r, ctx)
    go = _i64(group_off)
    G = len(go) - 1
    res, op, dev = _dest(out, (int(max_lag) + 1, G, 4), ctx)
    args = (ctx.h, F, E, rp, on_dev, float(scale), int(max_lag), G, ptr(go, C.c_int64), op)
    if async_:
        ctx.check(ctx.lib.mdhip_lag_msd_async(*args, dev))
        pend = Pending(ctx, res, keep=(keep, go, status_out))
        if dev and status_out is not None:
            ctx.check(ctx.lib.mdhip_lag_msd_status_dev(ctx.h, _dev_out(status_out, tuple(status_out.shape), ctx=ctx)))
        return pend
    ctx.check((ctx.lib.mdhip_lag_msd_dev if dev else ctx.lib.mdhip_lag_msd)(*args))
    ctx.note_fallbacks()
    return res


LAG_PLAN_INFO = ("status", "path", "gen", "m", "source", "Fc", "units", "inst_a", "inst_b", "n_items", "n_batches",
                 "launches", "L")


def lag_plan(F, E, max_lag, group_off, opts=None, ctx=None, cu_count=0, lds_bytes=0, aligned=True):
    """What `lag_msd` would run on its spectral path for this shape, decided without a device (mdhip_lag_plan) ->
    dict(kernel=<name last_kernel_name() reports>, **LAG_PLAN_INFO). `ctx`: a context whose options and device limits
    are read (None: a fresh context's); cu_count / lds_bytes > 0 and `opts` override them."""
    opts = dict(opts or {})
    go = _i64(group_off)
    keys = (C.c_char_p * max(1, len(opts)))(*[k.encode() for k in opts])
    vals = (C.c_int * max(1, len(opts)))(*[int(v) for v in opts.values()])
    text = C.create_string_buffer(256)
    info = np.zeros(len(LAG_PLAN_INFO), np.int32)
    rc = _lib.load().mdhip_lag_plan(None if ctx is None else ctx.h, int(F), int(E), int(max_lag), len(go) - 1, ptr(go, C.c_int64),
                               int(aligned), int(cu_count), int(lds_bytes), len(opts), keys, vals, text, len(text),
                               ptr(info, C.c_int32))
    if rc != 0:
        raise _lib.MdhipError(rc, "mdhip_lag_plan: unusable arguments")
    out = dict(zip(LAG_PLAN_INFO, (int(v) for v in info)))
    out["kernel"] = text.value.decode()
    return out


def charge_flux(vel, atom_mass, atom_q, seg_off, seg_type, n_types, vel_conv, charge_conv, ctx=None, out=None,
                async_=False):
    """`conductivity_loop` for every frame (_conductivity.py:11-35): vel [F,3,N] -> j [3,T,F] (`out`: float64 CUDA
    tensor of that shape)."""
    ctx = ctx or default_context()
    F, _, N = _shape3(vel, "vel")
    vp_, on_dev, keep = as_input(vel, ctx)
    m, q = _f64(atom_mass), _f64(atom_q)
    off = _i64(seg_off)
    st = _i32(seg_type)
    res, op, dev = _dest(out, (3, int(n_types), F), ctx)
    args = (ctx.h, F, N, vp_, on_dev, ptr(m), ptr(q), len(off) - 1, ptr(off, C.c_int64), ptr(st, C.c_int32),
            int(n_types), float(vel_conv), float(charge_conv), op)
    if async_:
        ctx.check(ctx.lib.mdhip_charge_flux_async(*args, dev))
        return Pending(ctx, res, keep=(keep, m, q, off, st))
    ctx.check((ctx.lib.mdhip_charge_flux_dev if dev else ctx.lib.mdhip_charge_flux)(*args))
    return res


def xcorr(a, b=None, method=XCORR_FFT, n_lags=None, ctx=None, lag_begin=0, out=None, async_=False):
    """
    c[p][k] = sum_t a_p[t+k] b_p[t] / (n-k) (conductivity.py:109-114, viscosity.py:103-115).
    a, b: [n] or [P,n]; b=None gives the autocorrelation. lag_begin > 0 (direct method): the lags
    lag_begin .. lag_begin + n_lags - 1 only. `out`: float64 CUDA tensor [P, n_lags] that receives the lags on the
    device (returned as it is).
    """
    ctx = ctx or default_context()
    single = len(a.shape) == 1
    ap, a_dev, k1 = as_input(a, ctx)
    k2 = None  # (the converted copies as_input hands the library must live until the call has completed)
    shp = tuple(a.shape)
    P, n = (1, shp[0]) if single else shp
    if b is None:
        bp, b_dev = ap, a_dev
    else:
        bp, b_dev, k2 = as_input(b, ctx)
        if b_dev != a_dev:
            raise ValueError("a and b must both be host arrays or both device tensors")
    n_lags = n - int(lag_begin) if n_lags is None else int(n_lags)
    res, op, dev = _dest(out, (P, n_lags), ctx, pinned=True)
    args = (ctx.h, n, P, ap, bp, a_dev, int(method), int(lag_begin), n_lags, op)
    if dev:
        fn = ctx.lib.mdhip_xcorr_lags_dev_async if async_ else ctx.lib.mdhip_xcorr_lags_dev
    elif async_:
        if lag_begin:
            raise ValueError("a lag range is asynchronous only with a device result buffer")
        fn, args = ctx.lib.mdhip_xcorr_async, args[:7] + args[8:]  # (this entry point takes no lag_begin)
    else:
        fn = ctx.lib.mdhip_xcorr_lags
    ctx.check(fn(*args))
    if single and not dev:
        res = res[0]
    return Pending(ctx, res, keep=(a, b, k1, k2)) if async_ else res


def cumtrapz(y, dx, leading_zero=False, ctx=None, out=None, async_=False):
    """Cumulative trapezoid (viscosity.py:151, conductivity.py:231): y [n] or [S,n] (`out`: float64 CUDA tensor
    [S, n-1 (+1)] that receives the integrals on the device)."""
    ctx = ctx or default_context()
    single = len(y.shape) == 1
    yp, on_dev, keep = as_input(y, ctx)
    shp = tuple(y.shape)
    S, n = (1, shp[0]) if single else shp
    m = n - 1 + (1 if leading_zero else 0)
    res, op, dev = _dest(out, (S, max(m, 0)), ctx, pinned=True)
    if dev:
        fn = ctx.lib.mdhip_cumtrapz_dev_async if async_ else ctx.lib.mdhip_cumtrapz_dev
    else:
        fn = ctx.lib.mdhip_cumtrapz_async if async_ else ctx.lib.mdhip_cumtrapz
    ctx.check(fn(ctx.h, n, S, yp, on_dev, float(dx), int(bool(leading_zero)), op))
    if single and not dev:
        res = res[0]
    return Pending(ctx, res, keep=keep) if async_ else res


def green_kubo(a, b=None, method=XCORR_FFT, acf_scale=1.0, dx=1.0, integral_scale=1.0, leading_zero=False,
               want_acf=True, want_mean=False, ctx=None, async_=False):
    """
    The Green-Kubo chain in ONE call, nothing but the results crossing the bus (mdhip_green_kubo):
      acf      = xcorr(a, b) * acf_scale                      viscosity.py:178-184, conductivity.py:109-114
      integral = integral_scale * cumtrapz(acf, dx)           viscosity.py:151-152, conductivity.py:229-231
      mean     = integral.mean(axis=0)                        viscosity.py:189
    a, b: [S, n] host arrays or CUDA tensors (b=None: autocorrelation). Returns (acf [S,n] or None, integral
    [S, n-1 (+1)], mean [n-1 (+1)] or None); large results are page-locked arrays (written by DMA).
    """
    ctx = ctx or default_context()
    ap, a_dev, k1 = as_input(a, ctx)
    S, n = tuple(a.shape)
    if b is None:
        bp, k2 = ap, None
    else:
        bp, b_dev, k2 = as_input(b, ctx)
        if b_dev != a_dev:
            raise ValueError("a and b must both be host arrays or both device tensors")
    m = n - 1 + (1 if leading_zero else 0)
    acf = result_array((S, n), device=ctx.device) if want_acf else None
    integral = result_array((S, max(m, 0)), device=ctx.device)
    mean = result_array((max(m, 0),), device=ctx.device) if want_mean else None
    fn = ctx.lib.mdhip_green_kubo_async if async_ else ctx.lib.mdhip_green_kubo
    ctx.check(fn(ctx.h, n, S, ap, bp, a_dev, int(method), float(acf_scale), float(dx), float(integral_scale),
                 int(bool(leading_zero)), None if acf is None else ptr(acf), ptr(integral),
                 None if mean is None else ptr(mean)))
    res = (acf, integral, mean)
    return Pending(ctx, res, keep=(k1, k2)) if async_ else res


bin_edges = _lib.bin_edges


def shell_residence(xyz_i, xyz_j, box, r_lo_sq, r_hi_sq, exclude_diagonal=False, ctx=None):
    """
    Numerators of the neighbour-shell autocovariance (residence_time.py:96-131): central atoms xyz_i [F,3,Ni],
    shell atoms xyz_j [F,3,Nj] -> (counts uint64 [F], number of in-shell records).
    counts[k] = sum_{i,j,t} h_ij(t) h_ij(t+k), h = (rsq > r_lo_sq) & (rsq <= r_hi_sq).
    """
    ctx = ctx or default_context()
    F, _, Ni = _shape3(xyz_i, "xyz_i")
    F2, _, Nj = _shape3(xyz_j, "xyz_j")
    if F2 != F:
        raise ValueError("xyz_i and xyz_j must have the same number of frames")
    ip, i_dev, k1 = as_input(xyz_i, ctx)
    jp, j_dev, k2 = as_input(xyz_j, ctx)
    bx = _f64(box).reshape(F, 3)
    counts = np.zeros(F, dtype=np.uint64)
    nrec = C.c_uint64(0)
    ctx.check(ctx.lib.mdhip_shell_residence(
        ctx.h, F, Ni, ip, i_dev, Nj, jp, j_dev, ptr(bx), float(r_lo_sq), float(r_hi_sq),
        int(bool(exclude_diagonal)), ptr(counts, C.c_uint64), C.byref(nrec)))
    return counts, int(nrec.value)


def _with_overflow_rerun(run, xyz, inp, bx, cap, pads, what, ctx, per_frame=None):
    """
    The capped per-row search behind shell_members and hydration_cosines. run(n_frames, pointer, on_device, box, cap)
    -> the per-row arrays [n_frames, C, cap], then count [n_frames, C] (exact even past cap); inp = as_input(xyz, ctx).
    Frames with a row that overflowed `cap` are run again, alone, with a cap of their largest count and spliced in; the
    other frames' rows are padded with `pads` (one value per per-row array). `what` = (function name, noun of a row)
    for the error texts. `per_frame` (optional, [n_frames, ...]): another per-frame input; run then takes it, or its
    re-run frames, as a sixth argument.
    """
    xp, x_dev, keep = inp
    cap = max(1, int(cap))
    more = () if per_frame is None else (per_frame,)
    *rows, count = run(len(bx), xp, x_dev, bx, cap, *more)
    over = np.flatnonzero((count > cap).any(axis=1))
    if len(over) == 0:
        return (*rows, count)
    big = int(count[over].max())
    if not x_dev:
        sub = np.ascontiguousarray(keep[over])
    elif hasattr(xyz, "index_select"):  # a torch tensor: the overflowing frames stay on the device
        import torch

        sub = xyz.index_select(0, torch.as_tensor(over, device=xyz.device)).contiguous()
    else:
        raise ValueError("%ss overflow cap=%d: pass a larger cap with a DevPtr input" % (what[1], cap))
    sp, s_dev, sub_keep = as_input(sub, ctx)  # (sub_keep: what sp points at, alive until the call below has returned)
    more = () if per_frame is None else (np.ascontiguousarray(per_frame[over]),)
    *rerun, rcount = run(len(over), sp, s_dev, np.ascontiguousarray(bx[over]), big, *more)
    del sub_keep
    if not np.array_equal(rcount, count[over]):
        raise RuntimeError("%s: the re-run found other %s sizes than the first sweep" % what)
    outs = []
    for first, again, pad in zip(rows, rerun, pads):
        out = np.full(first.shape[:2] + (big,), pad, dtype=first.dtype)
        out[:, :, :cap] = first
        out[over] = again
        outs.append(out)
    return (*outs, count)


def _with_larger_cap(run, count_of, cap, max_cap, cen, name, hint):
    """
    The capped whole-call search behind angle_hist and bond_order. run(cap) -> the call's result, count_of(result) its
    count [n_frames, C] (exact even past cap); cen [C] the centres' atoms. A call with a row of more than `cap`
    neighbours is run once more, whole, with a cap of the largest count (the first call's values are discarded); more
    than `max_cap`, what the row kernel stages, is a ValueError that names the frame and the centre atom. `name` and
    `hint` are the function's, for the error texts.
    """
    cap = int(cap)
    out = run(cap)
    count = count_of(out)
    big = int(count.max()) if count.size else 0
    if big > cap:
        if big > max_cap:
            f, c = np.unravel_index(int(count.argmax()), count.shape)
            raise ValueError("%s: frame %d, centre atom %d has %d neighbours; at most %d are supported (%s)"
                             % (name, f, int(cen[c]), big, max_cap, hint))
        out = run(big)
        if not np.array_equal(count_of(out), count):
            raise RuntimeError("%s: the re-run found other row sizes than the first sweep" % name)
    return out


SHELL_CAP = 32  # first-try molecules per (frame, centre) row of shell_members; rows that hold more are re-run


def shell_members(xyz, box, centres, mol_of, r_cut_sq, cap=SHELL_CAP, ctx=None):
    """
    Solvation shells of get_clusters (cluster_analysis.py:127-142): xyz [F,3,N] (atoms in id order), box [F,3],
    centre atom indices [C], mol_of [N] (contiguous molecules) -> (mols int32 [F,C,K], count int32 [F,C]).
    Row (f, c) of mols holds the count[f, c] molecules with an atom at rsq < r_cut_sq from centre c, ascending, then
    -1 up to K = max(cap, largest count). Frames whose shells overflow `cap` are run again with a cap of their
    largest count (include/mdhip.h: mdhip_shell_members).
    """
    ctx, F, N, bx, *inp = _xyz_box(xyz, box, ctx)
    cen = _i32(centres).ravel()
    mol = _mol_of(mol_of, N)
    C_ = len(cen)

    def run(n_f, p, dev, b, k):
        mols = np.empty((n_f, C_, k), dtype=np.int32)
        count = np.zeros((n_f, C_), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_shell_members(
            ctx.h, n_f, N, p, dev, ptr(b), C_, ptr(cen, C.c_int32), ptr(mol, C.c_int32), float(r_cut_sq), k,
            ptr(mols, C.c_int32), ptr(count, C.c_int32)))
        return mols, count

    return _with_overflow_rerun(run, xyz, inp, bx, cap, (-1,), ("shell_members", "shell"), ctx)


COORD_CLASSES = 8  # 8-bit counters in the 64-bit word of shell_coordination
COORD_NO_CLASS = 0xFF  # class of an atom that never counts
COORD_MOL_ATOMS = 255  # what one counter holds


def shell_coordination(xyz, box, centres, mol_of, seg_off, mol_type, cls, r_shell_sq, r_coord_sq, passes=None,
                       cap=SHELL_CAP, ctx=None):
    """
    The configuration census of get_unique_configurations (cluster_analysis.py:238-457) from the trajectory: xyz, box,
    centres, mol_of as shell_members, molecule m the atoms [seg_off[m], seg_off[m+1]) of type mol_type[m], cls uint8
    [N] the coordination class of every atom (0..7, or 255: never counted), passes [F,M] (None: all pass) the force
    filter's verdict -> (mols int32 [F,C,K], words uint64 [F,C,K], count int32 [F,C]).
    Row (f, c) holds the count[f, c] passing molecules other than the centre's own with an atom at rsq < r_shell_sq,
    each with a word of eight 8-bit counters: per class, its atoms at rsq < r_coord_sq. The entries are in ascending
    (type, word, molecule) order, then -1 / ~0 up to K = max(cap, largest count): equal configurations are equal
    (type, word) sequences. Frames whose rows overflow `cap` are run again with a cap of their largest count
    (include/mdhip.h: mdhip_shell_coordination).
    """
    ctx, F, N, bx, *inp = _xyz_box(xyz, box, ctx)
    cen = _i32(centres).ravel()
    mol = _i32(mol_of).ravel()
    off = _i64(seg_off).ravel()
    mty = _i32(mol_type).ravel()
    kls = np.ascontiguousarray(cls, dtype=np.uint8).ravel()
    M = len(off) - 1
    if len(mol) != N or len(kls) != N:
        raise ValueError("mol_of and cls must hold one value per atom")
    if len(mty) != M:
        raise ValueError("mol_type must hold one type per molecule of seg_off")
    used = kls[kls != COORD_NO_CLASS]
    if len(used) and int(used.max()) >= COORD_CLASSES:
        raise ValueError("at most %d coordination classes (class %d given)" % (COORD_CLASSES, int(used.max())))
    if M and int(np.diff(off).max()) > COORD_MOL_ATOMS:
        raise ValueError("a molecule of more than %d atoms: a coordination counter could wrap" % COORD_MOL_ATOMS)
    C_ = len(cen)
    mask = None
    if passes is not None:
        mask = np.ascontiguousarray(np.asarray(passes).reshape(F, M) != 0, dtype=np.uint8)

    def run(n_f, p, dev, b, k, sub=None):  # sub: the pass mask of the frames of this run
        mols = np.empty((n_f, C_, k), dtype=np.int32)
        words = np.empty((n_f, C_, k), dtype=np.uint64)
        count = np.zeros((n_f, C_), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_shell_coordination(
            ctx.h, n_f, N, p, dev, ptr(b), C_, ptr(cen, C.c_int32), M, ptr(mol, C.c_int32), ptr(off, C.c_int64),
            ptr(mty, C.c_int32), ptr(kls, C.c_uint8), None if sub is None else ptr(sub, C.c_uint8),
            float(r_shell_sq), float(r_coord_sq), k, ptr(mols, C.c_int32), ptr(words, C.c_uint64),
            ptr(count, C.c_int32)))
        return mols, words, count

    return _with_overflow_rerun(run, xyz, inp, bx, cap, (-1, np.uint64(0xFFFFFFFFFFFFFFFF)),
                                ("shell_coordination", "shell"), ctx, per_frame=mask)


def mol_kahan_sums(attr, seg_off, ctx=None):
    """
    Per-molecule sums of get_clusters' force filter (cluster_analysis.py:146-152): attr [F,K,N] -> [F,K,M], molecule m
    the atoms [seg_off[m], seg_off[m+1]), each value pandas' compensated groupby().sum() in ascending atom order.
    """
    ctx = ctx or default_context()
    if len(attr.shape) != 3:
        raise ValueError("attr must have shape [n_frames, n_attr, n_atoms]")
    F, K, N = tuple(attr.shape)
    off = _i64(seg_off).ravel()
    M = len(off) - 1
    ap, a_dev, keep = as_input(attr, ctx)
    out = np.zeros((F, K, M), dtype=np.float64)
    ctx.check(ctx.lib.mdhip_mol_kahan_sums(ctx.h, F, N, K, ap, a_dev, M, ptr(off, C.c_int64), ptr(out)))
    return out


HYDRATION_CAP = 16  # first-try waters per (frame, cation) row of hydration_cosines; rows that hold more are re-run


def hydration_cosines(xyz, box, cations, waters, r_cut_sq, cap=HYDRATION_CAP, ctx=None):
    """
    Cation-water cosines of get_hydration_number (hydration_number.py:13-99): xyz [F,3,N] (atoms in id order), box
    [F,3], cation atom indices [C], the first-atom (O) index of every water [W] (H1, H2 follow it) -> (idx int32
    [F,C,K], cos float64 [F,C,K], count int32 [F,C]). Row (f, c) holds the count[f, c] waters whose O is at
    rsq < r_cut_sq from cation c, ascending, and their cosines, then -1 / NaN up to K = max(cap, largest count).
    Frames whose rows overflow `cap` are run again with a cap of their largest count (include/mdhip.h:
    mdhip_hydration_cosines).
    """
    ctx, F, N, bx, *inp = _xyz_box(xyz, box, ctx)
    cat = _i32(cations).ravel()
    wat = _i32(waters).ravel()
    C_, W = len(cat), len(wat)

    def run(n_f, p, dev, b, k):
        idx = np.empty((n_f, C_, k), dtype=np.int32)
        cos = np.empty((n_f, C_, k), dtype=np.float64)
        count = np.zeros((n_f, C_), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_hydration_cosines(
            ctx.h, n_f, N, p, dev, ptr(b), C_, ptr(cat, C.c_int32), W, ptr(wat, C.c_int32), float(r_cut_sq), k,
            ptr(idx, C.c_int32), ptr(cos), ptr(count, C.c_int32)))
        return idx, cos, count

    return _with_overflow_rerun(run, xyz, inp, bx, cap, (-1, np.nan), ("hydration_cosines", "row"), ctx)


def hydration_counts(xyz, box, cations, waters, r_cut_sq, cos_cut, bin_width, n_bins, ctx=None):
    """
    The counts mode of the same search: -> (n_water int32 [F,C], n_away int32 [F,C], hist uint64 [n_bins]); n_away
    counts cos < cos_cut, hist bins trunc((cos + 1) / bin_width) clamped to n_bins - 1 over all rows, NaN in no bin
    (include/mdhip.h: mdhip_hydration_counts). No capacity limit.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    cat = _i32(cations).ravel()
    wat = _i32(waters).ravel()
    C_, W = len(cat), len(wat)
    n_water = np.zeros((F, C_), dtype=np.int32)
    n_away = np.zeros((F, C_), dtype=np.int32)
    hist = np.zeros(int(n_bins), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_hydration_counts(
        ctx.h, F, N, xp, x_dev, ptr(bx), C_, ptr(cat, C.c_int32), W, ptr(wat, C.c_int32), float(r_cut_sq),
        float(cos_cut), float(bin_width), int(n_bins), ptr(n_water, C.c_int32), ptr(n_away, C.c_int32),
        ptr(hist, C.c_uint64)))
    return n_water, n_away, hist


ANGLE_CAP = 64  # first-try neighbours per (frame, centre) row of angle_hist; a batch with a larger row is run again
ANGLE_MAX_CAP = 512  # what the angle kernel stages (include/mdhip.h: mdhip_angle_hist)
ANGLE_MAX_TRIPLETS = 8
ANGLE_MAX_CELLS = 4096  # n_triplets * n_bins


def angle_cos_edges(bin_size):
    """The cosine table of angle_hist: E[m] = cos(radians(m * bin_size)), m = 0 .. ceil(180 / bin_size) - 1; ValueError
    unless it is strictly decreasing (a bin_size so small that two edges round to one cosine)."""
    bin_size = float(bin_size)
    if not 0.0 < bin_size <= 180.0:
        raise ValueError("bin_size must be in (0, 180] degrees")
    n_bins = int(np.ceil(180.0 / bin_size))
    if not np.cos(np.radians(bin_size)) < 1.0:  # (the table is flattest at its ends: checked before it is built)
        raise ValueError("bin_size=%r: the cosine table is not strictly decreasing" % bin_size)
    if n_bins > ANGLE_MAX_CELLS:
        raise ValueError("bin_size=%r gives %d bins; at most %d" % (bin_size, n_bins, ANGLE_MAX_CELLS))
    edges = np.cos(np.radians(np.arange(n_bins) * bin_size))
    if not np.all(np.diff(edges) < 0):
        raise ValueError("bin_size=%r: the cosine table is not strictly decreasing" % bin_size)
    return edges


def angle_hist(xyz, box, types, triplets, r_cut_sq, cos_edges, mol_of=None, cap=ANGLE_CAP, ctx=None):
    """
    Bond-angle histograms (include/mdhip.h: mdhip_angle_hist): xyz [F,3,N], box [F,3], types [N] (the same in every
    frame), triplets [T] of (type_a, type_c, type_b), r_cut_sq [T,2] = (r_ca**2, r_cb**2), cos_edges [n_bins] from
    angle_cos_edges, mol_of [N] (None: no molecule exclusion) -> (hist uint64 [T,n_bins], n_degenerate uint64 [T],
    count int32 [F,C], centres int32 [C]). The centres are the atoms whose type is the type_c of a triplet, ascending;
    the candidates those whose type is a type_a or type_b. count[f, c] is the number of candidates within the largest
    cutoff of the centre's triplets. A batch with a row of more than `cap` neighbours is run once more with a cap of
    the largest count; more than 512 is a ValueError.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    typ = _i32(types).ravel()
    if len(typ) != N:
        raise ValueError("types must hold one type per atom")
    trip = _i32(triplets).reshape(-1, 3)
    T = len(trip)
    rc2 = _f64(r_cut_sq).reshape(-1, 2)
    if len(rc2) != T:
        raise ValueError("one (r_ca**2, r_cb**2) per triplet is required")
    edges = _f64(cos_edges).ravel()
    n_bins = len(edges)
    if n_bins < 1 or not np.all(np.diff(edges) < 0):
        raise ValueError("cos_edges must be strictly decreasing")
    mol = None if mol_of is None else _mol_of(mol_of, N)
    cen = np.flatnonzero(np.isin(typ, trip[:, 1])).astype(np.int32)
    cand = np.flatnonzero(np.isin(typ, np.concatenate([trip[:, 0], trip[:, 2]]))).astype(np.int32)
    cen_cls, cand_cls = np.ascontiguousarray(typ[cen]), np.ascontiguousarray(typ[cand])

    def run(k):
        hist = np.zeros((T, n_bins), dtype=np.uint64)
        degen = np.zeros(T, dtype=np.uint64)
        count = np.zeros((F, len(cen)), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_angle_hist(
            ctx.h, F, N, xp, x_dev, ptr(bx), len(cen), ptr(cen, C.c_int32), ptr(cen_cls, C.c_int32), len(cand),
            ptr(cand, C.c_int32), ptr(cand_cls, C.c_int32), None if mol is None else ptr(mol, C.c_int32), T,
            ptr(trip, C.c_int32), ptr(rc2), n_bins, ptr(edges), int(k), ptr(hist, C.c_uint64),
            ptr(degen, C.c_uint64), ptr(count, C.c_int32)))
        return hist, degen, count

    return (*_with_larger_cap(run, lambda out: out[2], cap, ANGLE_MAX_CAP, cen, "angle_hist", "smaller cutoffs?"), cen)


BOND_CAP = 64  # first-try neighbours per (frame, centre) row of bond_order; a batch with a larger row is run again
BOND_MAX_CAP = 512  # what the row kernel stages (include/mdhip.h: mdhip_bond_order)
BOND_MAX_DEGREES = 4
BOND_MAX_L = 12
# the bits of bond_order's flags
BOND_Q_SHORT, BOND_Q_DEGENERATE, BOND_TET_SHORT, BOND_TET_DEGENERATE, BOND_QBAR_SHORT = 1, 2, 4, 8, 16


def bond_order(xyz, box, types, centre_type, neighbour_types, r_cut_sq, degrees=(4, 6), n_nearest=None, averaged=False,
               tetrahedral=False, mol_of=None, cap=BOND_CAP, ctx=None):
    """
    Per-centre order parameters (include/mdhip.h: mdhip_bond_order): xyz [F,3,N], box [F,3], types [N] (the same in
    every frame), the centres the atoms of `centre_type`, the candidates those whose type is in `neighbour_types` (both
    ascending), degrees the l of q_l (distinct, 1..12, at most 4; may be empty with tetrahedral), n_nearest (None:
    every neighbour within the cutoff), mol_of [N] (None: no molecule exclusion) -> a dict:
      q float64 [F,C,D]; qbar float64 [F,C,D] (averaged, else None); tet float64 [F,C,2] = (q_tet, s_k) (tetrahedral,
      else None); flags int32 [F,C] (the BOND_* bits); count int32 [F,C]; centres int32 [C].
    NaN where a row is short or degenerate. A batch with a row of more than `cap` neighbours is run once more with a cap
    of the largest count; more than 512 is a ValueError.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    typ = _i32(types).ravel()
    if len(typ) != N:
        raise ValueError("types must hold one type per atom")
    deg = _i32(list(degrees)).ravel()
    D = len(deg)
    mol = None if mol_of is None else _mol_of(mol_of, N)
    cen = np.flatnonzero(typ == int(centre_type)).astype(np.int32)
    cand = np.flatnonzero(np.isin(typ, _i32(list(neighbour_types)).ravel())).astype(np.int32)
    C_ = len(cen)

    def run(k):
        q = np.full((F, C_, D), np.nan)
        qbar = np.full((F, C_, D), np.nan) if averaged else None
        tet = np.full((F, C_, 2), np.nan) if tetrahedral else None
        flags = np.zeros((F, C_), dtype=np.int32)
        count = np.zeros((F, C_), dtype=np.int32)
        ctx.check(ctx.lib.mdhip_bond_order(
            ctx.h, F, N, xp, x_dev, ptr(bx), C_, ptr(cen, C.c_int32), len(cand), ptr(cand, C.c_int32),
            None if mol is None else ptr(mol, C.c_int32), float(r_cut_sq), D, ptr(deg, C.c_int32),
            int(n_nearest or 0), int(bool(averaged)), int(bool(tetrahedral)), int(k), ptr(q),
            None if qbar is None else ptr(qbar), None if tet is None else ptr(tet), ptr(flags, C.c_int32),
            ptr(count, C.c_int32)))
        return {"q": q, "qbar": qbar, "tet": tet, "flags": flags, "count": count, "centres": cen}

    return _with_larger_cap(run, lambda out: out["count"], cap, BOND_MAX_CAP, cen, "bond_order", "a smaller cutoff?")


SDF_MAX_SPECIES = 8        # observed species per call of sdf_hist (include/mdhip.h: mdhip_sdf_hist)
SDF_MAX_GRID = 256         # cells per axis
SDF_MAX_CELLS = 1 << 25    # n_species * G**3


def sdf_grid(r_cut, bin_size):
    """G = ceil(2 * r_cut / bin_size): the cells per axis of sdf_hist's grid over [-r_cut, r_cut)."""
    r_cut, bin_size = float(r_cut), float(bin_size)
    if not (np.isfinite(r_cut) and np.isfinite(bin_size) and r_cut > 0.0 and bin_size > 0.0):
        raise ValueError("r_cut and bin_size must be positive and finite")
    return int(np.ceil(2.0 * r_cut / bin_size))


def body_frames(xyz, box, origin, x_atom, xy_atom, ctx=None):
    """
    The body-fixed frames of sdf_hist alone (include/mdhip.h: mdhip_body_frames): xyz [F,3,N] (numpy, or a torch device
    tensor), box [F,3], per molecule its origin, x-axis and xy-plane atom [M] each -> (e float64 [F,M,3,3] with rows
    e1, e2, e3, valid bool [F,M], n_degenerate_rows int). The rows of e where valid is False mean nothing.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    org, xa, xya = (_i32(v).ravel() for v in (origin, x_atom, xy_atom))
    M = len(org)
    if len(xa) != M or len(xya) != M:
        raise ValueError("origin, x_atom and xy_atom must hold one atom per molecule")
    rows = np.zeros((F, M, 10), dtype=np.float64)
    bad_rows = C.c_uint64(0)
    ctx.check(ctx.lib.mdhip_body_frames(ctx.h, F, N, xp, x_dev, ptr(bx), M, ptr(org, C.c_int32), ptr(xa, C.c_int32),
                                        ptr(xya, C.c_int32), ptr(rows), C.byref(bad_rows)))
    return rows[:, :, :9].reshape(F, M, 3, 3), rows[:, :, 9] != 0.0, int(bad_rows.value)


def sdf_hist(xyz, box, origin, x_atom, xy_atom, cand, cand_class, n_species, r_cut, bin_size, mol_of=None, ctx=None):
    """
    Spatial distribution histograms (include/mdhip.h: mdhip_sdf_hist): xyz [F,3,N] (numpy, or a torch device tensor),
    box [F,3], per reference molecule its origin, x-axis and xy-plane atom [M] each, the observed atoms cand [n_cand]
    with their species cand_class [n_cand] in [0, n_species), mol_of [N] (None: no molecule exclusion) -> (hist uint64
    [S,G,G,G] in the body frame (e1, e2, e3) with G = sdf_grid(r_cut, bin_size), n_degenerate uint64 [S]: the hits of
    rows without a frame, n_hits int32 [F,M], n_degenerate_rows int). No capacity limit.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    org, xa, xya = (_i32(v).ravel() for v in (origin, x_atom, xy_atom))
    M = len(org)
    if len(xa) != M or len(xya) != M:
        raise ValueError("origin, x_atom and xy_atom must hold one atom per reference molecule")
    cnd, cls = _i32(cand).ravel(), _i32(cand_class).ravel()
    if len(cls) != len(cnd):
        raise ValueError("cand_class must hold one species per candidate")
    S = int(n_species)
    G = sdf_grid(r_cut, bin_size)
    mol = None if mol_of is None else _mol_of(mol_of, N)
    ok = 1 <= S <= SDF_MAX_SPECIES and 1 <= G <= SDF_MAX_GRID and S * G ** 3 <= SDF_MAX_CELLS
    hist = result_array((S, G, G, G), np.uint64, device=ctx.device, zero=True) if ok else np.zeros(1, dtype=np.uint64)
    degen = np.zeros(max(S, 1), dtype=np.uint64)
    n_hits = np.zeros((F, M), dtype=np.int32)
    bad_rows = C.c_uint64(0)
    ctx.check(ctx.lib.mdhip_sdf_hist(
        ctx.h, F, N, xp, x_dev, ptr(bx), M, ptr(org, C.c_int32), ptr(xa, C.c_int32), ptr(xya, C.c_int32), len(cnd),
        ptr(cnd, C.c_int32), ptr(cls, C.c_int32), S, None if mol is None else ptr(mol, C.c_int32), float(r_cut),
        cutoff_sq(r_cut), float(bin_size), G, ptr(hist, C.c_uint64), ptr(degen, C.c_uint64), ptr(n_hits, C.c_int32),
        C.byref(bad_rows)))
    return hist, degen[:S], n_hits, int(bad_rows.value)


CONTACT_MAX_CLASSES = 16  # classes per side of contact_components (include/mdhip.h: mdhip_contact_components)


def contact_components(xyz, box, atoms_a, class_a, atoms_b, class_b, rsq_cut, node_of, n_nodes, ctx=None):
    """
    Connected components of the contact graph (include/mdhip.h: mdhip_contact_components): xyz [F,3,N] (numpy, or a
    torch device tensor), box [F,3], the atoms of list A [n_a] with their class [n_a], those of list B [n_b] with their
    class [n_b], rsq_cut [n_ca,n_cb] (squared cutoffs; <= 0: never links), node_of [N] (read for listed atoms only)
    -> (label int32 [F,n_nodes], n_components int32 [F], n_contacts uint64 [F]). label[f, m] is the smallest node of
    the component of m in frame f. No capacity: nothing in this call can overflow.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    aa, ca = _i32(atoms_a).ravel(), _i32(class_a).ravel()
    ab, cb = _i32(atoms_b).ravel(), _i32(class_b).ravel()
    if len(aa) != len(ca) or len(ab) != len(cb):
        raise ValueError("one class per listed atom is required")
    cut = _f64(rsq_cut)
    if cut.ndim != 2:
        raise ValueError("rsq_cut must be a [n_ca, n_cb] table")
    node = _i32(node_of).ravel()
    if len(node) != N:
        raise ValueError("node_of must hold one node index per atom")
    n_nodes = int(n_nodes)
    label = result_array((F, max(n_nodes, 0)), np.int32)
    n_comp = np.zeros(F, dtype=np.int32)
    n_con = np.zeros(F, dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_contact_components(
        ctx.h, F, N, xp, x_dev, ptr(bx), len(aa), ptr(aa, C.c_int32), ptr(ca, C.c_int32), len(ab),
        ptr(ab, C.c_int32), ptr(cb, C.c_int32), cut.shape[0], cut.shape[1], ptr(cut), n_nodes, ptr(node, C.c_int32),
        ptr(label, C.c_int32), ptr(n_comp, C.c_int32), ptr(n_con, C.c_uint64)))
    return label, n_comp, n_con


HBOND_MAX_CLASSES = 64  # n_dc * n_ac of hbond_counts (include/mdhip.h: mdhip_hbond_counts)
HBOND_MAX_CELLS = 4096  # n_dc * n_ac * n_bins
HBOND_MAX_FRAMES = 65535  # frames of one hbond_lifetime call


def _check_args(ctx, rc):
    """ctx.check, with the library's argument errors (MDHIP_EINVAL) as ValueError carrying its text."""
    try:
        ctx.check(rc)
    except _lib.MdhipError as e:
        if e.code == -1:
            raise ValueError(str(e)) from e
        raise


def _hbond_lists(N, donors, h_off, h_atoms, acceptors, mol_of):
    don, off, hat, acc = (_i32(donors).ravel(), _i32(h_off).ravel(), _i32(h_atoms).ravel(), _i32(acceptors).ravel())
    if len(off) != len(don) + 1:
        raise ValueError("h_off must hold one offset per donor and the end")
    return don, off, hat, acc, None if mol_of is None else _mol_of(mol_of, N)


def hbond_counts(xyz, box, donors, don_class, h_off, h_atoms, acceptors, acc_class, r_da_sq, cos_cut, r_ha_sq=0.0,
                 cos_edges=None, mol_of=None, n_dc=None, n_ac=None, ctx=None):
    """
    Hydrogen bonds per frame (include/mdhip.h: mdhip_hbond_counts): xyz [F,3,N] (numpy, or a torch device tensor), box
    [F,3], the donor atoms [n_don] with their class [n_don], their hydrogens in CSR form (h_off [n_don+1], h_atoms
    [n_h]), the acceptor atoms [n_acc] with their class [n_acc], the squared cutoffs (r_ha_sq <= 0: no H...A test),
    cos_cut = cos(angle_cut), cos_edges [n_bins] from angle_cos_edges (None: no histogram), mol_of [N] (None: no
    molecule exclusion), n_dc / n_ac (None: largest class + 1) -> (n_bonds int32 [F,n_dc,n_ac], n_donated uint64
    [n_don], n_accepted uint64 [n_acc], angle_hist uint64 [n_dc,n_ac,n_bins], n_degenerate int). angle_hist counts
    every (hydrogen, acceptor) that passes every test but the angle test. No capacity: nothing in this call can
    overflow.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    don, off, hat, acc, mol = _hbond_lists(N, donors, h_off, h_atoms, acceptors, mol_of)
    dcl, acl = _i32(don_class).ravel(), _i32(acc_class).ravel()
    if len(dcl) != len(don) or len(acl) != len(acc):
        raise ValueError("one class per donor and per acceptor is required")
    n_dc = int(n_dc) if n_dc is not None else (int(dcl.max()) + 1 if len(dcl) else 1)
    n_ac = int(n_ac) if n_ac is not None else (int(acl.max()) + 1 if len(acl) else 1)
    edges = np.zeros(0) if cos_edges is None else _f64(cos_edges).ravel()
    n_bins = len(edges)
    n_bonds = np.zeros((F, max(n_dc, 0), max(n_ac, 0)), dtype=np.int32)
    n_donated = np.zeros(len(don), dtype=np.uint64)
    n_accepted = np.zeros(len(acc), dtype=np.uint64)
    hist = np.zeros((max(n_dc, 0), max(n_ac, 0), n_bins), dtype=np.uint64)
    degen = C.c_uint64(0)
    _check_args(ctx, ctx.lib.mdhip_hbond_counts(
        ctx.h, F, N, xp, x_dev, ptr(bx), len(don), ptr(don, C.c_int32), ptr(dcl, C.c_int32), ptr(off, C.c_int32),
        len(hat), ptr(hat, C.c_int32), len(acc), ptr(acc, C.c_int32), ptr(acl, C.c_int32), n_dc, n_ac,
        None if mol is None else ptr(mol, C.c_int32), float(r_da_sq), float(r_ha_sq), float(cos_cut), n_bins,
        ptr(edges) if n_bins else None, ptr(n_bonds, C.c_int32), ptr(n_donated, C.c_uint64),
        ptr(n_accepted, C.c_uint64), ptr(hist, C.c_uint64) if n_bins else None, C.byref(degen)))
    return n_bonds, n_donated, n_accepted, hist, int(degen.value)


def hbond_lifetime(xyz, box, donors, h_off, h_atoms, acceptors, r_da_sq, cos_cut, r_ha_sq=0.0, mol_of=None,
                   max_lag=None, table_slots=0, ctx=None):
    """
    Hydrogen-bond time correlation numerators of a whole trajectory (include/mdhip.h: mdhip_hbond_lifetime): the
    inputs of hbond_counts without the classes, at most 65 535 frames, max_lag (None: F - 1) -> (c_int uint64
    [max_lag+1], c_cont uint64 [max_lag+1], n_pairs, n_records). With h(t) the bond indicator of a (hydrogen,
    acceptor) pair, c_int[k] = sum h(t) h(t+k) and c_cont[k] = the number of (pair, t) with h(t) = ... = h(t+k) = 1.
    table_slots > 0 forces the slot count of the first sweep's pair table (0: the library sizes it).
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    don, off, hat, acc, mol = _hbond_lists(N, donors, h_off, h_atoms, acceptors, mol_of)
    max_lag = max(F - 1, 0) if max_lag is None else int(max_lag)
    if max_lag < 0:
        raise ValueError("max_lag must not be negative")
    c_int = np.zeros(max_lag + 1, dtype=np.uint64)
    c_cont = np.zeros(max_lag + 1, dtype=np.uint64)
    n_pairs, n_rec = C.c_uint64(0), C.c_uint64(0)
    _check_args(ctx, ctx.lib.mdhip_hbond_lifetime(
        ctx.h, F, N, xp, x_dev, ptr(bx), len(don), ptr(don, C.c_int32), ptr(off, C.c_int32), len(hat),
        ptr(hat, C.c_int32), len(acc), ptr(acc, C.c_int32), None if mol is None else ptr(mol, C.c_int32),
        float(r_da_sq), float(r_ha_sq), float(cos_cut), max_lag, int(table_slots), ptr(c_int, C.c_uint64),
        ptr(c_cont, C.c_uint64), C.byref(n_pairs), C.byref(n_rec)))
    return c_int, c_cont, int(n_pairs.value), int(n_rec.value)


AP_REF_POS, AP_REF_NEG, AP_PROFILE = 0, 1, 2  # binning modes of axis_profile (include/mdhip.h: MDHIP_AP_*)
AP_SURFACE = 0x4000  # code bit: the atom belongs to the surface
AP_NONE = 0x3FFF     # row field of an atom that counts in no row


def axis_profile_codes(row, surface):
    """The 16-bit atom codes of axis_profile: `row` (integers, -1 = counts in no row) and `surface` (booleans), of one
    shape ([N] or [F,N])."""
    row = np.asarray(row, dtype=np.int64)
    if row.size and (row.min() < -1 or row.max() >= AP_NONE):
        raise ValueError("rows must be in [-1, %d)" % AP_NONE)
    code = np.where(row < 0, AP_NONE, row) | np.where(np.asarray(surface, dtype=bool), AP_SURFACE, 0)
    return np.ascontiguousarray(code, dtype=np.uint16)


def axis_profile(x, rows, mode, bin_size, dist, n_bins, n_rows, origin="lo", ctx=None):
    """
    Per-frame atom counts along one axis, measured from a surface (number_density.py:76-105; include/mdhip.h:
    mdhip_axis_profile): x [F,N] the axis coordinate (host array or contiguous float64 device tensor), rows the uint16 codes of
    axis_profile_codes, [N] shared by the frames or [F,N] -> (counts uint32 [F,n_rows,n_bins], extent float64 [F,2]
    (lo, hi of the surface atoms; NaN without any), outside uint32 [F]).
    mode AP_REF_POS / AP_REF_NEG: the reference's selection on `dist` (dist_from_interface) and its binning, negative
    bin indices wrapped; AP_PROFILE: s = x - origin ("lo", "hi" or a value per frame [F]), bins of bin_size from
    s = dist, nothing wraps. `outside` counts the selected atoms that have no bin.
    """
    ctx = ctx or default_context()
    shp = tuple(x.shape)
    if len(shp) != 2:
        raise ValueError("x must have shape [n_frames, n_atoms]")
    F, N = shp
    codes = np.ascontiguousarray(rows, dtype=np.uint16)
    if codes.shape not in ((N,), (F, N)):
        raise ValueError("rows must have shape [n_atoms] or [n_frames, n_atoms]")
    per_frame = codes.ndim == 2
    org, kind = None, 0
    if isinstance(origin, str):
        if origin not in ("lo", "hi"):
            raise ValueError('origin must be "lo", "hi" or a value per frame')
        kind = 1 if origin == "hi" else 0
    else:
        org, kind = _f64(np.broadcast_to(np.asarray(origin, dtype=np.float64), (F,))), 2
    xp, x_dev, keep = as_input(x, ctx)
    counts = result_array((F, int(n_rows), int(n_bins)), dtype=np.uint32, device=ctx.device)
    extent = np.empty((F, 2), dtype=np.float64)
    outside = np.empty(F, dtype=np.uint32)
    ctx.check(ctx.lib.mdhip_axis_profile(
        ctx.h, F, N, xp, x_dev, ptr(codes, C.c_uint16), int(per_frame), int(n_rows), int(mode), float(bin_size),
        float(dist), int(n_bins), kind, None if org is None else ptr(org), ptr(counts, C.c_uint32), ptr(extent),
        ptr(outside, C.c_uint32)))
    return counts, extent, outside


def displacement_hist(r, box, group_off, jobs, bin_size, n_bins, ctx=None):
    """
    Histogram of the distance travelled over a fixed lag, over all time origins (include/mdhip.h:
    mdhip_displacement_hist; the finished form of the reference's Displacement.calc_dist sketch, residence_time.py:
    211-254): r [F,3,E] (host array or contiguous float64 device tensor), box [F,3] edge lengths when r is wrapped (the
    kernel rebuilds the image counts) or None when it is unwrapped, group_off int64 [G+1] contiguous entity groups,
    jobs int32 [J,3] rows (group, lag, stride) -> (hist uint64 [J,n_bins], overflow uint64 [J], windows uint64 [J],
    moments float64 [J,3] = sums of r, r^2, r^4 over the job's windows, crossings int: the image shifts found).
    """
    F, _, E = _shape3(r, "r")
    bx, off, G, jb, n_bins = _group_jobs(F, E, box, group_off, jobs, "(group, lag, stride)", 1, bin_size, n_bins,
                                         1 << 20, "2^20")
    if len(jb):
        if jb[:, 1].min() < 1 or jb[:, 1].max() > F - 1:
            raise ValueError("every lag must be in [1, n_frames - 1 = %d]" % (F - 1))
        if jb[:, 2].min() < 1:
            raise ValueError("every stride must be at least 1")
    ctx = ctx or default_context()
    rp, r_dev, keep = as_input(r, ctx)
    J = len(jb)
    hist = result_array((J, n_bins), dtype=np.uint64, device=ctx.device)
    overflow = np.empty(J, dtype=np.uint64)
    windows = np.empty(J, dtype=np.uint64)
    moments = np.empty((J, 3), dtype=np.float64)
    crossings = C.c_uint64(0)
    ctx.check(ctx.lib.mdhip_displacement_hist(
        ctx.h, F, E, rp, r_dev, None if bx is None else ptr(bx), G, ptr(off, C.c_int64), J, ptr(jb, C.c_int32),
        float(bin_size), n_bins, None, ptr(hist, C.c_uint64), ptr(overflow, C.c_uint64), ptr(windows, C.c_uint64),
        ptr(moments), C.byref(crossings)))
    return hist, overflow, windows, moments, int(crossings.value)


def van_hove_distinct(r, box, group_off, jobs, bin_size, n_bins, ctx=None):
    """
    Pair histograms across a time lag, the distinct part of the van Hove function before normalisation (include/mdhip.h:
    mdhip_van_hove_distinct): r [F,3,E] WRAPPED coordinates (host array or contiguous float64 device tensor), box [F,3]
    edge lengths, group_off int64 [G+1] contiguous entity groups, jobs int32 [J,4] rows (group a, group b, lag, stride),
    lag 0 allowed -> (hist uint64 [J,n_bins], beyond uint64 [J], pairs uint64 [J]); hist.sum(1) + beyond == pairs.
    """
    F, _, E = _shape3(r, "r")
    if box is None:
        raise ValueError("box is required: the distinct van Hove function works on wrapped coordinates")
    bx, off, G, jb, n_bins = _group_jobs(F, E, box, group_off, jobs, "(group a, group b, lag, stride)", 2, bin_size,
                                         n_bins, 1 << 20, "2^20")
    if len(jb):
        if jb[:, 2].min() < 0 or jb[:, 2].max() > F - 1:
            raise ValueError("every lag must be in [0, n_frames - 1 = %d]" % (F - 1))
        if jb[:, 3].min() < 1:
            raise ValueError("every stride must be at least 1")
    ctx = ctx or default_context()
    rp, r_dev, keep = as_input(r, ctx)
    J = len(jb)
    hist = result_array((J, n_bins), dtype=np.uint64, device=ctx.device)
    beyond = np.empty(J, dtype=np.uint64)
    pairs = np.empty(J, dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_van_hove_distinct(
        ctx.h, F, E, rp, r_dev, ptr(bx), G, ptr(off, C.c_int64), J, ptr(jb, C.c_int32), float(bin_size), n_bins, None,
        ptr(hist, C.c_uint64), ptr(beyond, C.c_uint64), ptr(pairs, C.c_uint64)))
    return hist, beyond, pairs


RELAX_MAX_GROUPS = 16
RELAX_MAX_Q = 4
RELAX_MAX_FRAMES = (1 << 29) - 1
RELAX_GUARD = 1 << 30


def self_relaxation(r, box, group_off, max_lag, origin_stride=1, a=None, q=None, ctx=None):
    """
    Overlap counts and self-intermediate scattering sums at every lag 0 .. max_lag, per time origin (include/mdhip.h:
    mdhip_self_relaxation): r [F,3,E] (host array or contiguous float64 device tensor), box [F,3] edge lengths when r is
    wrapped (the kernel rebuilds the image counts) or None when it is unwrapped, group_off int64 [G+1] contiguous entity
    groups (G <= 16), origins 0, origin_stride, 2 origin_stride, ...; a: the overlap length, a float or one per group [G],
    or None for no overlap part; q: wave numbers [n_q] shared by the groups or [G,n_q], n_q <= 4, or None ->
    (origins uint64 [L], count1 uint64 [L,G] = sum over origins of n(t0, k), count2 uint64 [L,G] = the sum of n^2,
    fs int64 [L,G,n_q] = sum of rint(sinc(q |dr|) 2^32), nonfinite uint64 [L,G]), L = max_lag + 1. Without `a` the
    counts are zeros; without `q` fs is empty.
    """
    F, _, E = _shape3(r, "r")
    bx = None
    if box is not None:
        bx = _f64(box)
        if bx.shape != (F, 3):
            raise ValueError("box must have shape [n_frames, 3]")
    off = _i64(group_off)
    if off.ndim != 1 or off.size < 2 or off[0] < 0 or off[-1] > E or np.any(np.diff(off) < 0):
        raise ValueError("group_off must be ascending offsets [n_groups + 1] within [0, n_ent]")
    G = off.size - 1
    if G > RELAX_MAX_GROUPS:
        raise ValueError("at most %d groups per call (%d given)" % (RELAX_MAX_GROUPS, G))
    if not 1 <= F <= RELAX_MAX_FRAMES:
        raise ValueError("n_frames must be in [1, 2^29 - 1]")
    max_lag, stride = int(max_lag), int(origin_stride)
    if not 0 <= max_lag <= F - 1:
        raise ValueError("max_lag must be in [0, n_frames - 1 = %d]" % (F - 1))
    if stride < 1:
        raise ValueError("origin_stride must be at least 1")
    stride = min(stride, F)  # (beyond F - 1 every stride leaves the one origin 0; a Python int may not fit int64)
    if a is None and q is None:
        raise ValueError("at least one of a and q must be given")
    a_sq = None
    if a is not None:
        av = _f64(np.broadcast_to(_f64(a), (G,)) if np.ndim(a) == 0 else a)
        if av.shape != (G,):
            raise ValueError("a must be a number or hold one overlap length per group")
        if not np.all(av >= 0.0):
            raise ValueError("a must not be negative or NaN")
        a_sq = _f64(av * av)
    qv = np.zeros((G, 0))
    if q is not None:
        qv = _f64(q)
        if qv.ndim <= 1:
            qv = _f64(np.broadcast_to(qv.reshape(-1), (G, qv.size)))
        if qv.ndim != 2 or qv.shape[0] != G:
            raise ValueError("q must be wave numbers [n_q] or [n_groups, n_q]")
        if qv.shape[1] > RELAX_MAX_Q:
            raise ValueError("at most %d wave numbers per group (%d given)" % (RELAX_MAX_Q, qv.shape[1]))
        if not (np.all(qv >= 0.0) and np.all(np.isfinite(qv))):
            raise ValueError("q must be finite and not negative")
    n_q = qv.shape[1]
    if a_sq is None and n_q == 0:
        raise ValueError("at least one of a and q must be given")
    n_orig = (F - 1) // stride + 1
    sizes = np.diff(off)
    if G and n_orig * int(sizes.max()) >= RELAX_GUARD:
        raise ValueError("origins * group size = %d * %d reaches 2^30, beyond which the integer sums could overflow: "
                         "raise origin_stride" % (n_orig, int(sizes.max())))
    ctx = ctx or default_context()
    rp, r_dev, keep = as_input(r, ctx)
    L = max_lag + 1
    origins = np.empty(L, dtype=np.uint64)
    count1 = np.zeros((L, G), dtype=np.uint64)
    count2 = np.zeros((L, G), dtype=np.uint64)
    fs = np.zeros((L, G, n_q), dtype=np.int64)
    nonfinite = np.empty((L, G), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_self_relaxation(
        ctx.h, F, E, rp, r_dev, None if bx is None else ptr(bx), G, ptr(off, C.c_int64), max_lag, stride,
        None if a_sq is None else ptr(a_sq), n_q, ptr(qv) if n_q else None, ptr(origins, C.c_uint64),
        ptr(count1, C.c_uint64), ptr(count2, C.c_uint64), ptr(fs, C.c_int64) if n_q else None,
        ptr(nonfinite, C.c_uint64)))
    return origins, count1, count2, fs, nonfinite


def collective_displacement(r, weight, group_off, scale=1.0, out=None, weighted=None, ctx=None):
    """
    Charge-weighted collective displacement of every group per frame (include/mdhip.h: mdhip_collective_displacement):
    r [F,3,E] unwrapped coordinates (host array or contiguous float64 device tensor), weight [E], group_off int64 [G+1]
    contiguous groups -> P [G,3,F] with P[g,x,t] = sum_{e in g} weight[e] * scale * (r[t,x,e] - r[0,x,e]): a host array,
    or `out` (float64 CUDA tensor [G,3,F]) when given. `weighted`: a float64 CUDA tensor [F,3,E] that receives the
    per-entity terms, the input from which `lag_msd` yields the self part.
    """
    ctx = ctx or default_context()
    F, _, E = _shape3(r, "r")
    rp, r_dev, keep = as_input(r, ctx)
    w = _f64(weight)
    if w.shape != (E,):
        raise ValueError("weight must have shape [n_ent]")
    off = _i64(group_off)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("group_off must be offsets [n_groups + 1]")
    G = off.size - 1
    if out is None:
        res = np.empty((G, 3, F))
        op, o_dev = C.c_void_p(res.ctypes.data), 0
    else:
        res, op, o_dev = out, _dev_out(out, (G, 3, F), ctx=ctx), 1
    wp = None if weighted is None else _dev_out(weighted, (F, 3, E), ctx=ctx)
    ctx.check(ctx.lib.mdhip_collective_displacement(ctx.h, F, E, rp, r_dev, ptr(w), float(scale), G,
                                                    ptr(off, C.c_int64), op, o_dev, wp))
    return res


def cross_msd(P, max_lag, with_abs=False, out=None, abs_out=None, ctx=None):
    """
    Cross-displacement correlation of collective series at every lag (include/mdhip.h: mdhip_cross_msd): P [G,3,n]
    (host array or contiguous float64 device tensor) -> out [max_lag+1,G,G],
    out[k,a,b] = sum_t sum_x (P[a,x,t+k] - P[a,x,t]) (P[b,x,t+k] - P[b,x,t]) / (n - k). `with_abs`: also the same sum
    over the absolute terms (the scale of the rounding error); returns (out, abs) then. `out` / `abs_out`: float64 CUDA
    tensors of the result's shape that receive them on the device.
    """
    ctx = ctx or default_context()
    shp = tuple(P.shape)
    if len(shp) != 3 or shp[1] != 3:
        raise ValueError("P must have shape [n_groups, 3, n]")
    G, _, n = shp
    pp, p_dev, keep = as_input(P, ctx)
    L = int(max_lag) + 1
    if out is None and abs_out is not None:
        raise ValueError("abs_out on the device needs out on the device")
    if out is not None:
        op, ap = _dev_out(out, (L, G, G), ctx=ctx), None
        if abs_out is not None:
            ap = _dev_out(abs_out, (L, G, G), ctx=ctx)
        elif with_abs:
            raise ValueError("with_abs needs abs_out when out is a device tensor")
        ctx.check(ctx.lib.mdhip_cross_msd(ctx.h, n, G, pp, p_dev, int(max_lag), op, ap, 1))
        return (out, abs_out) if abs_out is not None else out
    res = np.empty((max(L, 0), G, G))
    ab = np.empty((max(L, 0), G, G)) if with_abs else None
    ctx.check(ctx.lib.mdhip_cross_msd(ctx.h, n, G, pp, p_dev, int(max_lag), C.c_void_p(res.ctypes.data),
                                      None if ab is None else C.c_void_p(ab.ctypes.data), 0))
    return (res, ab) if with_abs else res


ORIENT_MAX_GROUPS = 16


def _mol_jobs(x, box, job_atom0, job_mols, job_len, J, mismatch):
    """What the per-molecule series calls marshal alike: (F, A, box [F,3] or None, job_atom0 int64, job_mols int64,
    job_len int32, S = sum(job_mols)); `mismatch`: the ValueError text when the job arrays do not hold J entries."""
    F, _, A = _shape3(x, "x")
    bx = None if box is None else _f64(box)
    if bx is not None and bx.shape != (F, 3):
        raise ValueError("box must have shape [n_frames, 3]")
    a0, mols, length = _i64(job_atom0), _i64(job_mols), _i32(job_len)
    if not (a0.shape == mols.shape == length.shape == (J,)):
        raise ValueError(mismatch)
    return F, A, bx, a0, mols, length, int(mols.sum()) if J and mols.min() >= 0 else 0


def axis_vectors(x, box, job_atom0, job_mols, job_len, terms, out=None, ctx=None):
    """
    Molecule-fixed unit vectors per frame (include/mdhip.h: mdhip_axis_vectors): x [F,3,A] coordinates, atoms by id and
    molecules contiguous (host array or contiguous float64 device tensor); box [F,3] edge lengths, or None when x is
    unwrapped. Job j covers job_mols[j] molecules of job_len[j] atoms from atom job_atom0[j] on and has the terms
    terms[j] = [(k, w), ...], k the index of an atom inside the molecule (1 <= k < job_len[j], strictly ascending):
    v = sum_k w (x[a + k] - x[a]), each difference wrapped once when there is a box, u = v / |v|.
    Returns (U [S,3,F] with S = sum(job_mols), series job after job and molecule after molecule, degenerate uint64
    [n_jobs] = the zero vectors of every job): U is a host array, or `out` (float64 CUDA tensor [S,3,F]) when given.
    """
    ctx = ctx or default_context()
    J = len(terms)
    F, A, bx, a0, mols, length, S = _mol_jobs(x, box, job_atom0, job_mols, job_len, J,
                                              "job_atom0, job_mols, job_len and terms must hold one entry per job")
    t_off, t_atom, t_w = _term_lists(terms, J, "terms")
    xp, x_dev, keep = as_input(x, ctx)
    res, up, u_dev = _dest(out, (S, 3, F), ctx, pinned=True)
    degenerate = np.zeros(max(J, 1), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_axis_vectors(ctx.h, F, A, xp, x_dev, None if bx is None else ptr(bx), J,
                                         ptr(a0, C.c_int64), ptr(mols, C.c_int64), ptr(length, C.c_int32),
                                         ptr(t_off, C.c_int64), ptr(t_atom, C.c_int32), ptr(t_w), up, u_dev,
                                         ptr(degenerate, C.c_uint64)))
    return res, degenerate[:J]


def orient_corr(U, group_off, max_lag, out=None, ctx=None):
    """
    Orientational correlation sums at every lag (include/mdhip.h: mdhip_orient_corr): U [S,3,n] unit vectors, time-major
    (host array or contiguous float64 device tensor), group_off int64 [G+1] contiguous groups of series ->
    sums [max_lag+1,G,2]: sums[k,g,0] = sum over the series m of g and t < n - k of c = u_m(t) . u_m(t+k),
    sums[k,g,1] the same sum of c^2. C1 = S1 / W and C2 = 1.5 S2 / W - 0.5 with W = (n - k) * (size of g). A host array,
    or `out` (float64 CUDA tensor of that shape) when given.
    """
    ctx = ctx or default_context()
    shp = tuple(U.shape)
    if len(shp) != 3 or shp[1] != 3:
        raise ValueError("U must have shape [n_series, 3, n]")
    S, _, n = shp
    off = _i64(group_off)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("group_off must be offsets [n_groups + 1]")
    G = off.size - 1
    L = int(max_lag) + 1
    up, u_dev, keep = as_input(U, ctx)
    if out is None:
        res = np.empty((max(L, 0), G, 2))
        op, o_dev = C.c_void_p(res.ctypes.data), 0
    else:
        res, op, o_dev = out, _dev_out(out, (L, G, 2), ctx=ctx), 1
    ctx.check(ctx.lib.mdhip_orient_corr(ctx.h, n, S, up, u_dev, G, ptr(off, C.c_int64), int(max_lag), op, o_dev))
    return res


def _term_lists(terms, J, what):
    """(offsets int64 [J+1], atoms int32, weights float64) of J lists [(k, w), ...]."""
    if len(terms) != J:
        raise ValueError("%s must hold one list of (k, w) per job" % what)
    off = np.zeros(J + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in terms])
    return off, _i32([k for t in terms for k, _ in t]), _f64([w for t in terms for _, w in t])


def mol_moments(x, box, job_atom0, job_mols, job_len, site_terms, vec_terms, job_unit, site_out=None, vec_out=None,
                want_site=True, want_vec=True, totals=False, ctx=None):
    """
    Per-molecule sites and vectors, frame-major, and the per-frame totals of the vectors (include/mdhip.h:
    mdhip_mol_moments): x [F,3,A] coordinates, atoms by id and molecules contiguous (host array or contiguous float64
    device tensor); box [F,3] edge lengths, or None when x is unwrapped. Job j covers job_mols[j] molecules of
    job_len[j] atoms from atom job_atom0[j] on; site_terms[j] and vec_terms[j] are lists [(k, w), ...] (1 <= k <
    job_len[j], strictly ascending, possibly empty): site = x[a] + sum_k w (x[a + k] - x[a]), v = sum_k w (x[a + k] -
    x[a]), each difference wrapped once when there is a box; job_unit[j] = 1 normalises v.
    Returns a dict: "site", "vec" [F,3,S] with S = sum(job_mols) — host arrays, or `site_out` / `vec_out` (float64 CUDA
    tensors [F,3,S]; give both or neither), or None where want_site / want_vec is False —, "degenerate" uint64 [J], and
    with `totals` "total" [J,3,F] (the sum of the job's vectors per frame and axis) and "sq_total" [J,F] (the sum of
    their squared lengths).
    """
    ctx = ctx or default_context()
    J = len(job_unit)
    F, A, bx, a0, mols, length, S = _mol_jobs(x, box, job_atom0, job_mols, job_len, J,
                                              "job_atom0, job_mols, job_len and job_unit must hold one entry per job")
    s_off, s_atom, s_w = _term_lists(site_terms, J, "site_terms")
    v_off, v_atom, v_w = _term_lists(vec_terms, J, "vec_terms")
    unit = _i32(job_unit)
    given = [o is not None for o, want in ((site_out, want_site), (vec_out, want_vec)) if want]
    if any(given) and not all(given):
        raise ValueError("site_out and vec_out go together: both device tensors, or neither")
    on_dev = int(any(given))
    xp, x_dev, keep = as_input(x, ctx)
    site = vec = sp = vp_ = None
    if want_site:
        site, sp, _ = _dest(site_out, (F, 3, S), ctx, pinned=True)
    if want_vec:
        vec, vp_, _ = _dest(vec_out, (F, 3, S), ctx, pinned=True)
    total = np.empty((J, 3, F)) if totals else None
    sq_total = np.empty((J, F)) if totals else None
    degenerate = np.zeros(max(J, 1), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_mol_moments(
        ctx.h, F, A, xp, x_dev, None if bx is None else ptr(bx), J, ptr(a0, C.c_int64), ptr(mols, C.c_int64),
        ptr(length, C.c_int32), ptr(s_off, C.c_int64), ptr(s_atom, C.c_int32), ptr(s_w), ptr(v_off, C.c_int64),
        ptr(v_atom, C.c_int32), ptr(v_w), ptr(unit, C.c_int32), sp, vp_, on_dev,
        None if total is None else ptr(total), None if sq_total is None else ptr(sq_total), ptr(degenerate, C.c_uint64)))
    return {"site": site, "vec": vec, "degenerate": degenerate[:J], "total": total, "sq_total": sq_total}


VECTOR_PAIR_MAX_BINS = 4096  # bins per call of vector_pair_hist (include/mdhip.h: mdhip_vector_pair_hist)
VECTOR_PAIR_ONE = 1 << 32    # the fixed-point unit of its sums


def combine_words(words):
    """The signed Python integers behind 128-bit two's-complement words: uint64 [..., 2] (low, high) -> object array
    [...] of int."""
    w = np.asarray(words, dtype=np.uint64)
    if w.shape[-1:] != (2,):
        raise ValueError("words must have shape [..., 2]: (low, high)")
    flat = w.reshape(-1, 2)
    out = np.empty(len(flat), dtype=object)
    for n, (lo, hi) in enumerate(flat.tolist()):
        v = (hi << 64) | lo
        out[n] = v - (1 << 128) if hi >> 63 else v
    return out.reshape(w.shape[:-1])


def vector_pair_hist(site, vec, box, group_off, jobs, bin_size, n_bins, ctx=None):
    """
    Distance-resolved orientational pair sums (include/mdhip.h: mdhip_vector_pair_hist): site, vec [F,3,E] (both host
    arrays or both contiguous float64 device tensors, as mol_moments returns them), box [F,3] edge lengths, group_off
    int64 [G+1] contiguous entity groups, jobs int32 [J,2] rows (group a, group b) ->
    (hist uint64 [J,n_bins], sums object [J,3,n_bins] of Python int, beyond, unsummed, pairs uint64 [J]).
    sums[j, 0], [j, 1], [j, 2] are the exact sums of rint(2^32 c), rint(2^32 c^2), rint(2^32 e) over the pairs of a bin, c
    the cosine between the two vectors and e the cosine of vector j against the direction i -> j: divide by
    VECTOR_PAIR_ONE * hist. hist.sum(1) + beyond == pairs; unsummed pairs are inside hist and in no sum.
    """
    F, _, E = _shape3(site, "site")
    if tuple(vec.shape) != (F, 3, E):
        raise ValueError("vec must have the shape of site")
    if box is None:
        raise ValueError("box is required: the pair sums take the nearest image")
    bx, off, G, jb, n_bins = _group_jobs(F, E, box, group_off, jobs, "(group a, group b)", 2, bin_size, n_bins,
                                         VECTOR_PAIR_MAX_BINS, VECTOR_PAIR_MAX_BINS)
    ctx = ctx or default_context()
    sp, s_dev, keep_s = as_input(site, ctx)
    vp_, v_dev, keep_v = as_input(vec, ctx)
    if s_dev != v_dev:
        raise ValueError("site and vec must both be host arrays or both be device tensors")
    J = len(jb)
    hist = np.empty((J, n_bins), dtype=np.uint64)
    words = np.empty((J, 3, n_bins, 2), dtype=np.uint64)
    beyond, unsummed, pairs = (np.empty(J, dtype=np.uint64) for _ in range(3))
    ctx.check(ctx.lib.mdhip_vector_pair_hist(
        ctx.h, F, E, sp, vp_, s_dev, ptr(bx), G, ptr(off, C.c_int64), J, ptr(jb, C.c_int32), float(bin_size), n_bins,
        None, ptr(hist, C.c_uint64), ptr(words, C.c_uint64), ptr(beyond, C.c_uint64), ptr(unsummed, C.c_uint64),
        ptr(pairs, C.c_uint64)))
    return hist, combine_words(words), beyond, unsummed, pairs


DIHEDRAL_MAX_ROWS = 16    # histogram rows per call of dihedral_angles (include/mdhip.h: mdhip_dihedral_angles)
DIHEDRAL_MAX_BINS = 1440  # bins over [-180, 180): 0.25 degrees


def dihedral_cos_edges(n_bins):
    """cos(m * D), m = 0 .. n_bins/2 - 1, D = 360 / n_bins degrees: the bin table of dihedral_angles."""
    return np.cos(np.radians(np.arange(n_bins // 2) * (360.0 / n_bins)))


def dihedral_angles(x, box, job_atom0, job_mols, job_len, quads, job_row=None, n_bins=None, want_series=False, out=None,
                    ctx=None):
    """
    Dihedral angles i-j-k-l inside molecules (include/mdhip.h: mdhip_dihedral_angles): x [F,3,A] coordinates, atoms by id
    and molecules contiguous (host array or contiguous float64 device tensor); box [F,3] edge lengths, or None when x is
    unwrapped. Job j covers job_mols[j] molecules of job_len[j] atoms from atom job_atom0[j] on; quads[j] = (i, j, k, l),
    0-based atoms inside the molecule, all different; job_row[j] the histogram row it adds to (default: row j).
    n_bins (even, 2 .. 1440): histograms over [-180, 180) in bins of 360 / n_bins degrees, mirrored about 0 (the
    negative half is right-closed); None: no histogram. want_series (or `out`): the series U [S,3,F] = (cos phi,
    sin phi, 0), S = sum(job_mols), series job after job and molecule after molecule.
    Returns (hist uint64 [n_rows, n_bins] or None, U or None, degenerate uint64 [n_jobs] = the (molecule, frame) pairs
    of every job with three collinear atoms): U is a host array, or `out` (float64 CUDA tensor [S,3,F]) when given.
    """
    ctx = ctx or default_context()
    quad = _i32(quads)
    J = len(quad)
    mismatch = "job_atom0, job_mols and job_len must hold one entry, quads one (i, j, k, l), per job"
    F, A, bx, a0, mols, length, S = _mol_jobs(x, box, job_atom0, job_mols, job_len, J, mismatch)
    if quad.shape != (J, 4):
        raise ValueError(mismatch)
    want_series = bool(want_series) or out is not None
    if n_bins is None and not want_series:
        raise ValueError("nothing asked for: give n_bins for histograms, want_series or out for the series")
    if n_bins is None:
        rows, n_rows = np.zeros(J, dtype=np.int32), 1
    else:
        rows = _i32(np.arange(J) if job_row is None else job_row)
        if rows.shape != (J,):
            raise ValueError("job_row must hold one row per job")
        n_rows = int(rows.max()) + 1 if J else 1
    nb = 2 if n_bins is None else int(n_bins)
    edges = hist = None
    if n_bins is not None:
        edges = _f64(dihedral_cos_edges(nb))
        hist = np.zeros((max(n_rows, 0), max(nb, 0)), dtype=np.uint64)
    xp, x_dev, keep = as_input(x, ctx)
    res, up, u_dev = _dest(out, (S, 3, F), ctx, pinned=True) if want_series else (None, None, 0)
    degenerate = np.zeros(max(J, 1), dtype=np.uint64)
    ctx.check(ctx.lib.mdhip_dihedral_angles(ctx.h, F, A, xp, x_dev, None if bx is None else ptr(bx), J,
                                            ptr(a0, C.c_int64), ptr(mols, C.c_int64), ptr(length, C.c_int32),
                                            ptr(quad, C.c_int32), ptr(rows, C.c_int32), n_rows, nb,
                                            None if edges is None else ptr(edges),
                                            None if hist is None else ptr(hist, C.c_uint64), up, u_dev,
                                            ptr(degenerate, C.c_uint64)))
    return hist, res, degenerate[:J]


SHAPE_MAX_BINS = 4096    # bins of Rg and Ree per call of mol_shape (include/mdhip.h: mdhip_mol_shape)
SHAPE_MAX_KBINS = 1024   # bins of kappa^2 over [0, 1]
SHAPE_TOTALS = ("Rg2", "Rg", "Ree2", "l1", "l2", "l3", "k2", "I2", "Rg4")  # the rows of its totals
SHAPE_VALUES = ("Rg2", "Ree2", "k2", "l1", "l2", "l3")                    # the rows of its per-molecule values


def mol_shape(x, box, job_atom0, job_mols, job_len, weights, ends=None, unwrap=1, bin_size=0.05, n_bins=200, n_kbins=50,
              per_mol=False, out=None, totals=True, ctx=None):
    """
    Gyration tensors and chain size of molecules (include/mdhip.h: mdhip_mol_shape): x [F,3,A] coordinates, atoms by id
    and molecules contiguous (host array or contiguous float64 device tensor); box [F,3] edge lengths, or None when x is
    unwrapped. Job j covers job_mols[j] molecules of job_len[j] atoms from atom job_atom0[j] on; weights[j] the masses of
    one molecule's atoms [job_len[j]]; ends[j] = (e0, e1) the end atoms, 0-based inside the molecule (default: first and
    last). unwrap 1: positions follow the chain, every bond difference wrapped once; 0: every atom against the first.
    Histograms of Rg and Ree in n_bins bins of bin_size, of kappa^2 in n_kbins bins over [0, 1].
    Returns a dict: "hist_rg", "hist_ee" uint64 [J,n_bins], "hist_k" uint64 [J,n_kbins], "beyond" uint64 [J,2] (Rg, Ree
    without a bin), "degenerate" uint64 [J] (Rg == 0), "totals" [J,9,F] (rows SHAPE_TOTALS; None without `totals`) and
    "per_mol" [F,6,S] (rows SHAPE_VALUES, S = sum(job_mols)): a host array with `per_mol`, `out` (float64 CUDA tensor of
    that shape) when given, else None.
    """
    ctx = ctx or default_context()
    J = len(weights)
    F, A, bx, a0, mols, length, S = _mol_jobs(x, box, job_atom0, job_mols, job_len, J,
                                              "job_atom0, job_mols, job_len and weights must hold one entry per job")
    rows = [_f64(w).ravel() for w in weights]
    w_off = np.zeros(J + 1, dtype=np.int64)
    w_off[1:] = np.cumsum([len(r) for r in rows])
    w = _f64(np.concatenate(rows)) if rows else np.zeros(0)
    if ends is None:
        ends = [(0, max(int(n) - 1, 0)) for n in length]
    e = _i32(ends)
    if e.shape != (J, 2):
        raise ValueError("ends must hold one (e0, e1) per job")
    nb, nk = int(n_bins), int(n_kbins)
    hist_rg, hist_ee = (np.zeros((J, max(nb, 0)), dtype=np.uint64) for _ in range(2))
    hist_k = np.zeros((J, max(nk, 0)), dtype=np.uint64)
    beyond, degenerate = np.zeros((J, 2), dtype=np.uint64), np.zeros(max(J, 1), dtype=np.uint64)
    tot = np.empty((J, len(SHAPE_TOTALS), F)) if totals else None
    xp, x_dev, keep = as_input(x, ctx)
    res, pp, p_dev = _dest(out, (F, len(SHAPE_VALUES), S), ctx, pinned=True) if per_mol or out is not None else (None, None, 0)
    ctx.check(ctx.lib.mdhip_mol_shape(
        ctx.h, F, A, xp, x_dev, None if bx is None else ptr(bx), J, ptr(a0, C.c_int64), ptr(mols, C.c_int64),
        ptr(length, C.c_int32), ptr(w_off, C.c_int64), ptr(w), ptr(e, C.c_int32), int(unwrap), float(bin_size), nb, None, nk,
        ptr(hist_rg, C.c_uint64), ptr(hist_ee, C.c_uint64), ptr(hist_k, C.c_uint64), ptr(beyond, C.c_uint64),
        ptr(degenerate, C.c_uint64), None if tot is None else ptr(tot), pp, p_dev))
    return {"hist_rg": hist_rg, "hist_ee": hist_ee, "hist_k": hist_k, "beyond": beyond, "degenerate": degenerate[:J],
            "totals": tot, "per_mol": res}


VELOCITY_MAX_GROUPS = 16


def spectrum_length(n_frames):
    """The default padded transform length of velocity_spectrum: the smallest power of two >= 2 * n_frames (at least 4)."""
    L = 4
    while L < 2 * int(n_frames):
        L *= 2
    return L


def velocity_spectrum(v, ent_group, max_lag, L=None, coef=None, want_power=False, out=None, ctx=None):
    """
    Per-group lag sums and power spectra of velocity series (include/mdhip.h: mdhip_velocity_spectrum): v [F,3,E], frames
    in time order (host array or contiguous float64 device tensor); ent_group int32 [E], the group of every entity in
    -1 .. G-1 (-1: in no group; G = max + 1, at least 1; groups may be interleaved); coef [E] or None: the series are
    coef[e] * v[t,a,e]. L: the padded transform length, a power of two >= F + max_lag (default: the smallest >= 2 F).
    Returns (sums [max_lag+1,G,4], power [G,4,L/2+1] or None without `want_power`, a0 [G,4]): sums[k,g,a] = sum over the
    entities of g and t < F - k of s(t) s(t+k), power the unnormalised |DFT_L|^2 summed over the entities, a0 the sum of
    the squares (the scale of the documented error bounds); column 3 is the total over the axes. sums and power are host
    arrays, or `out` = (sums, power or None), float64 CUDA tensors of those shapes, when given; a0 is a host array.
    """
    ctx = ctx or default_context()
    F, _, E = _shape3(v, "v")
    grp = _i32(ent_group).ravel()
    if len(grp) != E:
        raise ValueError("ent_group must hold one group per entity")
    G = max(int(grp.max()) + 1, 1) if E else 1
    c = None
    if coef is not None:
        c = _f64(coef).ravel()
        if len(c) != E:
            raise ValueError("coef must hold one factor per entity")
    L = spectrum_length(F) if L is None else int(L)
    n_lags = max(int(max_lag) + 1, 0)
    vp, v_dev, keep = as_input(v, ctx)
    a0 = np.zeros((G, 4))
    if out is None:
        sums = np.empty((n_lags, G, 4))
        power = np.empty((G, 4, L // 2 + 1)) if want_power else None
        sp, pp, o_dev = C.c_void_p(sums.ctypes.data), None if power is None else C.c_void_p(power.ctypes.data), 0
    else:
        sums, power = out if isinstance(out, (tuple, list)) else (out, None)
        if want_power and power is None:
            raise ValueError("want_power with device results needs out = (sums, power)")
        sp, o_dev = _dev_out(sums, (n_lags, G, 4), ctx=ctx), 1
        pp = None if power is None else _dev_out(power, (G, 4, L // 2 + 1), ctx=ctx)
    ctx.check(ctx.lib.mdhip_velocity_spectrum(ctx.h, F, E, vp, v_dev, None if c is None else ptr(c), G, ptr(grp, C.c_int32),
                                              L, int(max_lag), sp, pp, o_dev, ptr(a0)))
    return sums, power, a0


FREE_VOLUME_MAX_CLASSES = 16   # atom classes per call of free_volume (include/mdhip.h: mdhip_free_volume)
FREE_VOLUME_MAX_BINS = 4096
FREE_VOLUME_MAX_PROBES = 8
FREE_VOLUME_MAX_POINTS = 1 << 27


def free_volume(xyz, box, atom_class, radius, grid, r_search, edges, probe=(0.0,), want_map=False, field=False,
                out=None, counts=True, ctx=None):
    """
    Free volume and cavity sizes on a grid (include/mdhip.h: mdhip_free_volume): xyz [F,3,N] (host array or contiguous
    float64 device tensor), box [F,3] edge lengths, atom_class int32 [N] in -1 .. C-1 (-1: the atom is ignored), radius
    [C], grid = (gx, gy, gz), r_search the search radius (its square is formed here, r_search * r_search), edges
    [nbins+1] from 0 ascending, probe [P] radii. Per grid point s = the distance to the nearest atom surface within
    r_search and `nearest`, the lowest atom index that attains it.
    Returns a dict: "hist" uint64 [C,nbins], "occupied" uint64 [C], "beyond" uint64 (a number) — None without `counts` —,
    "n_free" int64 [F,P], "free_map" uint32 [gx,gy,gz] with `want_map` (else None), and with `field` "s" float64
    [F,gx,gy,gz] and "nearest" int32 [F,gx,gy,gz] as host arrays, or `out` = (s, nearest), CUDA tensors of those shapes
    and dtypes float64 and int32, when given.
    """
    ctx, F, N, bx, xp, x_dev, keep = _xyz_box(xyz, box, ctx)
    cls = _i32(atom_class).ravel()
    if len(cls) != N:
        raise ValueError("atom_class must hold one class per atom")
    rad, ed, pr, g = _f64(radius).ravel(), _f64(edges).ravel(), _f64(probe).ravel(), _i32(grid).ravel()
    if len(g) != 3:
        raise ValueError("grid must hold (gx, gy, gz)")
    n_cls, nb, n_pr = len(rad), len(ed) - 1, len(pr)
    shape = tuple(max(int(v), 0) for v in g)
    G = shape[0] * shape[1] * shape[2]
    if G > FREE_VOLUME_MAX_POINTS:
        raise ValueError("the grid holds %d points; at most 2^27" % G)
    hist = np.zeros((max(n_cls, 0), max(nb, 0)), dtype=np.uint64) if counts else None
    occupied = np.zeros(max(n_cls, 1), dtype=np.uint64) if counts else None
    beyond = np.zeros(1, dtype=np.uint64) if counts else None
    n_free = np.zeros((F, max(n_pr, 1)), dtype=np.int64)
    fmap = np.zeros(shape, dtype=np.uint32) if want_map else None
    s = near = sp = npn = None
    f_dev = 0
    if out is not None:
        s, near = out
        sp, npn, f_dev = _dev_out(s, (F,) + shape, ctx=ctx), _dev_out(near, (F,) + shape, "torch.int32", ctx), 1
    elif field:
        s, near = np.empty((F,) + shape), np.empty((F,) + shape, dtype=np.int32)
        sp, npn = C.c_void_p(s.ctypes.data), C.c_void_p(near.ctypes.data)
    r = float(r_search)
    ctx.check(ctx.lib.mdhip_free_volume(
        ctx.h, F, N, xp, x_dev, ptr(bx), ptr(cls, C.c_int32), n_cls, ptr(rad), ptr(g, C.c_int32), r, r * r, nb, ptr(ed), n_pr,
        ptr(pr), None if hist is None else ptr(hist, C.c_uint64), None if hist is None else ptr(occupied, C.c_uint64),
        None if hist is None else ptr(beyond, C.c_uint64), ptr(n_free, C.c_int64),
        None if fmap is None else ptr(fmap, C.c_uint32), sp, npn, f_dev))
    return {"hist": hist, "occupied": None if occupied is None else occupied[:n_cls],
            "beyond": None if beyond is None else int(beyond[0]), "n_free": n_free[:, :n_pr], "free_map": fmap, "s": s,
            "nearest": near}
