"""
Every kernel family across the 65 535 limit on gridDim.y / gridDim.z: frame, pair and series counts of 65 535, 65 536
and beyond 2 x 65 535, where an offset error, a dropped last slice or a stride bug would give wrong numbers silently.

How each entry point meets the limit (include/mdhip.h):
- msd_pairs / msd_pairs_cols / msd_pairs_dev / msd_origin (+ _async): the pair list runs in launches of <= 65 535
  pairs with offset pointers (csrc/msd.hip: msd_pairs_impl);
- segment_com / charge_flux: segment_frame_kernel strides over the (frame, plane group) steps beyond grid.y, the staged
  kernel over frame slices; type_sum_kernel runs in 65 535-frame slices;
- xcorr: the FFT path and the direct path group their series by <= 65 535;
- RDF / CN: frame batches of <= 32 768 (with the cull workspace reset at every batch);
- cumtrapz / green_kubo: refuse more than 65 535 series (a deliberate limit, tested here);
- msd_windows: no launch dimension grows with the frames (slabs <= 1024), tested past 65 535 kept frames all the same.

The inputs are built so that every sum is exact (coordinates k/1024 with small integers k, integer or power-of-two
masses, integer samples): the answer then does not depend on the summation order and the kernels are compared with
plain numpy float64 bit for bit. One case per MSD form keeps scale = 1e-10 at rtol 1e-12.
"""
import os
import sys

import numpy as np
import pytest

from oracle import cpu_ref as O
from oracle import cref as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = 65535


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ctx(B):
    return B.default_context()


def _torch():
    import torch

    return torch


def _k1024(rng, shape, k=40):
    """Exact coordinates: k/1024 with |k| <= 40."""
    return rng.integers(-k, k + 1, shape).astype(np.float64) / 1024.0


def _group_sums(v, go):
    """v [..., E] -> [..., G] sums over the entity groups (empty groups give 0) by prefix differences: exact on exact
    data, whatever the order."""
    cs = np.concatenate([np.zeros(v.shape[:-1] + (1,)), np.cumsum(v, axis=-1)], axis=-1)
    return cs[..., go[1:]] - cs[..., go[:-1]]


def _pair_ref(r, pairs, go, scale=1.0, origin=None, per_entity=True, block=8192):
    """numpy float64 of msd_pairs: sums [P,G,4] and per-entity rows [P,E,4] (or None). A pair (-1, t) takes `origin`."""
    P, E, G = len(pairs), r.shape[2], len(go) - 1
    sums = np.empty((P, G, 4))
    pe = np.empty((P, E, 4)) if per_entity else None
    for p0 in range(0, P, block):
        pr = pairs[p0:p0 + block]
        r0 = origin[None] if origin is not None and pr[0, 0] < 0 else r[pr[:, 0]]
        d = r[pr[:, 1]] * scale - r0 * scale
        d2 = d * d  # [b,3,E]
        tot = (d2[:, 0] + d2[:, 1]) + d2[:, 2]
        allc = np.concatenate([d2, tot[:, None]], axis=1)  # [b,4,E]
        sums[p0:p0 + block] = _group_sums(allc, go).transpose(0, 2, 1)
        if pe is not None:
            pe[p0:p0 + block] = allc.transpose(0, 2, 1)
    return sums, pe


# ---------------------------------------------------------------------------------------------------------- B1: MSD
GROUPS = {3: [0, 1, 1, 3], 37: [0, 20, 20, 37], 1025: [0, 0, 1025], 1026: [0, 1026, 1026]}


def _pairs(rng, F, P):
    """(0, t) for every frame, then arbitrary (t1, t0) pairs up to P."""
    head = np.column_stack([np.zeros(F, np.int32), np.arange(F, dtype=np.int32)])
    return np.concatenate([head, rng.integers(0, F, (P - F, 2)).astype(np.int32)])


@pytest.mark.parametrize("E", [3, 37, 1025, 1026])
@pytest.mark.parametrize("P", [LIM, LIM + 1, 140_000])
def test_msd_pairs_any_pair_count(B, E, P):
    """mdhip_msd_pairs / _cols / _dev with 65 535, 65 536 and 140 000 pairs over a 300-frame trajectory: E = 3, 37
    and 1025 take the scalar path (odd count, 1025 = one MSD_CHUNK + 1 in one group), 1026 the 16-byte path over two
    chunks; ragged groups with an empty one. Sums on the host and on the device, per-entity rows and strided column
    blocks (sentinels around them) are bit-equal to numpy, and the rows past 65 535 to a call on those pairs alone."""
    torch = _torch()
    rng = np.random.default_rng(E * 7 + P)
    F = 300
    r = _k1024(rng, (F, 3, E))
    go = np.array(GROUPS[E], dtype=np.int64)
    pairs = _pairs(rng, F, P)
    with_pe = P * E <= 70_000_000
    want, want_pe = _pair_ref(r, pairs, go, 0.5, per_entity=with_pe)
    if with_pe:
        sums, pe = B.msd_pairs(r, pairs, go, scale=0.5, per_entity=True)
        np.testing.assert_array_equal(pe, want_pe)
        pad = 5
        block = np.full((4, P * E + 2 * pad), -7.0)
        s2 = B.msd_pairs_cols(r, pairs, go, block[:, pad:pad + P * E], scale=0.5)
        np.testing.assert_array_equal(s2, want)
        np.testing.assert_array_equal(block[:, pad:pad + P * E], want_pe.reshape(P * E, 4).T)
        assert (block[:, :pad] == -7.0).all() and (block[:, pad + P * E:] == -7.0).all()
        if P > LIM:
            _, tail_pe = B.msd_pairs(r, pairs[LIM:], go, scale=0.5, per_entity=True)
            np.testing.assert_array_equal(pe[LIM:], tail_pe)
    else:
        sums = B.msd_pairs(r, pairs, go, scale=0.5)
    np.testing.assert_array_equal(sums, want)
    if P > LIM:
        np.testing.assert_array_equal(sums[LIM:], B.msd_pairs(r, pairs[LIM:], go, scale=0.5))
    dev = torch.full((P, len(go) - 1, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    B.msd_pairs(torch.from_numpy(r).cuda(), pairs, go, scale=0.5, out=dev)
    np.testing.assert_array_equal(dev.cpu().numpy(), want)


def test_msd_pairs_past_the_limit_physical_scale(B):
    """140 000 pairs at scale 1e-10 (the drop-in's unit factor) against the C oracle at rtol 1e-12."""
    rng = np.random.default_rng(5)
    r = np.cumsum(rng.normal(0, 0.3, (400, 3, 37)), axis=0)
    go = np.array([0, 20, 20, 37], dtype=np.int64)
    pairs = _pairs(rng, 400, 140_000)
    np.testing.assert_allclose(B.msd_pairs(r, pairs, go, scale=1e-10), C.msd_pairs(r * 1e-10, pairs, go),
                               rtol=1e-12, atol=0)


@pytest.mark.parametrize("E,F", [(3, LIM), (3, LIM + 1), (3, 140_000), (37, LIM + 1), (37, 140_000),
                                 (1025, LIM), (1025, LIM + 1)])
def test_msd_origin_any_frame_count(B, E, F):
    """mdhip_msd_origin (+ _async) with 65 535, 65 536 and 140 000 frames against a separate origin frame: host and
    device sums, host columns with sentinels and device columns, bit-equal to numpy; the frames past 65 535 equal a
    call on those frames alone; the asynchronous twin is one ticket and gives the same bits."""
    torch = _torch()
    rng = np.random.default_rng(E + F)
    r = _k1024(rng, (F, 3, E))
    origin = _k1024(rng, (3, E))
    go = np.array(GROUPS[E], dtype=np.int64)
    pairs = np.column_stack([np.full(F, -1, np.int32), np.arange(F, dtype=np.int32)])
    with_pe = F * E <= 70_000_000
    want, want_pe = _pair_ref(r, pairs, go, 1.0, origin=origin, per_entity=with_pe)
    if with_pe:
        pad = 3
        block = np.full((4, F * E + pad), np.nan)
        sums = B.msd_origin(r, origin, go, cols=block[:, :F * E])
        np.testing.assert_array_equal(block[:, :F * E], want_pe.reshape(F * E, 4).T)
        assert np.isnan(block[:, F * E:]).all()
    else:
        sums = B.msd_origin(r, origin, go)
    np.testing.assert_array_equal(sums, want)
    if F > LIM:
        np.testing.assert_array_equal(sums[LIM:], B.msd_origin(np.ascontiguousarray(r[LIM:]), origin, go))
    d_r = torch.from_numpy(r).cuda()
    d_s = torch.full((F, len(go) - 1, 4), -1.0, dtype=torch.float64, device="cuda")
    d_c = torch.full((4, F * E), -1.0, dtype=torch.float64, device="cuda") if with_pe else None
    torch.cuda.synchronize()
    B.msd_origin(d_r, torch.from_numpy(origin).cuda(), go, out=d_s, cols=d_c)
    np.testing.assert_array_equal(d_s.cpu().numpy(), want)
    if with_pe:
        np.testing.assert_array_equal(d_c.cpu().numpy(), want_pe.reshape(F * E, 4).T)
    np.testing.assert_array_equal(B.msd_origin(r, origin, go, async_=True).wait(), want)


def test_msd_origin_past_the_limit_physical_scale(B):
    rng = np.random.default_rng(6)
    F, E = 70_000, 37
    r = np.cumsum(rng.normal(0, 0.05, (F, 3, E)), axis=0)
    go = np.array([0, 20, 20, 37], dtype=np.int64)
    got = B.msd_origin(r, r[0], go, scale=1e-10)
    want = C.msd_pairs(r * 1e-10, np.column_stack([np.zeros(F, np.int32), np.arange(F, dtype=np.int32)]), go)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------- B2: Diffusion drop-in
# 10 atoms, two molecule types of two molecules each: type 1 = atoms of types (1, 2), type 2 = (1, 1, 3). The masses
# make every molecule weigh 4, so the centres are exact too.
DUMP_MASS = [1.0, 3.0, 2.0]
NUM_MOLS, ATOMS_PER_MOL = [2, 2], [2, 3]
ATOM_TYPES = np.array([1, 2, 1, 2, 1, 1, 3, 1, 1, 3])


def _walk(F, seed=11):
    """[F, N, 3] exact unwrapped coordinates: integer random walk / 1024 around distinct starting points."""
    rng = np.random.default_rng(seed)
    N = len(ATOM_TYPES)
    steps = rng.integers(-2, 3, (F, N, 3))
    steps[0] = rng.integers(0, 20_000, (N, 3))
    return np.cumsum(steps, axis=0).astype(np.float64) / 1024.0


def _write_dump(path, x):
    N = x.shape[1]
    ids = np.arange(1, N + 1)
    with open(path, "wt") as fh:
        for t in range(x.shape[0]):
            fh.write("ITEM: TIMESTEP\n%d\nITEM: NUMBER OF ATOMS\n%d\nITEM: BOX BOUNDS pp pp pp\n"
                     "0.0 50.0\n0.0 50.0\n0.0 50.0\nITEM: ATOMS id type xu yu zu\n" % (t, N))
            fh.write("".join("%d %d %.10f %.10f %.10f\n" % (ids[i], ATOM_TYPES[i], *x[t, i]) for i in range(N)))


@pytest.fixture(scope="module")
def long_dumps(tmp_path_factory):
    """A 70 000-frame dump (~35 MB) and its first 65 535 frames as a second dump."""
    x = _walk(70_000)
    d = tmp_path_factory.mktemp("long")
    os.makedirs(d / "a")
    os.makedirs(d / "b")
    _write_dump(str(d / "a" / "traj.dump"), x)
    _write_dump(str(d / "b" / "traj.dump"), x[:LIM])
    return x, str(d)


def _values(df, k=4):
    return df.to_numpy(dtype=np.float64)[:, -k:]


@pytest.mark.parametrize("msd_type", ["allatom", "com"])
def test_diffusion_dropin_past_65535_frames(long_dumps, msd_type):
    """get_msd_from_dump (avg_interval, com with the drift removed) on 70 000 frames: msd, msd_all and msd_int against
    the oracle's restatement; the first 65 535 rows of msd and msd_all are bit-equal to a run on a 65 535-frame dump."""
    from mdproptools_amd.dynamical.diffusion import Diffusion

    x, d = long_dumps
    dist = 1e-10  # DISTANCE_CONVERSION["real"]
    kw = dict(msd_type=msd_type, avg_interval=True, tao_coeff=3)
    if msd_type == "com":
        kw.update(num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL, mass=DUMP_MASS, com_drift=True)
    res = {}
    for sub in ("a", "b"):
        diff = Diffusion(timestep=1, units="real", outputs_dir=os.path.join(d, sub), diff_dir=os.path.join(d, sub))
        res[sub] = diff.get_msd_from_dump("traj.dump", **kw)
    msd, msd_all, msd_int = res["a"]
    F = x.shape[0]
    assert len(msd) == F
    if msd_type == "allatom":
        r = x * dist
        go = np.array([0, x.shape[1]])
    else:
        _, _, off, _ = O.molecule_layout(NUM_MOLS, ATOMS_PER_MOL)
        m = np.asarray(DUMP_MASS)[ATOM_TYPES - 1]
        seg_m = np.add.reduceat(m, off[:-1])
        com = np.add.reduceat(x * m[None, :, None], off[:-1], axis=1) / seg_m[None, :, None]
        go = np.array([0, 2, 4])
        from mdproptools_amd.common import constants

        r = O.remove_type_drift(com * dist, seg_m * constants.MASS_CONVERSION["real"], go)
    per = O.msd_single_origin(r)
    want = O.msd_group_mean(per, go)  # [F, G, 4]
    got = _values(msd, 4 * (len(go) - 1)).reshape(F, len(go) - 1, 4)
    tol = dict(rtol=1e-12, atol=0) if msd_type == "allatom" else dict(rtol=1e-9, atol=1e-9 * np.abs(want).max())
    np.testing.assert_allclose(got, want, **tol)
    np.testing.assert_allclose(_values(msd_all).reshape(F, -1, 4), per, **tol)
    np.testing.assert_allclose(_values(msd_int), O.msd_fixed_lag(r, 3), **tol)
    msd_b, all_b, _ = res["b"]
    np.testing.assert_array_equal(msd.to_numpy()[:LIM], msd_b.to_numpy())
    np.testing.assert_array_equal(_values(msd_all)[:LIM * per.shape[1]], _values(all_b))


def _sharded_case():
    rng = np.random.default_rng(23)
    return 140_000, _k1024(rng, (140_000, 3, 37)), np.array([0, 20, 20, 37], dtype=np.int64)


def _sharded_worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch
    import torch.distributed as dist

    from mdproptools_amd import dist as D

    dist.init_process_group("gloo", rank=rank, world_size=world)  # two ranks share the one GPU of the test box
    F, r, go = _sharded_case()
    lo, hi = D.frame_shard(F)
    assert hi - lo > LIM
    res = {}
    for tag, put in (("h", lambda a: a), ("d", lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())):
        res["s0_" + tag] = D.msd_single_origin_sharded(put(r[lo:hi]), F, go, origin_frame=0)
        res["s9_" + tag] = D.msd_single_origin_sharded(put(r[lo:hi]), F, go, origin_frame=F - 9)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_msd_single_origin_sharded_past_65535_frames_per_rank(B, tmp_path):
    """msd_single_origin_sharded over two gloo ranks of 70 000 frames each (host and device shards, the origin in
    either shard): every rank's result is bit-equal to the single-process call and to numpy."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    F, r, go = _sharded_case()
    t = np.arange(F, dtype=np.int32)
    want = {"s0": _pair_ref(r, np.column_stack([np.zeros(F, np.int32), t]), go, per_entity=False)[0],
            "s9": _pair_ref(r, np.column_stack([np.full(F, F - 9, np.int32), t]), go, per_entity=False)[0]}
    np.testing.assert_array_equal(B.msd_pairs(r, np.column_stack([np.zeros(F, np.int32), t]), go), want["s0"])
    for rank in range(2):
        g = np.load(tmp_path / ("rank%d.npz" % rank))
        for k in ("s0", "s9"):
            for tag in ("h", "d"):
                np.testing.assert_array_equal(g[k + "_" + tag], want[k])


# -------------------------------------------------------------------------------------- B3: segment_com, charge_flux
def _segments(kind, rng):
    """Segment sizes and integer masses with a power-of-two total per segment (exact centres and fluxes). 'one': 24
    atoms, one run; 'many': ~1900 atoms, two or more 1024-atom runs."""
    sizes = np.array([1, 5, 3, 7, 2, 6]) if kind == "one" else rng.integers(1, 31, 120)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mass = np.ones(int(off[-1]))
    for s, n in enumerate(sizes):
        p2 = 1 << int(n).bit_length()  # > n
        mass[off[s + 1] - 1] = p2 - (n - 1)
    q = rng.integers(-3, 4, int(off[-1])).astype(np.float64)
    return off, mass, q


SEG_CASES = [("one", F, K) for F in (LIM, LIM + 1, 140_000) for K in (1, 3, 7)] + \
            [("many", LIM, 1), ("many", LIM + 1, 3), ("many", 140_000, 1), ("many", 22_000, 7)]


@pytest.mark.parametrize("kind,F,K", SEG_CASES)
def test_segment_com_past_grid_rows(B, ctx, kind, F, K):
    """segment_com for 65 535, 65 536 and 140 000 frames of 1, 3 and 7 planes (steps = frames x plane groups: 7 planes
    at 22 000 frames is 66 000 steps) through both seg_frame kernels: bit-equal to each other and to numpy reduceat."""
    rng = np.random.default_rng(F + K)
    off, mass, _ = _segments(kind, rng)
    attr = _k1024(rng, (F, K, int(off[-1])), k=1000)
    want = np.add.reduceat(attr * mass, off[:-1], axis=2) / np.add.reduceat(mass, off[:-1])
    try:
        for mode in (1, 0):
            ctx.set_option("seg_frame", mode)
            com, _, _ = B.segment_com(attr, mass, off)
            assert ctx.last_kernel_name().startswith("segment_frame_kernel" if mode else "segment_staged_kernel")
            np.testing.assert_array_equal(com, want)
    finally:
        ctx.set_option("seg_frame", 1)


@pytest.mark.parametrize("kind", ["one", "many"])
def test_charge_flux_past_65535_frames(B, ctx, kind):
    """charge_flux over 140 000 frames (both seg_frame kernels; type sums in 65 535-frame slices): bit-equal to numpy
    at every frame and to oracle.cpu_ref.charge_flux at the frames around the slice edges."""
    rng = np.random.default_rng(3 if kind == "one" else 4)
    off, mass, q = _segments(kind, rng)
    M, F = len(off) - 1, 140_000
    st = (np.arange(M) * 2 // M).astype(np.int32)  # 0-based, non-decreasing (the oracle: 1-based)
    vel = _k1024(rng, (F, 3, int(off[-1])), k=500)
    vcom = np.add.reduceat(vel * mass, off[:-1], axis=2) / np.add.reduceat(mass, off[:-1])  # [F,3,M]
    qm = np.add.reduceat(q, off[:-1])
    want = np.stack([np.stack([(vcom[:, k, st == t] * qm[st == t]).sum(axis=1) for t in range(2)])
                     for k in range(3)])  # [3,T,F]
    try:
        for mode in (1, 0):
            ctx.set_option("seg_frame", mode)
            j = B.charge_flux(vel, mass, q, off, st, 2, 1.0, 1.0)
            np.testing.assert_array_equal(j, want)
            for f in (0, LIM - 1, LIM, LIM + 1, 2 * LIM - 1, 2 * LIM, F - 1):
                np.testing.assert_array_equal(j[:, :, f], O.charge_flux(vel[f].T, q, mass, off, st + 1, 2, 1.0, 1.0))
    finally:
        ctx.set_option("seg_frame", 1)


# ------------------------------------------------------------------------------------------------- B4: msd_windows
@pytest.mark.parametrize("tao", [1, 2, 3])
def test_msd_windows_past_65535_kept_frames(B, tao):
    """msd_windows with 65 537 .. 196 609 kept frames (196 609 frames: not a multiple of 2 or 3), bit-equal to the
    window sums of numpy and, as means, to oracle.cpu_ref.msd_fixed_lag."""
    rng = np.random.default_rng(tao)
    F, E = 196_609, 37
    r = _k1024(rng, (F, 3, E))
    kept = r[::tao]
    n = len(kept)
    assert n - 1 > LIM
    d2 = (kept[1:] - kept[:-1]) ** 2
    ax = d2.sum(axis=0)  # [3,E]
    want = np.concatenate([ax.T, ((d2[:, 0] + d2[:, 1]) + d2[:, 2]).sum(axis=0)[:, None]], axis=1)
    got = B.msd_windows(r, tao)
    np.testing.assert_array_equal(got, want)
    ref = O.msd_fixed_lag(r.transpose(0, 2, 1), tao)
    np.testing.assert_array_equal(got[:, :3] / (n - 1), ref[:, :3])
    np.testing.assert_array_equal(got[:, 3] / n, ref[:, 3])


# ------------------------------------------------------------------------------------------------------- B5: xcorr
def _direct(a, b, lag0, n_lags):
    """c[k] = sum_t a[t+k] b[t] / (n-k) of integer series: the sums are integers far below 2^53, found exactly by
    rounding their FFT value (off by ~1e-9 here, checked), then divided once as the kernels do."""
    n = a.shape[1]
    L = 1 << (2 * n - 1).bit_length()
    s = np.fft.irfft(np.fft.rfft(a, L) * np.conj(np.fft.rfft(b, L)), L)[:, lag0:lag0 + n_lags]
    exact = np.rint(s)
    assert np.abs(s - exact).max() < 1e-3
    return exact / (n - np.arange(lag0, lag0 + n_lags))


@pytest.mark.parametrize("P", [70_000, 131_075])
@pytest.mark.parametrize("n", [33, 64, 257])
def test_xcorr_many_series(B, P, n):
    """xcorr with 70 000 and 131 075 series (one or two 65 535-series groups plus a short one): the direct path on
    integer samples (auto, cross, n_lags < n, lag_begin > 0) bit-equal to numpy; the FFT path (auto and cross, all lags
    and n_lags < n) within 1e-13 |a| |b| per series on the sums c[k] (n - k)."""
    rng = np.random.default_rng(P + n)
    a = rng.integers(-50, 51, (P, n)).astype(np.float64)
    b = rng.integers(-50, 51, (P, n)).astype(np.float64)
    np.testing.assert_array_equal(B.xcorr(a, method=B.XCORR_DIRECT), _direct(a, a, 0, n))
    nl = n // 3
    np.testing.assert_array_equal(B.xcorr(a, b, method=B.XCORR_DIRECT, n_lags=nl), _direct(a, b, 0, nl))
    lb = n // 4
    np.testing.assert_array_equal(B.xcorr(a, b, method=B.XCORR_DIRECT, lag_begin=lb, n_lags=n - lb - 1),
                                  _direct(a, b, lb, n - lb - 1))
    w = n - np.arange(n)
    for x, y in ((a, a), (a, b)):
        got = B.xcorr(x, None if y is a else y, method=B.XCORR_FFT)
        exact = _direct(x, y, 0, n) * w
        bound = 1e-13 * np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1)
        assert (np.abs(got * w - exact).max(axis=1) <= bound).all()
        few = B.xcorr(x, None if y is a else y, method=B.XCORR_FFT, n_lags=nl)
        np.testing.assert_array_equal(few, got[:, :nl])


def test_xcorr_direct_slab_cap(B, ctx):
    """The direct path's time slabs are capped at 65 535 (grid.y). The default never asks for more than 6 x CUs x 4
    (6144 on 256 CUs), so the cap is reached only with the "xcorr_tile" knob AND a series of more than
    65 534 x 2016 samples (one slab is at least one 2016-step stage): 132 118 567 integer samples, two lags, 70 000
    slabs asked for. Bit-equal to numpy."""
    rng = np.random.default_rng(2016)
    n = LIM * 2016 + 7
    a = rng.integers(-3, 4, n).astype(np.float64)
    try:
        ctx.set_option("xcorr_tile", 70_000)
        got = B.xcorr(a, method=B.XCORR_DIRECT, n_lags=2)
    finally:
        ctx.set_option("xcorr_tile", 0)
    want = np.array([np.dot(a, a) / n, np.dot(a[1:], a[:-1]) / (n - 1)])
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------ B6: cumtrapz, green_kubo
def test_cumtrapz_and_green_kubo_series_limit(B, ctx):
    """cumtrapz and green_kubo at exactly 65 535 series (exact integer data, against oracle.cpu_ref.cumtrapz; the
    Green-Kubo correlation on the direct path), and a clean MdhipError at 65 536 that leaves the sentinel-filled
    results untouched. The limit is deliberate (include/mdhip.h)."""
    import ctypes

    torch = _torch()
    from mdproptools_amd._lib import MdhipError, ptr

    rng = np.random.default_rng(65535)
    n = 40
    y = rng.integers(-100, 101, (LIM, n)).astype(np.float64)
    got = B.cumtrapz(y, 0.5, leading_zero=True)
    for s in (0, 1, LIM // 2, LIM - 1):
        np.testing.assert_array_equal(got[s], O.cumtrapz(y[s], 0.5, leading_zero=True))
    np.testing.assert_array_equal(got[:, 1:], np.cumsum(0.5 * (y[:, 1:] + y[:, :-1]) / 2.0, axis=1))
    acf, integ, mean = B.green_kubo(y, method=B.XCORR_DIRECT, dx=0.5, want_mean=True)
    np.testing.assert_array_equal(acf, _direct(y, y, 0, n))
    for s in (0, LIM - 1):
        np.testing.assert_allclose(integ[s], O.cumtrapz(acf[s], 0.5), rtol=1e-13, atol=1e-13 * np.abs(acf[s]).max())
    np.testing.assert_allclose(mean, integ.mean(axis=0), rtol=1e-12)

    y1 = np.concatenate([y, y[:1]])
    out = torch.full((LIM + 1, n - 1), 3.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(MdhipError, match="65535 series"):
        B.cumtrapz(y1, 0.5, out=out)
    assert (out == 3.25).all().item()
    host = np.full((LIM + 1, n - 1), 3.25)
    with pytest.raises(MdhipError, match="65535 series"):
        ctx.check(ctx.lib.mdhip_cumtrapz(ctx.h, n, LIM + 1, y1.ctypes.data_as(ctypes.c_void_p), 0, ctypes.c_double(0.5),
                                         0, ptr(host)))
    assert (host == 3.25).all()
    acf_h, int_h, mean_h = np.full((LIM + 1, n), 3.25), np.full((LIM + 1, n - 1), 3.25), np.full(n - 1, 3.25)
    p = y1.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(MdhipError, match="65535 series"):
        ctx.check(ctx.lib.mdhip_green_kubo(
            ctx.h, n, LIM + 1, p, p, 0, B.XCORR_DIRECT, 1.0, 0.5, 1.0, 0, ptr(acf_h), ptr(int_h), ptr(mean_h)))
    assert (acf_h == 3.25).all() and (int_h == 3.25).all() and (mean_h == 3.25).all()


# ------------------------------------------------------------------------------------------------ B7: RDF, CN
RDF_REL = np.array([[1, 1], [1, 2], [2, 3]])
RDF_CUT, RDF_DDR, RDF_NB = 6.0, 0.1, 60
CN_CUT = [2.5, 3.5, 5.0]


@pytest.fixture(scope="module")
def rdf_case():
    """70 000 frames of 48 atoms of 3 types, a new box every frame, and the oracle's per-frame counts."""
    rng = np.random.default_rng(48)
    F, N = 70_000, 48
    box = 12.0 + rng.integers(0, 64, (F, 3)) / 16.0
    xyz = rng.uniform(0, 1, (F, 3, N)) * box[:, :, None]
    ty = (1 + np.arange(N) % 3).astype(np.int32)
    full = np.empty((F, RDF_NB), np.uint64)
    part = np.empty((F, len(RDF_REL), RDF_NB), np.uint64)
    cn = np.empty((F, len(RDF_REL)), np.uint64)
    rc2 = RDF_CUT * RDF_CUT
    cn2 = [c * c for c in CN_CUT]
    for f in range(F):
        full[f], part[f], _ = C.rdf_pairs(xyz[f], ty, RDF_REL, box[f], rc2, RDF_DDR, RDF_NB)
        cn[f] = C.cn_pairs(xyz[f], ty, RDF_REL, box[f], cn2)
    return xyz, ty, box, full, part, cn


@pytest.mark.parametrize("opts", [dict(rdf_cull=0), dict(rdf_cull=1), dict(rdf_batch=1000)], ids=str)
def test_rdf_cn_past_65535_frames(B, ctx, rdf_case, opts):
    """RDF, CN and RDF+CN on 70 000 frames: dense sweep, culling asked for (48 atoms are fewer than the 8 tiles of
    256 atoms culling needs, so this checks that the request falls back cleanly), and 1000-frame batches. Host frames
    are batched from a quarter of the trajectory on, device frames at 32 768: both are run. Frame sums equal the sum of
    the oracle over all frames; per-frame rows equal it at frames 0, 32 767, 32 768, 65 535, 65 536 and F - 1."""
    torch = _torch()
    xyz, ty, box, full, part, cn = rdf_case
    F = xyz.shape[0]
    rows = (0, 32767, 32768, LIM, LIM + 1, F - 1)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        for x in (xyz, torch.from_numpy(xyz).cuda()):
            f_s, p_s, ov = B.rdf_loop(x, ty, box, RDF_REL, RDF_CUT, RDF_DDR, RDF_NB, per_frame=False)
            assert ov == 0
            np.testing.assert_array_equal(f_s, full.sum(axis=0))
            np.testing.assert_array_equal(p_s, part.sum(axis=0))
            np.testing.assert_array_equal(B.cn_loop(x, ty, box, RDF_REL, CN_CUT, per_frame=False), cn.sum(axis=0))
            f_f, p_f, _ = B.rdf_loop(x, ty, box, RDF_REL, RDF_CUT, RDF_DDR, RDF_NB)
            c_f = B.cn_loop(x, ty, box, RDF_REL, CN_CUT)
            f2, p2, _, c2 = B.rdf_cn_loop(x, ty, box, RDF_REL, RDF_CUT, RDF_DDR, RDF_NB, CN_CUT)
            for f in rows:
                np.testing.assert_array_equal(f_f[f], full[f])
                np.testing.assert_array_equal(p_f[f], part[f])
                np.testing.assert_array_equal(c_f[f], cn[f])
                np.testing.assert_array_equal(f2[f], full[f])
                np.testing.assert_array_equal(p2[f], part[f])
                np.testing.assert_array_equal(c2[f], cn[f])
            np.testing.assert_array_equal(f2.sum(axis=0), full.sum(axis=0))
            np.testing.assert_array_equal(c2.sum(axis=0), cn.sum(axis=0))
            np.testing.assert_array_equal(f_f.sum(axis=0), full.sum(axis=0))
    finally:
        ctx.set_option("rdf_cull", -1)
        ctx.set_option("rdf_batch", 0)


# -------------------------------------------------------------------------------------- B8: 64-bit offsets
def test_trajectory_of_more_than_2_31_doubles(B):
    """E = 2^24 + 3 entities x 43 frames (2.16e9 doubles, 17 GB) made on the device: msd_pairs with pairs that touch
    the last frame, msd_windows, and segment_com of device input into a device result, against numpy on the frames
    copied back."""
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2**30:
        pytest.skip("needs 24 GiB of free device memory, %.1f GiB free" % (free / 2**30))
    F, E = 43, (1 << 24) + 3
    g = torch.Generator(device="cuda")
    g.manual_seed(43)
    r = torch.randint(-40, 41, (F, 3, E), generator=g, device="cuda", dtype=torch.float64) / 1024.0
    assert r.numel() > 2**31
    torch.cuda.synchronize()

    def frame(t):
        return r[t].cpu().numpy()

    go = np.array([0, 5, E], dtype=np.int64)
    pairs = np.array([[0, 42], [42, 41], [1, 42], [42, 42], [41, 0]], dtype=np.int32)
    got = B.msd_pairs(r, pairs, go)
    for p, (t0, t1) in enumerate(pairs):
        d2 = (frame(t1) - frame(t0)) ** 2
        want = np.stack([_group_sums(d2[0], go), _group_sums(d2[1], go), _group_sums(d2[2], go),
                         _group_sums((d2[0] + d2[1]) + d2[2], go)], axis=1)
        np.testing.assert_array_equal(got[p], want)

    win = B.msd_windows(r, 21)  # kept frames 0, 21, 42
    f0, f21, f42 = frame(0), frame(21), frame(42)
    d2 = (f21 - f0) ** 2 + (f42 - f21) ** 2
    np.testing.assert_array_equal(win[:, :3], d2.T)
    a1, a2 = (f21 - f0) ** 2, (f42 - f21) ** 2
    np.testing.assert_array_equal(win[:, 3], ((a1[0] + a1[1]) + a1[2]) + ((a2[0] + a2[1]) + a2[2]))
    del d2, a1, a2

    off = np.concatenate([np.arange(0, E - 3, 4), [E]]).astype(np.int64)  # 4-atom segments, the last one 7 atoms
    mass = np.ones(E)
    mass[3::4] = 5.0  # 1 + 1 + 1 + 5 = 8 per 4-atom segment
    mass[-3:] = [2.0, 2.0, 4.0]  # the last segment: 1 + 1 + 1 + 5 + 2 + 2 + 4 = 16
    M = len(off) - 1
    out = torch.empty((F, 3, M), dtype=torch.float64, device="cuda")
    B.segment_com(r, mass, off, out=out)
    msum = np.add.reduceat(mass, off[:-1])
    for t in (0, 42):
        want = np.add.reduceat(frame(t) * mass, off[:-1], axis=1) / msum
        np.testing.assert_array_equal(out[t].cpu().numpy(), want)
