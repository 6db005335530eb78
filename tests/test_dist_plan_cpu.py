"""
CPU: the shard plan of mdproptools_amd.dist (pure arithmetic, no process group) and the collective sequence of one fused
MSD step (gloo, the oracle standing in for the kernels). The numbers of the sharded paths are tests/test_dist_gloo.py's.
"""
import os
import sys

import numpy as np
import pytest

from test_dist_gloo import REPO, _free_port, _np_windows, _walk


# ------------------------------------------------------------------ the plan: which rank holds what
def _count_splits(F, world):
    """None (frame_shard's even split) and, where there is room, a split with empty ranks in the middle."""
    yield None
    if world >= 3:
        counts = [0] * world
        counts[0], counts[-1] = F // 2, F - F // 2
        yield counts


def test_frame_plan_properties():
    from mdproptools_amd.dist import _FramePlan

    for F in (1, 2, 5, 11, 64):
        for world in (1, 2, 3, 8):
            for counts in _count_splits(F, world):
                for tao in (1, 2, 3, 7, F + 1):
                    kept_all = list(range(0, F, tao))
                    for origin in range(F):
                        plans = [_FramePlan(F, tao, origin, counts, rank, world) for rank in range(world)]
                        kept, windows = [], 0
                        for rank, p in enumerate(plans):
                            assert (p.lo, p.hi) == p.blocks[rank] and p.blocks == plans[0].blocks
                            kept += [p.lo + int(k) for k in p.kept_local]
                            assert all(p.lo <= p.lo + int(k) < p.hi for k in p.kept_local)
                            if len(p.kept_local):
                                assert p.k0 == int(p.kept_local[0])
                            below = [q for q in range(rank) if len(plans[q].kept_local)]
                            assert p.halo_rank == (below[-1] if below else None)
                            windows += max(len(p.kept_local) - 1, 0)
                            windows += 1 if len(p.kept_local) and p.halo_rank is not None else 0
                            assert p.owner == plans[0].owner
                        assert kept == kept_all  # (rank order is frame order: the union, once each, ascending)
                        assert windows == len(kept_all) - 1
                        lo, hi = plans[0].blocks[plans[0].owner]
                        assert lo <= origin < hi


@pytest.mark.parametrize("E, group_off", [
    (1, [0, 1]),
    (7, [0, 0, 7]),               # an empty group in front
    (7, [0, 3, 3, 7]),            # an empty group in the middle
    (300, [0, 100, 300]),
    (300, [0, 10, 290, 300]),     # group 1 straddles every boundary of 3 and 8 ranks
    (300, [0, 150, 150, 300]),    # an empty group AT a rank boundary (world 2)
])
def test_lag_shard_properties(E, group_off):
    from mdproptools_amd.dist import _LagShard, entity_shard

    goff = np.asarray(group_off)
    G = len(goff) - 1
    for world in (1, 2, 3, 8):
        for F, n_lags in ((5, 5), (11, 4)):
            total = np.zeros((n_lags, G))
            for rank in range(world):
                e_lo, e_hi = entity_shard(E, rank, world)
                s = _LagShard(group_off, (e_lo, e_hi), F, n_lags)
                expect = (F - np.arange(n_lags))[:, None] * (goff[1:] - goff[:-1])[None, :]
                assert np.array_equal(s.counts, expect.astype(np.float64))
                # what the rank holds of group g, counted entity by entity
                part = [len(range(max(goff[g], e_lo), min(goff[g + 1], e_hi))) for g in range(G)]
                assert s.held == [g for g in range(G) if part[g] > 0]
                if not s.held:
                    assert e_hi == e_lo or all(p == 0 for p in part)
                    continue
                # contiguous: between the first and the last held group only groups that are empty everywhere are left
                # out, so the held groups' columns follow each other in the slice without a gap
                assert all(g in s.held or goff[g + 1] == goff[g] for g in range(s.held[0], s.held[-1] + 1))
                assert s.weights.shape == (n_lags, len(s.held))
                first = max(goff[s.held[0]], e_lo) - e_lo  # this rank's first held column
                assert s.loc_off[0] == first and len(s.loc_off) == len(s.held) + 1
                assert np.all(np.diff(s.loc_off) > 0) and np.array_equal(np.diff(s.loc_off), [part[g] for g in s.held])
                assert (s.cols.start, s.cols.stop) == (first, first + sum(part))
                total[:, s.held] += s.weights
            assert np.array_equal(total, expect.astype(np.float64))  # integers in float64: exact


# ------------------------------------------------------------------ the collectives of one fused step
def _sequence_worker(rank, world, port, out_dir, post_group):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      MDHIP_STEP_POST_GROUP="1" if post_group else "0")
    import torch.distributed as dist

    from mdproptools_amd import dist as D
    from oracle import cref

    dist.init_process_group("gloo", rank=rank, world_size=world)
    stand_in = {
        "origin": lambda rr, r0, goff, sc: cref.msd_pairs(np.concatenate([r0[None], rr]) * sc,
                                                          [(0, 1 + t) for t in range(len(rr))], goff),
        "windows": lambda rr, tao, sc: _np_windows(rr[::tao], sc),
        "lag": lambda x, ml, goff, sc: cref.lag_msd(np.asarray(x) * sc, np.arange(ml + 1), goff),
    }
    log = []

    def recorded(name, fn):
        def wrapper(*args, **kwargs):
            tensors = [a for a in args if hasattr(a, "dtype") and hasattr(a, "numel")]
            group = kwargs.get("group")
            log.append((name, tuple(tensors[-1].shape), str(tensors[-1].dtype),
                        "default" if group is None or group is dist.group.WORLD else "other"))
            return fn(*args, **kwargs)
        return wrapper

    for name in ("all_gather", "all_gather_into_tensor", "all_reduce", "broadcast"):
        setattr(dist, name, recorded(name, getattr(dist, name)))
    E, goff = 30, [0, 10, 30]
    e_lo, e_hi = D.entity_shard(E)
    per_step = []
    for F, tao, origin in ((2, 1, 1), (7, 3, 4)):  # (F = 2: rank 2 of 3 holds no frame)
        rw = _walk(F, E)
        lo, hi = D.frame_shard(F)
        del log[:]
        D.msd_step_sharded_async(rw[lo:hi], rw[:, :, e_lo:e_hi], F, (e_lo, e_hi), goff, tao, scale=1e-10, lag_scale=2.0,
                                 origin_frame=origin, compute=stand_in).wait()
        per_step.append((F, list(log)))
    with open(os.path.join(out_dir, "seq%d.txt" % rank), "w") as fh:
        fh.write(repr(per_step))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("post_group", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_fused_step_is_one_all_gather_and_one_all_reduce(tmp_path, world, post_group):
    """msd_step_sharded_async's promise: ONE collective before the kernels — an all-gather of two frames [2, 3, E] per
    rank, default group — and ONE after them — an all-reduce of F G 4 + E 4 + F G 4 + 2 float64 words, on the default
    group or (MDHIP_STEP_POST_GROUP=1) on the second communicator. On every rank, one without frames included."""
    import ast

    import torch.multiprocessing as mp

    mp.spawn(_sequence_worker, args=(world, _free_port(), str(tmp_path), post_group), nprocs=world, join=True)
    E, G = 30, 2
    for rank in range(world):
        per_step = ast.literal_eval((tmp_path / ("seq%d.txt" % rank)).read_text())
        assert [F for F, _ in per_step] == [2, 7]
        for F, log in per_step:
            assert len(log) == 2, (rank, F, log)
            gather, reduce_ = log
            assert gather[0] in ("all_gather", "all_gather_into_tensor") and gather[1:] == ((2, 3, E), "torch.float64", "default")
            assert reduce_ == ("all_reduce", (F * G * 4 + E * 4 + F * G * 4 + 2,), "torch.float64",
                               "other" if post_group else "default"), (rank, F, log)
