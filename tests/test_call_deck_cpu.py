"""
The call deck (tests/call_deck.py) tests something: shown on the CPU, from the restatements alone. For every entry the
reference result is non-trivial (hits within the cut-off, for van Hove and displacement counts beyond it too) and
make() gives the same bytes twice; every large variant is at least four times its small one in every staged input and
every result array; the capped entries overflow their cap; the three transform lengths differ; the scan entries have
the tile counts the one-pass scan's state depends on; every public kernel entry of backend.py is in the deck, and the
listed order has the neighbours the state entries are there for.
"""
import numpy as np
import pytest

import call_deck as D

_CACHE = {}


def made(name):
    if name not in _CACHE:
        inputs = D.DECK[name].make()
        _CACHE[name] = (inputs, D.DECK[name].reference(inputs))
    return _CACHE[name]


def _bytes(inputs):
    return {k: (np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in inputs.items()}


@pytest.mark.parametrize("name", sorted(D.DECK))
def test_entry_is_reproducible_and_not_trivial(name):
    e = D.DECK[name]
    inputs, want = made(name)
    assert _bytes(e.make()) == _bytes(inputs)
    for k in e.staged:
        assert inputs[k].dtype == np.float64 and inputs[k].flags.c_contiguous, k
    if "refused" in e.tags:
        assert want == ()
        return
    assert e.nontrivial(want), name
    e.check(want if e.check in (D.same, D.same_signed, D.same_bytes, D._rows_same) else _self_result(e, want), want)


def _self_result(e, want):
    """What a perfect library would return for the entries whose reference is not the result itself (exact sums for a
    bounded comparison): the criterion must accept it."""
    if e.fn == "lag_msd":
        S, Q, F, go, L = want
        return (D.lag_exact.exact_means(S, F, go)[0],)
    if e.fn == "xcorr":
        return (want[0],)
    if e.fn == "msd_windows":
        ref, n = want
        return (np.concatenate([ref[:, :3] * (n - 1), ref[:, 3:] * n], axis=1),)
    if e.fn == "green_kubo":
        acf = want[0]
        integ = np.stack([D.cpu_ref.cumtrapz(a, 0.5) for a in acf])
        return acf, integ, integ.mean(axis=0)
    return want


FAMILIES = sorted({e.fn for e in D.DECK.values() if e.size == "large"})


@pytest.mark.parametrize("fn", FAMILIES)
def test_large_is_four_times_small_in_every_array(fn):
    small = [e for e in D.DECK.values() if e.fn == fn and e.size == "small"]
    large = [e for e in D.DECK.values() if e.fn == fn and e.size == "large"]
    assert len(small) == len(large) and small
    for s, g in zip(sorted(small, key=lambda e: e.name), sorted(large, key=lambda e: e.name)):
        (si, sw), (gi, gw) = made(s.name), made(g.name)
        assert s.staged == g.staged
        for k in s.staged:
            assert gi[k].nbytes >= 4 * si[k].nbytes, (g.name, k, gi[k].shape, si[k].shape)
        sa, ga = s.arrays(sw), g.arrays(gw)
        assert len(sa) == len(ga) and sa
        for n, (a, b) in enumerate(zip(sa, ga)):
            assert b.nbytes >= 4 * a.nbytes, (g.name, n, b.shape, a.shape)
        for k in g.staged:  # the ceiling: 4 100 atoms x 12 frames, or series of 70 000 samples
            assert gi[k].size <= 3 * 4100 * 12 or gi[k].shape[-1] <= 70_000, (g.name, k, gi[k].shape)


def test_every_public_kernel_entry_is_in_the_deck():
    from mdproptools_amd import backend

    for fn in D.PUBLIC:
        assert callable(getattr(backend, fn))
        sizes = {e.size for e in D.DECK.values() if e.fn == fn}
        assert {"small", "large"} <= sizes, (fn, sizes)
    assert {e.name for e in D.DECK.values() if e.fn == "xcorr" and e.size != "state"} >= {
        "xcorr_fft_small", "xcorr_fft_large", "xcorr_direct_small", "xcorr_direct_large"}
    assert sorted(D.ORDER) == sorted(D.DECK)


@pytest.mark.parametrize("name", sorted(D.CAPS))
def test_capped_entries_overflow_their_cap(name):
    cap, where = D.CAPS[name]
    _, want = made(name)
    assert int(np.asarray(want[where]).max()) > cap, (name, int(np.asarray(want[where]).max()), cap)


def test_the_three_transform_lengths_differ():
    lengths = [D.xcorr_padded(made("xcorr_fft_small")[0]["a"].shape[1]),
               D.xcorr_padded(made("xcorr_fft_large")[0]["a"].shape[1]),
               made("lag_msd_variant4")[1][4]]
    assert lengths[:2] == [1024, 16384] and len(set(lengths)) == 3, lengths
    assert made("xcorr_fft_small_again")[0]["a"].shape == made("xcorr_fft_small")[0]["a"].shape
    plan = D.lag_planned(made("lag_msd_variant4")[0], D.VARIANT4)
    assert plan["kernel"] == "lag_msd_fft", plan  # the batched transforms: the ones that share the twiddle table


def test_the_overlap_entry_plans_the_partitioned_streams():
    """csrc/lag_plan.h: the overlapped plan is the residue-class path with lag_overlap wanted and at least three
    batches. 8193 frames is the shortest series of that path; with one or two entities there are fewer batches."""
    i = made("lag_msd_overlap")[0]
    plan = D.lag_planned(i, D.OVERLAP)
    assert plan["path"] == 3 and plan["n_batches"] >= 3, plan
    assert D.lag_planned(i, dict(D.OVERLAP, lag_overlap=0))["n_batches"] < 3
    assert i["r"].nbytes < 100 << 20


def test_the_scan_entries_have_their_tile_counts():
    shapes = [made(n)[0]["y"].shape for n in ("cumtrapz_large", "cumtrapz_70_series", "cumtrapz_two_launches")]
    assert shapes == [(3, 5000), (70, 300), (5, 1_000_001)]
    tiles = [D.scan_tiles(s) for s in shapes]
    assert tiles[:2] == [9, 70] and tiles[2] > 2048, tiles  # one launch, more than 64 series, two launches
    y = made("cumtrapz_two_launches")[0]["y"]
    assert np.array_equal(y, np.rint(y))  # integer samples, dx = 2: numpy's cumsum is exact


def test_the_listed_order_has_the_neighbours_the_state_needs():
    order = D.ORDER
    consumers = {"shell_members", "shell_coordination", "hydration_cosines", "hydration_counts", "angle_hist"}
    for name in D.CAPS:
        nxt = D.DECK[order[order.index(name) + 1]]
        assert nxt.fn in consumers - {D.DECK[name].fn} and nxt.size == "small", (name, nxt)
    k = order.index("rdf_loop_async")
    assert order[k + 1] == "rdf_cn_loop_async"
    assert [D.DECK[n].fn for n in order[k + 2:k + 6]] == ["van_hove_distinct", "sdf_hist", "orient_corr", "cumtrapz"]
    for name in ("refused_einval", "refused_python"):
        k = order.index(name)
        assert "refused" not in D.DECK[order[k - 1]].tags and "refused" not in D.DECK[order[k + 1]].tags
    k = order.index("xcorr_fft_small")
    assert order[k:k + 4] == ["xcorr_fft_small", "xcorr_fft_large", "xcorr_fft_small_again", "lag_msd_variant4"]
    k = order.index("cumtrapz_large")
    assert order[k:k + 4] == ["cumtrapz_large", "cumtrapz_70_series", "green_kubo_small", "cumtrapz_two_launches"]
