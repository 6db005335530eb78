"""
mdhip_collective_displacement and mdhip_cross_msd (csrc/collective.hip) and Conductivity.einstein / nernst / ionicity on
the GPU, against the numpy restatement (tests/einstein_ref.py). Integer inputs are asserted by equality (every product
and partial sum is an exact double in any order); floating-point ones within bounds derived from the number of terms
and their absolute sum, never measured: |out - want| <= (3 (n - k) + 4) 2^-52 abs (each side within
(terms + 2) 2^-53 abs of the true sum, plus the division), |P - want| <= (n_g + 3) 2^-52 sum |c_e d_e|. Shapes are the
smallest at which the kernels can go wrong: 2 and 3 frames, series either side of the time stage (128) and the lag tile
(512) and of twice the tile, every lag of a 5000-frame series (ten lag tiles, several time slabs), 70 001 frames, three
lag chunks (16 groups with the |term| sums at 70 001 frames and 1101 lags: the slab sums reach the 1 GiB budget), an
empty group, group counts that take every instance of the kernel (1-4 on the diagonal, 4 x 1-4 off it, 16).
The independent check is the full-lag MSD kernel.
"""
import os

import numpy as np
import pytest

import einstein_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _exact(B, P, max_lag):
    """out and abs_out of integer-valued P equal int_sum / (n - k); the call without abs_out gives the same bits."""
    sums, cnt = R.cross_msd_exact_int(P, max_lag)
    out, ab = B.cross_msd(P, max_lag, with_abs=True)
    assert out.shape == sums.shape
    want = sums / cnt[:, None, None].astype(np.float64)
    bad = np.argwhere(out != want)
    print("lags", max_lag + 1, "mismatches", len(bad), bad[:5].tolist())
    assert np.array_equal(out, want)
    assert np.array_equal(ab, R.cross_msd(P, max_lag)[1])
    assert np.array_equal(B.cross_msd(P, max_lag), out)
    return out


def _walk_case(B, n, n_ent, off, max_lag, seed=None):
    r, w = R.int_walk(n if seed is None else seed, n, n_ent)
    want_P, _ = R.collective(r, w, 1.0, off)
    P = B.collective_displacement(r, w, off, scale=1.0)
    assert P.shape == want_P.shape and np.array_equal(P, want_P)
    return _exact(B, P, max_lag)


@pytest.mark.parametrize("n", [2, 3, R.TT - 1, R.TT, R.TT + 1, R.KT - 1, R.KT, R.KT + 1, R.KT + R.TT + 1,
                               2 * R.KT - 1, 2 * R.KT, 2 * R.KT + 1])
def test_exact_integers_at_every_lag(B, n):
    _walk_case(B, n, 7, np.array([0, 3, 7], dtype=np.int64), n - 1)


def test_exact_integers_5000_frames_every_lag_empty_middle_group(B):
    out = _walk_case(B, 5000, 257, np.array([0, 100, 100, 257], dtype=np.int64), 4999)
    assert not out[:, 1, :].any() and not out[:, :, 1].any()


def test_exact_integers_70001_frames(B):
    _walk_case(B, 70001, 3, np.array([0, 3], dtype=np.int64), 64)


def test_exact_integers_several_lag_chunks(B):
    """The chunk loop of csrc/lag_tiles.h (run_chunks), which no other shape reaches: 16 groups with the |term| sums,
    70 001 samples, 1101 lags are 3 lag tiles and, on 256 CUs, 547 time slabs that the 1 GiB budget of the slab sums
    cuts to 512 and to one tile per chunk — three chunks of ten 4 x 4 group-tile launches each, every chunk pairing its
    own tiles from its own first lag. Lags either side of every chunk boundary against int64 sums of those lags alone
    (the magnitudes stay below 2^43). mdhip_orient_corr runs the same loop, but reaches a second chunk only at about
    13 GB of input; its plan is walked natively (tests/test_lag_tiles_native_cpu.py)."""
    P = R.int_series(16, 16, 70001)
    n, max_lag = P.shape[2], 1100
    out, ab = B.cross_msd(P, max_lag, with_abs=True)
    launches = B.default_context().last_kernel_ms()[1]
    assert out.shape == ab.shape == (max_lag + 1, 16, 16)
    Pi = P.astype(np.int64)
    for k in (0, 1, 511, 512, 513, 1023, 1024, 1100):
        d = Pi[:, :, k:] - Pi[:, :, :n - k]
        want = np.tensordot(d, d, axes=([1, 2], [1, 2]))
        want_abs = np.tensordot(np.abs(d), np.abs(d), axes=([1, 2], [1, 2]))
        assert want_abs.max() < 2 ** 53
        assert np.array_equal(out[k], want / float(n - k)), k
        assert np.array_equal(ab[k], want_abs / float(n - k)), k
    assert launches == 30, launches


def test_max_lag_zero(B):
    out = _walk_case(B, 40, 5, np.array([0, 2, 5], dtype=np.int64), 0)
    assert out.shape == (1, 2, 2) and not out.any()


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7, 16])
def test_every_group_count_takes_its_kernel(B, G):
    """600 samples: two lag tiles (one of them short) and the predicated steps; G = 16 is ten launches of 4 x 4 tiles."""
    _exact(B, R.int_series(G, G, 600), 599)


@pytest.fixture(scope="module")
def gauss():
    r, w = R.gauss_walk(11, 700, 90)
    off = np.array([0, 30, 30, 70, 90], dtype=np.int64)
    P, A = R.collective(r, w, 1e-10, off)
    val, ab = R.cross_msd(P, 699)
    return {"r": r, "w": w, "off": off, "P": P, "A": A, "val": val, "abs": ab}


def test_floating_point_within_the_derived_bounds(B, gauss):
    n = 700
    P = B.collective_displacement(gauss["r"], gauss["w"], gauss["off"], scale=1e-10)
    tol_P = R.collective_bound(gauss["A"], gauss["off"])
    used = np.abs(P - gauss["P"])[tol_P > 0] / tol_P[tol_P > 0]
    print("P: worst share of the bound", used.max())
    assert np.all(np.abs(P - gauss["P"]) <= tol_P)
    assert not P[1].any()
    # the lag sums of the RESTATEMENT's P: identical inputs on both sides
    out, ab = B.cross_msd(gauss["P"], n - 1, with_abs=True)
    bound = R.cross_msd_bound(gauss["abs"], n)
    live = bound > 0
    print("out: worst share of the bound", (np.abs(out - gauss["val"])[live] / bound[live]).max(),
          "abs:", (np.abs(ab - gauss["abs"])[live] / bound[live]).max())
    assert np.all(np.abs(out - gauss["val"]) <= bound)
    assert np.all(np.abs(ab - gauss["abs"]) <= bound)
    assert np.array_equal(out, np.swapaxes(out, 1, 2)) and np.array_equal(ab, np.swapaxes(ab, 1, 2))
    # the same bits from call to call
    out2, ab2 = B.cross_msd(gauss["P"], n - 1, with_abs=True)
    assert out.tobytes() == out2.tobytes() and ab.tobytes() == ab2.tobytes()
    assert P.tobytes() == B.collective_displacement(gauss["r"], gauss["w"], gauss["off"], scale=1e-10).tobytes()


def test_one_entity_per_group_gives_the_self_part(B):
    r, w = R.gauss_walk(12, 300, 5)
    off = np.arange(6, dtype=np.int64)
    P = B.collective_displacement(r, w, off, scale=1e-10)
    assert np.array_equal(P, R.collective(r, w, 1e-10, off)[0])  # one term per sum: nothing to reorder
    out = B.cross_msd(P, 299)
    S = R.self_part(r, w, 1e-10, off, 299)
    diag = np.diagonal(out, axis1=1, axis2=2)
    bound = (3.0 * (300 - np.arange(300.0))[:, None] + 4.0) * R.EPS * S  # (non-negative terms: abs is the sum itself)
    print("worst share", (np.abs(diag - S)[1:] / bound[1:]).max())
    assert np.all(np.abs(diag - S) <= bound)


def test_merged_groups_give_the_sum_over_pairs(B, gauss):
    n, L = 700, 699
    r, w, off = gauss["r"], gauss["w"], gauss["off"]
    one = np.array([0, 90], dtype=np.int64)
    Ps, Pm = B.collective_displacement(r, w, off, scale=1e-10), B.collective_displacement(r, w, one, scale=1e-10)
    outs, abss = B.cross_msd(Ps, L, with_abs=True)
    outm, absm = B.cross_msd(Pm, L, with_abs=True)
    # each result is within half of cross_msd_bound of the true sum over ITS P; the two P differ from the true
    # collective sums by at most collective_bound each; the host adds 16 numbers
    Am = R.collective(r, w, 1e-10, one)[1]
    tol = (R.cross_msd_bound(absm, n)[:, 0, 0] + R.cross_msd_bound(abss, n).sum(axis=(1, 2))
           + R.cross_msd_input_bound(Pm, R.collective_bound(Am, one), L)[:, 0, 0]
           + R.cross_msd_input_bound(Ps, R.collective_bound(gauss["A"], off), L).sum(axis=(1, 2))
           + 17 * R.EPS * np.abs(outs).sum(axis=(1, 2)))
    diff = np.abs(outm[:, 0, 0] - outs.sum(axis=(1, 2)))
    print("worst share", (diff[1:] / tol[1:]).max())
    assert np.all(diff <= tol)


def test_invalid_arguments_are_refused_by_the_library(B):
    """Straight to the C entry points: MDHIP_EINVAL before anything is written."""
    import ctypes as C

    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    P = np.zeros((17, 3, 8))
    for G, n, max_lag in ((17, 8, 3), (0, 8, 3), (2, 8, 8), (2, 8, -1), (2, 0, 0)):
        out = np.full((9, 17, 17), 77.0)
        ab = np.full((9, 17, 17), 77.0)
        with pytest.raises(MdhipError):
            ctx.check(ctx.lib.mdhip_cross_msd(ctx.h, n, G, vp(P), 0, max_lag, vp(out), vp(ab), 0))
        assert (out == 77.0).all() and (ab == 77.0).all()
    r = np.zeros((4, 3, 6))
    w = np.ones(6)
    for G, off, F in ((17, np.arange(18), 4), (0, np.array([0]), 4), (2, np.array([0, 4, 3]), 4),
                      (2, np.array([0, 3, 7]), 4), (2, np.array([0, 3, 6]), 0)):
        off = off.astype(np.int64)
        out = np.full((17, 3, 4), 77.0)
        with pytest.raises(MdhipError):
            ctx.check(ctx.lib.mdhip_collective_displacement(ctx.h, F, 6, vp(r), 0, ptr(w), 1.0, G, ptr(off, C.c_int64),
                                                            vp(out), 0, None))
        assert (out == 77.0).all()


def test_one_entity_against_the_full_lag_msd(B):
    """An independent kernel: a one-entity group through both calls is the total column of mdhip_lag_msd on that entity
    with the weight as its scale, to the rtol 1e-10 include/mdhip.h states for it."""
    rng = np.random.default_rng(4)
    r = np.ascontiguousarray(np.cumsum(rng.normal(0.0, 0.3, size=(1000, 3, 3)), axis=0))
    w = np.array([1.5, -2.5, 0.75])
    off = np.arange(4, dtype=np.int64)
    out = B.cross_msd(B.collective_displacement(r, w, off, scale=0.5), 999)
    for e in range(3):
        msd = B.lag_msd(np.ascontiguousarray(r[:, :, e:e + 1]), 999, np.array([0, 1], dtype=np.int64), scale=w[e] * 0.5)
        assert np.allclose(out[:, e, e], np.asarray(msd)[:, 0, 3], rtol=1e-10, atol=0.0)


def test_host_and_device_inputs_give_the_same_bytes_and_nan_stays_home(B, gauss):
    import torch

    r, w, off = gauss["r"][:300], gauss["w"], gauss["off"]
    P = B.collective_displacement(r, w, off, scale=1e-10)
    out, ab = B.cross_msd(P, 299, with_abs=True)
    dev = torch.device("cuda", B.default_context().device)
    r_dev = torch.as_tensor(r, device=dev)
    P_dev = torch.empty((4, 3, 300), dtype=torch.float64, device=dev)
    wt = torch.full((300, 3, 90), 7.0, dtype=torch.float64, device=dev)
    B.collective_displacement(r_dev, w, off, scale=1e-10, out=P_dev, weighted=wt)
    assert P_dev.cpu().numpy().tobytes() == P.tobytes()
    assert np.array_equal(wt.cpu().numpy(), R.weighted(r, w, 1e-10))
    out_dev = torch.empty((300, 4, 4), dtype=torch.float64, device=dev)
    ab_dev = torch.empty((300, 4, 4), dtype=torch.float64, device=dev)
    B.cross_msd(P_dev, 299, out=out_dev, abs_out=ab_dev)
    assert out_dev.cpu().numpy().tobytes() == out.tobytes() and ab_dev.cpu().numpy().tobytes() == ab.tobytes()
    # entities outside every group weigh nothing
    inner = np.array([10, 40, 80], dtype=np.int64)
    wt.fill_(7.0)
    B.collective_displacement(r_dev, w, inner, scale=1e-10, out=torch.empty((2, 3, 300), dtype=torch.float64, device=dev),
                              weighted=wt)
    want = R.weighted(r, w, 1e-10)
    want[:, :, :10] = 0.0
    want[:, :, 80:] = 0.0
    assert np.array_equal(wt.cpu().numpy(), want)
    # NaN in one entity (group 2, the y axis, from frame 100 on)
    bad = r.copy()
    bad[100:, 1, 45] = np.nan
    Pn = B.collective_displacement(bad, w, off, scale=1e-10)
    assert np.isnan(Pn[2, 1, 100:]).all() and not np.isnan(Pn[2, 1, :100]).any()
    clean = np.ones(Pn.shape, dtype=bool)
    clean[2, 1] = False
    assert np.array_equal(Pn[clean], P[clean])
    outn = B.cross_msd(Pn, 299)
    hit = np.zeros((4, 4), dtype=bool)
    hit[2, :] = hit[:, 2] = True
    assert np.isnan(outn[1:][:, hit]).all()
    assert np.array_equal(outn[:, ~hit], out[:, ~hit])


@pytest.mark.parametrize("coords", ["unwrapped", "wrapped"])
@pytest.mark.parametrize("mass_from", ["dump", "argument"])
def test_dropin_on_dumps(coords, mass_from, tmp_path):
    from mdproptools_amd.dynamical.conductivity import Conductivity

    xu, types, q, mass = R.dump_system(21, 60)
    with_mass = mass_from == "dump"
    pattern = R.write_dumps(str(tmp_path), xu, types, q, mass, unwrapped=coords == "unwrapped", with_mass=with_mass)
    arg_mass = None if with_mass else R.TYPE_MASS
    com, q_mol, steps = R.read_dumps(pattern, mass=arg_mass)
    T = R.einstein_tables(com, q_mol, steps, "real", 2, 300.0, R.BOX ** 3)
    c = Conductivity("dump.*.lammpstrj", R.NUM_MOLS, R.ATOMS_PER_MOL, R.BOX ** 3, mass=arg_mass, temp=300.0, timestep=2,
                     units="real", working_dir=str(tmp_path))
    e = c.einstein(save=True)
    nr = c.nernst(save=True)
    ion = c.ionicity()
    print("einstein", e.tolist(), "want", T["einstein"].tolist(), "tol", T["einstein_tol"].tolist())
    print("nernst", nr.tolist(), "want", T["nernst"].tolist(), "tol", T["nernst_tol"].tolist())
    print("ionicity", ion, T["ionicity"], T["ionicity_tol"])
    assert e.shape == (4,) and nr.shape == (4,)
    assert np.all(np.abs(e - T["einstein"]) <= T["einstein_tol"])
    assert np.all(np.abs(c.onsager - T["onsager"]) <= T["onsager_tol"])
    assert not c.onsager[2, :].any() and not c.onsager[:, 2].any() and e[2] == 0.0  # the neutral solvent
    assert np.all(np.abs(nr - T["nernst"]) <= T["nernst_tol"]) and nr[2] == 0.0
    assert abs(ion - T["ionicity"]) <= T["ionicity_tol"] and 0.0 < ion
    for table, key in ((c.einstein_msd, "einstein_msd"), (c.nernst_msd, "nernst_msd")):
        assert list(table.columns) == ["t", "1", "2", "3", "tot"]
        assert np.array_equal(table["t"].to_numpy(), T["t"])
        assert np.all(np.abs(table.to_numpy()[:, 1:] - T[key]) <= T[key + "_tol"])
    for name in ("einstein", "nernst"):
        msd = np.loadtxt(os.path.join(str(tmp_path), name + "_msd.csv"), delimiter=",", skiprows=1)
        assert msd.shape == (30, 5)
        with open(os.path.join(str(tmp_path), name + "_msd.csv")) as fh:
            assert fh.readline().strip() == "t,1,2,3,tot"
        cond = np.loadtxt(os.path.join(str(tmp_path), name + "_conductivity.csv"), delimiter=",", skiprows=1)
        assert cond.shape == (4, 3) and np.all(cond[:, 0] == T["window"][0]) and np.all(cond[:, 1] == T["window"][1])
        assert np.allclose(cond[:, 2], e if name == "einstein" else nr, rtol=1e-15, atol=0.0)
    assert c.time == []
    # an explicit window and lag range, and the plot
    e2 = c.einstein(max_lag=40, initial_time=T["t"][5], final_time=T["t"][20], plot=True)
    T2 = R.einstein_tables(com, q_mol, steps, "real", 2, 300.0, R.BOX ** 3, max_lag=40, window=(5, 20))
    assert np.all(np.abs(e2 - T2["einstein"]) <= T2["einstein_tol"]) and len(c.einstein_msd) == 41
    assert os.path.exists(os.path.join(str(tmp_path), "einstein.png"))


@pytest.mark.parametrize("mass_from", ["dump", "argument"])
def test_collective_streamed_equals_load_all(mass_from, tmp_path, monkeypatch):
    """Conductivity._collective on the frame stream (four batches of two frames) == the load-everything-first route on
    the same unwrapped dumps, bit for bit: frame times, collective displacement and per-molecule weighted terms."""
    from mdproptools_amd import stream as S
    from mdproptools_amd.dynamical import conductivity as cm

    xu, types, q, mass = R.dump_system(21, 8)
    with_mass = mass_from == "dump"
    R.write_dumps(str(tmp_path), xu, types, q, mass, unwrapped=True, with_mass=with_mass)
    two_frames = 2 * 24 * xu.shape[2]
    monkeypatch.setattr(S, "DEFAULT_BATCH_BYTES", two_frames)
    orig = S.FrameStream.__init__
    sizes = []

    def small_batches(self, *a, **k):
        k["batch_bytes"] = two_frames  # taken literally: two frames per batch
        sizes.append(two_frames)
        orig(self, *a, **k)

    monkeypatch.setattr(S.FrameStream, "__init__", small_batches)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(cm, "STREAM", on)
        c = cm.Conductivity("dump.*.lammpstrj", R.NUM_MOLS, R.ATOMS_PER_MOL, R.BOX ** 3,
                            mass=None if with_mass else R.TYPE_MASS, temp=300.0, timestep=2, units="real",
                            working_dir=str(tmp_path))
        col = c._collective()
        res[on] = (col["times"], col["P"].cpu().numpy(), col["weighted"].cpu().numpy())
        assert len(sizes) == 1  # one stream, opened by the streamed route only
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert res[True][1].shape == (3, 3, 8) and np.abs(res[True][1]).max() > 0
