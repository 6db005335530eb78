"""
mdhip_velocity_spectrum (csrc/velocity_spectrum.hip) and `VelocityCorrelation` on the GPU, against the numpy restatement
(tests/velocity_ref.py).

Integer input (v in -3 .. 3, coef in {1, 2, 3}) has exact int64 lag sums: the result must lie within the documented bound
4 * 2^-52 * log2(L) * a0 of them and, wherever that bound is below 0.5, round to them; a0 itself is compared with `==`.
Floating-point input is compared with long-double direct sums and a long-double direct DFT within the documented bounds,
never measured ones. Shapes are the smallest at which the kernels can go wrong: either side of the 64 x 64 tile in frames
and entities, both transform routes and the lengths at their edge, F + max_lag equal to L, groups of no and one entity,
sixteen groups, several batches, and the two launch dimensions beyond 65 535.
"""
import ctypes as C

import numpy as np
import pytest

import velocity_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _integers(seed, F, E):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, size=(F, 3, E)), rng.integers(1, 4, size=E)


def _check_integers(B, v, coef, grp, max_lag, L=None, ctx=None, poison=True, truth=None):
    """The call on integer input against the exact sums (`truth`: lag_truth and a0_truth of it, when the caller holds
    them); entities of no group hold NaN (they must never be read into a sum). Returns (sums, a0) of the call."""
    F = v.shape[0]
    L = R.default_length(F) if L is None else L
    x = v.astype(np.float64)
    if poison:
        x[:, :, np.asarray(grp) < 0] = np.nan
    G = R.n_groups_of(grp)
    got, _, a0 = B.velocity_spectrum(x, grp, max_lag, L=L, coef=None if coef is None else coef.astype(np.float64), ctx=ctx)
    if truth is None:
        s = R.series(v, coef)
        truth = R.lag_truth(s, grp, max_lag, G), R.a0_truth(s, grp, G)
    want, a0_want = truth
    assert got.shape == (max_lag + 1, G, 4) and a0.shape == (G, 4)
    assert np.array_equal(a0, a0_want.astype(np.float64))
    bound = R.sums_bound(a0_want, L)
    err = np.abs(got - want.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.nanmax(np.where(bound[None] > 0, err / bound[None], 0.0)) if err.size else 0.0
    print("F", F, "E", v.shape[2], "L", L, "lags", max_lag + 1, "worst share of the bound", float(share))
    assert np.all(err <= bound[None])
    exact = np.broadcast_to(bound[None] < 0.5, got.shape)
    assert np.array_equal(np.rint(got[exact]), want.astype(np.float64)[exact])
    return got, a0


# ---- grid of shapes ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 130])
def test_either_side_of_the_tile(B, F, E):
    v, coef = _integers(1000 * F + E, F, E)
    _check_integers(B, v, coef, R.interleaved_groups(E), F - 1)


# ---- both transform routes and their edge -------------------------------------------------------------------------------


@pytest.mark.parametrize("F,L,route", [(500, None, "r2c_power_rows"), (1024, None, "fft_power_pass"),
                                       (1025, None, "fft_power_pass"), (500, 4096, "fft_power_pass"),
                                       (63, 512, "r2c_power_rows")])
def test_both_transform_routes(B, F, L, route):
    """F = 500 -> L = 1024: the packed transform; F = 1024 -> 2048 and F = 1025 -> 4096: two passes; an L four times
    the minimum on either route."""
    v, coef = _integers(F, F, 7)
    _check_integers(B, v, coef, R.interleaved_groups(7), F - 1, L=L)
    assert route in B.default_context().last_kernel_name()


def test_equality_of_series_plus_lags_and_length(B):
    from mdproptools_amd._lib import MdhipError

    v, coef = _integers(724, 724, 5)
    grp = R.interleaved_groups(5)
    _check_integers(B, v, coef, grp, 300, L=1024)                       # F + max_lag == L: still the linear correlation
    with pytest.raises(MdhipError) as err:
        B.velocity_spectrum(v.astype(np.float64), grp, 301, L=1024)
    assert err.value.code == -1
    for max_lag in (0, 1):
        _check_integers(B, v, coef, grp, max_lag)
        _check_integers(B, v[:65], None, grp, max_lag)


# ---- groups and batches -------------------------------------------------------------------------------------------------


def test_sixteen_groups_and_the_same_bits_twice(B):
    v, coef = _integers(16, 130, 40)
    grp = (np.arange(40) * 7 % 13).astype(np.int32)                     # groups 0 .. 12 interleaved, 13 .. 15 below
    grp[5], grp[11] = 15, -1                                            # group 15: one entity; 13 and 14: none
    sizes = np.bincount(grp[grp >= 0], minlength=16)
    assert sizes[15] == 1 and sizes[13] == sizes[14] == 0 and sizes.max() > 2
    got, a0 = _check_integers(B, v, coef, grp, 129)
    assert not got[:, 13:15].any() and not a0[13:15].any()
    x = v.astype(np.float64)
    x[:, :, 11] = np.nan
    again = B.velocity_spectrum(x, grp, 129, coef=coef.astype(np.float64), want_power=True)
    assert again[0].tobytes() == got.tobytes() and again[2].tobytes() == a0.tobytes()
    third = B.velocity_spectrum(x, grp, 129, coef=coef.astype(np.float64), want_power=True)
    assert third[1].tobytes() == again[1].tobytes() and third[0].tobytes() == got.tobytes()


def test_several_batches(B):
    """lag_batch_mb = 1 at F = 700, E = 130: rows of 700 * 8 + 2048 * 8 bytes, 47 a batch, nine batches; the result
    stays within the bound of the truth the one-batch result is held to."""
    v, coef = _integers(700, 700, 130)
    grp = R.interleaved_groups(130)
    ctx = B.default_context()
    s = R.series(v, coef)
    truth = R.lag_truth(s, grp, 699), R.a0_truth(s, grp)
    one, a0 = _check_integers(B, v, coef, grp, 699, truth=truth)
    ctx.set_option("lag_batch_mb", 1)
    try:
        many, a0_many = _check_integers(B, v, coef, grp, 699, truth=truth)
    finally:
        ctx.set_option("lag_batch_mb", 0)                                # (0: the library's default)
    assert a0_many.tobytes() == a0.tobytes()
    assert _check_integers(B, v, coef, grp, 699, truth=truth)[0].tobytes() == one.tobytes()   # restored


# ---- launch limits ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("E", [22000, 66000])
def test_more_rows_than_a_launch_dimension(B, E):
    """E = 22 000: 66 000 rows in all; E = 66 000: as many series in ONE batch, which the shared transforms take in parts
    of 32 768 (the gather's own grid still has 1 032 entity tiles there: see the next test)."""
    v, coef = _integers(E, 8, E)
    _check_integers(B, v, coef, np.where(np.arange(E) % 3 == 0, 0, 1).astype(np.int32), 7)


def test_more_entity_tiles_than_a_launch_dimension(B):
    """65 538 tiles of 64 entities in one batch (F = 1, 100 MB): the gather's grid is split along the entities and its
    second launch starts at tile 65 535; the entities behind the split are checked apart."""
    E = 64 * 65537 + 5
    rng = np.random.default_rng(E)
    v, coef = rng.integers(-3, 4, size=(1, 3, E)), rng.integers(1, 4, size=E)
    grp = np.where(np.arange(E) % 3 == 0, 0, 1).astype(np.int32)
    grp[64 * 65535:] += 2                                               # groups 2 and 3: the second launch's entities alone
    got, a0 = _check_integers(B, v, coef, grp, 0)
    assert a0[2:, :3].min() > 0 and a0[2, 3] + a0[3, 3] < a0[0, 3] / 1000


def test_more_frames_than_a_launch_dimension(B):
    v, coef = _integers(70001, 70001, 2)
    _check_integers(B, v, coef, np.array([1, 0], dtype=np.int32), 5)


# ---- floating point -----------------------------------------------------------------------------------------------------

FP_F, FP_E, FP_L = 700, 14, 2048
FP_GROUPS = np.array([0, 1, 1, 2, 1, 1, 2, 1, 0, 1, 2, 1, 1, 1], dtype=np.int32)


@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(21)
    white = rng.normal(size=(FP_F, 3, FP_E))
    ar1 = np.empty_like(white)
    ar1[0] = white[0]
    for t in range(1, FP_F):
        ar1[t] = 0.9 * ar1[t - 1] + np.sqrt(1 - 0.81) * rng.normal(size=(3, FP_E))
    coef = rng.uniform(0.5, 2.0, size=FP_E)
    out = {"coef": coef}
    for name, v in (("white", white), ("ar1", ar1)):
        s = R.series(v, coef)
        out[name] = {"v": np.ascontiguousarray(v), "sums": R.lag_truth(s, FP_GROUPS, FP_F - 1, 3),
                     "a0": R.a0_truth(s, FP_GROUPS, 3)}
    out["white"]["power"] = R.power_truth(R.series(white, coef), FP_GROUPS, FP_L, 3)
    return out


@pytest.mark.parametrize("kind", ["white", "ar1"])
def test_floating_point_within_the_documented_bounds(B, floats, kind):
    d = floats[kind]
    sums, power, a0 = B.velocity_spectrum(d["v"], FP_GROUPS, FP_F - 1, L=FP_L, coef=floats["coef"], want_power=True)
    a0_want = d["a0"].astype(np.float64)
    # a0: W = 700 * (entities) terms of one rounded square each, any order: (W + 1) 2^-53 relative
    assert np.all(np.abs(a0 - a0_want) <= (FP_F * FP_E + 4) * 2.0 ** -53 * a0_want)
    bs = R.sums_bound(a0_want, FP_L)
    e = np.abs(sums - d["sums"].astype(np.float64))
    print(kind, "sums: worst share of the bound", float((e / bs[None]).max()))
    assert np.all(e <= bs[None])
    back = np.fft.irfft(power, n=FP_L, axis=2)[:, :, :FP_F]                 # [G, 4, F]
    e = np.abs(np.transpose(back, (2, 0, 1)) - sums)
    print(kind, "irfft(power) against sums: worst share of twice the bound", float((e / (2 * bs[None])).max()))
    assert np.all(e <= 2 * bs[None])
    if kind == "white":
        bp = R.power_bound(a0_want, FP_L, FP_F)
        e = np.abs(power - d["power"].astype(np.float64))
        print(kind, "power: worst share of the bound", float((e / bp[:, :, None]).max()))
        assert np.all(e <= bp[:, :, None])


# ---- non-finite input, device buffers, invalid arguments ------------------------------------------------------------------


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_stays_in_its_group_and_axis(B, floats, bad):
    v = floats["white"]["v"]
    clean = B.velocity_spectrum(v, FP_GROUPS, FP_F - 1, L=FP_L, coef=floats["coef"], want_power=True)
    x = v.copy()
    x[350, 1, 6] = bad                                                    # entity 6: group 2, axis y
    got = B.velocity_spectrum(x, FP_GROUPS, FP_F - 1, L=FP_L, coef=floats["coef"], want_power=True)
    for c, g in zip(clean, got):
        hit = np.zeros(c.shape, dtype=bool)
        if c.ndim == 3 and c.shape[1] == 3:
            hit[:, 2, 1] = hit[:, 2, 3] = True                            # sums [k][g][a]
        elif c.ndim == 3:
            hit[2, 1, :] = hit[2, 3, :] = True                            # power [g][a][j]
        else:
            hit[2, 1] = hit[2, 3] = True                                  # a0 [g][a]
        assert not np.isfinite(g[hit]).any()
        assert g[~hit].tobytes() == c[~hit].tobytes()


def test_device_buffers_give_the_same_bytes(B, floats):
    import torch

    v = floats["ar1"]["v"]
    host = B.velocity_spectrum(v, FP_GROUPS, 300, L=1024, coef=floats["coef"], want_power=True)
    dev = torch.device("cuda", B.default_context().device)
    sums = torch.full((301, 3, 4), 7.0, dtype=torch.float64, device=dev)
    power = torch.full((3, 4, 513), 7.0, dtype=torch.float64, device=dev)
    got = B.velocity_spectrum(torch.as_tensor(v, device=dev), FP_GROUPS, 300, L=1024, coef=floats["coef"], want_power=True,
                              out=(sums, power))
    assert got[0] is sums and got[1] is power
    assert sums.cpu().numpy().tobytes() == host[0].tobytes() and power.cpu().numpy().tobytes() == host[1].tobytes()
    assert got[2].tobytes() == host[2].tobytes()
    only = B.velocity_spectrum(torch.as_tensor(v, device=dev), FP_GROUPS, 300, L=1024, coef=floats["coef"], out=sums)
    assert only[1] is None and sums.cpu().numpy().tobytes() == host[0].tobytes()


def test_invalid_arguments(B):
    from mdproptools_amd._lib import MdhipError, default_context, ptr

    ctx = default_context()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    v = np.ones((8, 3, 6))
    good = dict(F=8, E=6, G=2, grp=[0, 1, 1, -1, 0, 1], L=16, max_lag=3)
    bad = [dict(G=0), dict(G=17), dict(F=0, max_lag=0), dict(E=-1), dict(grp=[0, 1, 2, -1, 0, 1]),
           dict(grp=[0, 1, 1, -2, 0, 1]), dict(grp=[0, 1, 1, -1, 0, 1 << 20]), dict(L=12), dict(L=8), dict(L=2, F=1, max_lag=0),
           dict(L=1 << 30), dict(L=0), dict(max_lag=8), dict(max_lag=-1), dict(max_lag=7, L=8),
           dict(null="v"), dict(null="grp"), dict(null="sums"), dict(null="a0")]
    for change in bad:
        c = dict(good, **{k: x for k, x in change.items() if k != "null"})
        grp = np.array(c["grp"], dtype=np.int32)
        sums, power, a0 = np.full((9, 17, 4), 77.0), np.full((17, 4, 9), 77.0), np.full((17, 4), 77.0)
        args = {"v": vp(v), "grp": ptr(grp, C.c_int32), "sums": vp(sums), "a0": ptr(a0)}
        if "null" in change:
            args[change["null"]] = None
        with pytest.raises(MdhipError) as err:
            ctx.check(ctx.lib.mdhip_velocity_spectrum(ctx.h, c["F"], c["E"], args["v"], 0, None, c["G"], args["grp"], c["L"],
                                                      c["max_lag"], args["sums"], vp(power), 0, args["a0"]))
        assert err.value.code == -1, change
        assert (sums == 77.0).all() and (power == 77.0).all() and (a0 == 77.0).all(), change
    sums, power, a0 = B.velocity_spectrum(v, good["grp"], 3, L=16, want_power=True)
    assert sums.shape == (4, 2, 4) and power.shape == (2, 4, 9) and a0.tolist() == [[16.0] * 3 + [48.0], [24.0] * 3 + [72.0]]
    for empty in (np.zeros((8, 3, 0)), np.ones((8, 3, 2))):               # no entity, and no grouped entity: zeros
        sums, power, a0 = B.velocity_spectrum(empty, [-1] * empty.shape[2], 7, want_power=True)
        assert sums.shape == (8, 1, 4) and not sums.any() and not power.any() and not a0.any()


# ---- end to end ------------------------------------------------------------------------------------------------------------

HOST_ROUNDINGS = 3 * 2.0 ** -53  # a division, a multiplication and the truth's own rounding, relative to the value


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("velocity")
    traj = R.synthetic_trajectory()
    return {"dir": d, "pattern": R.write_dumps(d, traj), "traj": traj}


def _check_tables(c, v, grp, counts, labels, coef):
    """calc_vacf, calc_vdos(window=None) and calc_diffusion of the instance against the restatement on v [F,3,E]."""
    from mdproptools_amd.common import constants

    F = v.shape[0]
    conv = constants.VELOCITY_CONVERSION["real"] ** 2
    s = R.series(v, coef)
    G = len(labels)
    a0 = R.a0_truth(s, grp, G).astype(np.float64)
    for max_lag in (None, F - 1):
        df = c.calc_vacf(max_lag=max_lag)
        n = (F - 1) // 2 + 1 if max_lag is None else F
        assert len(df) == n and np.array_equal(df["Time (s)"], (500 * np.arange(n) * 2) * constants.TIME_CONVERSION["real"])
        want = R.lag_truth(s, grp, n - 1, G)
        bound = R.sums_bound(a0, R.default_length(F))
        worst = 0.0
        for g, lab in enumerate(labels):
            w = (F - np.arange(n)) * float(counts[g])
            for a, name in enumerate(("vacf_x", "vacf_y", "vacf_z", "vacf")):
                truth = (want[:, g, a] / w * conv).astype(np.float64)
                err = np.abs(df["%s%d" % (name, lab)].to_numpy() - truth)
                tol = bound[g, a] / w * conv + HOST_ROUNDINGS * np.abs(truth)
                worst = max(worst, float((err / tol).max()))
                assert np.all(err <= tol), (lab, name)
            assert np.array_equal(df["cvv%d" % lab], df["vacf%d" % lab] / df["vacf%d" % lab][0])
        print("vacf: worst share of the bound", worst)
    c.normalize = False
    L = R.default_length(F)
    vd = c.calc_vdos(window=None)
    dt = 500 * 2 * constants.TIME_CONVERSION["real"]
    power = R.power_truth(s, grp, L, G)
    bp = R.power_bound(a0, L, F)
    assert len(vd) == L // 2 + 1
    for g, lab in enumerate(labels):
        scale = dt / (F * float(counts[g])) * conv
        truth = (power[g, 3] * scale).astype(np.float64)
        err = np.abs(vd["vdos%d" % lab].to_numpy() - truth)
        assert np.all(err <= bp[g, 3] * scale + 2 * HOST_ROUNDINGS * np.abs(truth)), lab
    c.normalize = True
    d = c.calc_diffusion()
    t = c.vacf_df["Time (s)"].to_numpy()
    for g, lab in enumerate(labels):
        y = c.vacf_df["vacf%d" % lab].to_numpy()
        want = np.sum(0.5 * (y[1:] + y[:-1])) * (t[1] - t[0]) / 3.0
        assert abs(d["D (m^2/s)"][g] - want) <= 1e-12 * np.abs(y).sum() * (t[1] - t[0])


@pytest.mark.parametrize("stream", [True, False])
def test_velocity_correlation_end_to_end(B, dumps, stream, monkeypatch):
    from mdproptools_amd.common import constants
    from mdproptools_amd.dynamical import velocity_correlation as M

    traj = dumps["traj"]
    monkeypatch.setattr(M, "STREAM", stream)
    monkeypatch.setattr(M, "BATCH_BYTES", 7 * 150 * 24)                   # seven frames per streamed batch: nine batches
    c = M.VelocityCorrelation(dumps["pattern"], timestep=2, working_dir=str(dumps["dir"]))
    v, times, labels, grp, counts, coef = c._load()
    assert labels == [1, 2, 3, 4, 5] and counts.tolist() == [25, 50, 30, 30, 15] and coef is None
    assert grp.tolist() == (traj["types"] - 1).tolist()                   # interleaved inside the molecules
    assert v.is_cuda and np.array_equal(v.cpu().numpy(), traj["v"]) and c._load()[0] is v
    _check_tables(c, traj["v"], grp, counts, labels, None)
    # centre-of-mass velocities, grouped by molecule type; the masses from the dump's column
    cm = M.VelocityCorrelation(dumps["pattern"], vel_type="com", num_mols=R.NUM_MOLS, num_atoms_per_mol=R.ATOMS_PER_MOL,
                               timestep=2, working_dir=str(dumps["dir"]))
    cm.save_mode = False
    vc, _, labels, grp, counts, _ = cm._load()
    want, mol_type, _ = R.com_velocities(traj)
    vc = vc.cpu().numpy()
    assert vc.shape == want.shape and np.all(np.abs(vc - want) <= 8 * 2.0 ** -53 * np.abs(traj["v"]).max())
    assert labels == [1, 2] and counts.tolist() == R.NUM_MOLS and grp.tolist() == (mol_type - 1).tolist()
    _check_tables(cm, vc, grp, counts, labels, None)
    # mass weighting: sqrt(m) per atom, the masses from a table by type
    w = M.VelocityCorrelation(dumps["pattern"], mass=R.MASSES, weighting="mass", timestep=2, working_dir=str(dumps["dir"]))
    w.save_mode = False
    coef = w._load()[5]
    assert np.array_equal(coef, np.sqrt(traj["mass"]))
    df = w.calc_vacf(max_lag=3)
    s = R.series(traj["v"], coef)
    a0 = R.a0_truth(s, traj["types"] - 1, 5).astype(np.float64)
    weight, conv = (60 - np.arange(4)) * 30.0, constants.VELOCITY_CONVERSION["real"] ** 2   # type 3: 30 atoms
    truth = (R.lag_truth(s, traj["types"] - 1, 3, 5)[:, 2, 3] / weight * conv).astype(np.float64)
    err = np.abs(df["vacf3"].to_numpy() - truth)
    assert np.all(err <= R.sums_bound(a0, 128)[2, 3] / weight * conv + HOST_ROUNDINGS * np.abs(truth))
    with pytest.raises(ValueError):
        w.calc_diffusion()


@pytest.mark.parametrize("stream", [True, False])
def test_several_frames_in_one_file(B, dumps, stream, monkeypatch, tmp_path):
    """One file of 23 frames, five frames per streamed batch: the trajectory tensor, sized by the files, grows as the
    frames come and holds them in order."""
    from mdproptools_amd.dynamical import velocity_correlation as M

    traj = dumps["traj"]
    with open(tmp_path / "all.dump", "w") as out:
        for f in range(23):
            with open(dumps["dir"] / ("vel.%d.dump" % traj["steps"][f])) as fh:
                out.write(fh.read())
    monkeypatch.setattr(M, "STREAM", stream)
    monkeypatch.setattr(M, "BATCH_BYTES", 5 * 150 * 24)
    c = M.VelocityCorrelation("all.dump", timestep=2, working_dir=str(tmp_path))
    v, times, labels, grp, counts, _ = c._load()
    assert tuple(v.shape) == (23, 3, 150) and v.is_contiguous() and np.array_equal(v.cpu().numpy(), traj["v"][:23])
    assert len(times) == 23 and labels == [1, 2, 3, 4, 5]


def test_refusals_of_the_dumps(B, dumps, tmp_path):
    from mdproptools_amd.dynamical.velocity_correlation import VelocityCorrelation

    no_vx = tmp_path / "no_vx"
    no_vx.mkdir()
    pattern = R.write_dumps(no_vx, dumps["traj"], frames=range(4), columns="id type mass q x y z vy vz")
    with pytest.raises(ValueError, match="'vx'"):
        VelocityCorrelation(pattern, working_dir=str(no_vx)).calc_vacf()
    gap = tmp_path / "gap"
    gap.mkdir()
    pattern = R.write_dumps(gap, dumps["traj"], frames=[0, 1, 2, 4, 5])
    with pytest.raises(ValueError, match="equally spaced"):
        VelocityCorrelation(pattern, working_dir=str(gap)).calc_vacf()
