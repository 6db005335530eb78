"""
CPU-only: Diffusion.get_msd_from_dump, Conductivity.get_charge_flux and the error paths of Conductivity.einstein end to
end — text dumps in, DataFrames and arrays out — with numpy stand-ins behind mdproptools_amd.backend, and the frame
loader they share (common/trajectory.py `attribute_batches`) on its own. 80 atoms (20 molecules of 3 atoms, 10 of 2),
7 frames, one file per frame, rows in another order in every file. Every backend call is recorded (name, shapes, dtypes,
bytes), so that two commits can be compared:

    python tests/test_dynamical_dropin_cpu.py dump    calls.npz     # at one commit
    python tests/test_dynamical_dropin_cpu.py compare calls.npz     # at the other
"""
import gzip
import inspect
import os
import shutil
import sys

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)
from test_dist_gloo import _numpy_dynamical_backend

NUM_MOLS, ATOMS_PER_MOL = [20, 10], [3, 2]
N, F = 80, 7
TYPES = np.concatenate([np.tile([1, 2, 1], 20), np.tile([2, 2], 10)])
CHARGE = np.concatenate([np.tile([0.5, -1.0, 0.5], 20), np.tile([1.0, 0.0], 10)])
MASS = [1.0, 12.0]
BOUNDS = [(-1.5, 18.5), (0.5, 20.0), (2.0, 23.0)]  # non-zero lo on every axis
LENGTHS = np.array([hi - lo for lo, hi in BOUNDS])
STEPS = [0, 50, 100, 150, 200, 250, 300]
SHUFFLED = [150, 0, 300, 50, 250, 100, 200]  # the timestep of file k in the out-of-time-order variant
UNWRAPPED_COLS = ["id", "type", "q", "mass", "xu", "yu", "zu", "vx", "vy", "vz"]
WRAPPED_COLS = ["id", "type", "q", "mass", "x", "y", "z", "ix", "iy", "iz", "vx", "vy", "vz"]
BACKEND_NAMES = ("segment_com", "msd_pairs", "msd_pairs_cols", "msd_windows", "charge_flux", "msd_origin")
DEVICE_ONLY_NAMES = ("collective_displacement", "cross_msd")  # behind Conductivity.einstein: no stand-in, recorded on a GPU
RESULT_ARGS = ("cols", "out", "weighted", "abs_out")  # destinations: their shape is recorded, not their bytes
TWO_FRAMES = 2 * 24 * N


def _signatures():
    from mdproptools_amd import backend

    return {name: inspect.signature(getattr(backend, name)) for name in BACKEND_NAMES + DEVICE_ONLY_NAMES}


_SIGNATURES = _signatures()  # of the real functions, before any test replaces them


def trajectory():
    """{column: [F, N] values by (frame in time order, atom id - 1)}; xu is x + ix * L to the bit. Coordinates are
    multiples of 1/256 and the box lengths of 1/2: sums and decimal texts are exact, so that the pandas reader (whose
    float parser may be an ulp off on 17 digits) and the native one read the same doubles."""
    rng = np.random.default_rng(8)
    lo = np.array([b[0] for b in BOUNDS])
    walk = np.cumsum(rng.normal(0, 0.4, (F, N, 3)), axis=0) + rng.uniform(-30, 50, (N, 3))
    walk = np.round(walk * 256) / 256
    img = np.floor((walk - lo) / LENGTHS)
    xyz = walk - img * LENGTHS
    cols = {"id": np.tile(np.arange(1, N + 1), (F, 1)), "type": np.tile(TYPES, (F, 1)), "q": np.tile(CHARGE, (F, 1)),
            "mass": np.tile(np.array(MASS)[TYPES - 1], (F, 1))}
    vel = np.round(rng.normal(0, 1e-3, (F, N, 3)), 7)
    for k, a in enumerate("xyz"):
        cols[a], cols["i" + a], cols["v" + a] = xyz[:, :, k], img[:, :, k], vel[:, :, k]
        cols[a + "u"] = cols[a] + cols["i" + a] * (BOUNDS[k][1] - BOUNDS[k][0])
    return cols


def write_case(tmp_dir, columns, steps=STEPS, data=None):
    """One file per frame, dyn.<k * 50>.dump holding the frame of timestep steps[k]; returns the directory."""
    from mdproptools_amd import io as mio

    data = data or trajectory()
    rng = np.random.default_rng(11)
    os.makedirs(tmp_dir, exist_ok=True)
    for k, ts in enumerate(steps):
        f = STEPS.index(ts)
        tbl = np.column_stack([data[c][f] for c in columns])[rng.permutation(N)]
        mio.write_dump(os.path.join(tmp_dir, "dyn.%d.dump" % (k * 50)), ts, BOUNDS, columns, tbl)
    return tmp_dir


def install(monkeypatch, log=None, real=False):
    """Puts the numpy stand-ins into mdproptools_amd.backend (`real`: leaves the real functions there); with `log` (a
    list) every call is appended to it first as (name, [its arguments as arrays]): the arguments as the real function's
    signature binds them, defaults filled in, the ones left at None and the context omitted, a destination by its shape
    only, a device tensor through .cpu() — copies, because a streamed batch's buffer is reused."""
    from mdproptools_amd import backend

    if real:
        fns = {n: getattr(backend, n) for n in BACKEND_NAMES + DEVICE_ONLY_NAMES}
    else:  # numpy's sums round by the shape of the whole batch; the kernel works frame by frame: so does this
        fns = dict(zip(BACKEND_NAMES, _numpy_dynamical_backend()))
        whole = fns["charge_flux"]
        fns["charge_flux"] = lambda vel, *a, **k: np.concatenate([whole(vel[f:f + 1], *a, **k) for f in range(len(vel))],
                                                                 axis=2)

    def as_array(name, v):
        if name in RESULT_ARGS:
            return np.array(tuple(v.shape), dtype=np.int64)
        return np.array(v.cpu().numpy() if hasattr(v, "is_cuda") else v)

    for name, fn in fns.items():
        def recorded(*args, _name=name, _fn=fn, _sig=_SIGNATURES[name], **kw):
            if log is not None:
                bound = _sig.bind(*args, **kw)
                bound.apply_defaults()
                log.append((_name, [as_array(k, v) for k, v in bound.arguments.items()
                                    if v is not None and k != "ctx"]))
            return _fn(*args, **kw)

        monkeypatch.setattr(backend, name, recorded)


def two_frame_batches(monkeypatch):
    """Every frame stream opened from here on cuts its batches after two frames."""
    from mdproptools_amd import stream as S

    orig = S.FrameStream.__init__

    def small_batches(self, *a, **k):
        k["batch_bytes"] = TWO_FRAMES  # taken literally
        orig(self, *a, **k)

    monkeypatch.setattr(S.FrameStream, "__init__", small_batches)


def _frames_per_call(log, name):
    return tuple(len(args[0]) for n, args in log if n == name)


def _same_frame(a, b):
    assert list(a.columns) == list(b.columns)
    assert [str(t) for t in a.dtypes] == [str(t) for t in b.dtypes]
    np.testing.assert_array_equal(a.to_numpy(), b.to_numpy())


# ---------------------------------------------------------------------------------------------------- charge flux
def charge_flux(tmp_dir, monkeypatch, log, stream, native, mass, filename="dyn.*.dump"):
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical import conductivity as cm

    monkeypatch.setattr(cm, "STREAM", stream)
    monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
    c = cm.Conductivity(filename, NUM_MOLS, ATOMS_PER_MOL, 8000.0, mass=mass, temp=300.0, timestep=2, units="real",
                        working_dir=tmp_dir)
    del log[:]
    return c.get_charge_flux(), np.asarray(c.time)


def expected_flux(data):
    """J [3, n_types, F] of the trajectory in SI units, from the definition."""
    from mdproptools_amd.common import constants

    m = np.array(MASS)[TYPES - 1]
    off = np.concatenate([np.arange(0, 60, 3), np.arange(60, 80, 2)])
    v = np.stack([data["vx"], data["vy"], data["vz"]], axis=1)  # [F,3,N]
    v_mol = np.add.reduceat(v * m, off, axis=2) / np.add.reduceat(m, off)
    j_mol = v_mol * constants.VELOCITY_CONVERSION["real"] * (np.add.reduceat(CHARGE, off)
                                                             * constants.CHARGE_CONVERSION["real"])
    return np.stack([j_mol[:, :, :20].sum(axis=2), j_mol[:, :, 20:].sum(axis=2)], axis=1).transpose(2, 1, 0)


@pytest.fixture(scope="module")
def flux_dir(tmp_path_factory):
    return write_case(str(tmp_path_factory.mktemp("flux")), UNWRAPPED_COLS)


def test_charge_flux_is_the_same_on_every_route_reader_and_mass_source(flux_dir, monkeypatch):
    from mdproptools_amd.common import constants

    log = []
    install(monkeypatch, log)
    two_frame_batches(monkeypatch)
    want_time = np.array([s * constants.TIME_CONVERSION["real"] * 2 for s in STEPS])
    base = None
    for stream, native in ((True, True), (False, True), (False, False), (True, False)):
        for mass in (MASS, None):
            j, time = charge_flux(flux_dir, monkeypatch, log, stream, native, mass)
            # stream on: four batches of two frames, the last one ragged; otherwise every frame in one call
            assert _frames_per_call(log, "charge_flux") == ((2, 2, 2, 1) if stream and native else (7,))
            assert [n for n, _ in log] == ["charge_flux"] * len(log)
            for _, args in log:  # masses and charges of the first frame, by id
                assert args[1].tobytes() == np.array(MASS)[TYPES - 1].tobytes() and args[2].tobytes() == CHARGE.tobytes()
            if base is None:
                base = (j, time)
                assert j.shape == (3, 2, 7) and time.tobytes() == want_time.tobytes()
                np.testing.assert_allclose(j, expected_flux(trajectory()), rtol=1e-12, atol=0)
            assert j.tobytes() == base[0].tobytes() and time.tobytes() == base[1].tobytes()


def test_charge_flux_compressed_file_takes_the_general_route(flux_dir, tmp_path, monkeypatch):
    log = []
    install(monkeypatch, log)
    two_frame_batches(monkeypatch)
    want = charge_flux(flux_dir, monkeypatch, log, False, True, MASS)
    for name in os.listdir(flux_dir):
        shutil.copy(os.path.join(flux_dir, name), str(tmp_path))
    with open(tmp_path / "dyn.150.dump", "rb") as src, gzip.open(tmp_path / "dyn.150.dump.gz", "wb") as dst:
        shutil.copyfileobj(src, dst)
    os.remove(tmp_path / "dyn.150.dump")
    j, time = charge_flux(str(tmp_path), monkeypatch, log, True, True, MASS, filename="dyn.*")
    assert _frames_per_call(log, "charge_flux") == (7,)
    assert j.tobytes() == want[0].tobytes() and time.tobytes() == want[1].tobytes()


def test_charge_flux_errors(flux_dir, tmp_path, monkeypatch):
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical import conductivity as cm

    log = []
    install(monkeypatch, log)
    no_q = write_case(str(tmp_path / "no_q"), [c for c in UNWRAPPED_COLS if c != "q"])
    for stream in (True, False):  # the stream declines a dump that lacks a column: the general route's reader names it
        with pytest.raises(ValueError) as e:
            charge_flux(no_q, monkeypatch, log, stream, True, MASS)
        assert str(e.value) == "'q' is not in list"
        with pytest.raises(KeyError) as e:
            charge_flux(no_q, monkeypatch, log, stream, False, MASS)
        assert e.value.args == ("q",)
    for stream, native in ((True, True), (False, True), (False, False)):
        monkeypatch.setattr(cm, "STREAM", stream)
        monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
        c = cm.Conductivity("dyn.*.dump", [20, 11], ATOMS_PER_MOL, 8000.0, mass=MASS, working_dir=flux_dir)
        with pytest.raises(ValueError) as e:
            c.get_charge_flux()
        assert str(e.value) == "Length of values (82) does not match length of index (80)"
    c = cm.Conductivity("dyn.*.dump", NUM_MOLS, ATOMS_PER_MOL, 8000.0, mass=MASS, working_dir=flux_dir)
    with pytest.raises(ValueError) as e:
        c._finish_flux(None, [], [], 7)  # a rank whose share of the files held no frame
    assert str(e.value) == "this rank holds no frame: use at most as many ranks as there are dump files"


# ---------------------------------------------------------------------------------------------------- MSD, general route
MSD_CASES = {
    "allatom": dict(msd_type="allatom"),
    "com": dict(msd_type="com", num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL, mass=MASS),
    "com_dump_mass": dict(msd_type="com", num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL),
    "com_drift": dict(msd_type="com", num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL, mass=MASS, com_drift=True),
    "allatom_int2": dict(msd_type="allatom", avg_interval=True, tao_coeff=2),
    "com_drift_int3": dict(msd_type="com", num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL, mass=MASS,
                           com_drift=True, avg_interval=True, tao_coeff=3),
}


def msd(tmp_dir, monkeypatch, native, stream=False, **kw):
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical import diffusion as dm

    monkeypatch.setattr(dm, "STREAM", stream)
    monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
    return dm.Diffusion(timestep=2, units="real", outputs_dir=tmp_dir, diff_dir=tmp_dir).get_msd_from_dump(
        "dyn.*.dump", **kw)


def expected_msd(data, msd_type="com", com_drift=False, avg_interval=False, tao_coeff=4, **_):
    """(msd, msd_all[, msd_int]) as arrays, from the definitions (frames in time order)."""
    from mdproptools_amd.common import constants

    dist = constants.DISTANCE_CONVERSION["real"]
    r = np.stack([data["xu"], data["yu"], data["zu"]], axis=1) * dist  # [F,3,N]
    times = np.array(STEPS) * 2 * constants.TIME_CONVERSION["real"]
    if msd_type == "allatom":
        groups, ident = [np.arange(N)], [np.arange(1, N + 1)]
    else:
        m = np.array(MASS)[TYPES - 1]
        off = np.concatenate([np.arange(0, 60, 3), np.arange(60, 80, 2)])
        mol_mass = np.add.reduceat(m, off)
        r = np.add.reduceat(r * m, off, axis=2) / mol_mass
        groups = [np.arange(20), np.arange(20, 30)]
        ident = [np.repeat([1, 2], [20, 10]), np.concatenate([np.arange(1, 21), np.arange(1, 11)])]
        if com_drift:
            for g in groups:
                w = mol_mass[g] * constants.MASS_CONVERSION["real"]
                centre = (r[:, :, g] * w).sum(axis=2) / w.sum()
                r[:, :, g] -= (centre - centre[0])[:, :, None]
    d2 = (r - r[0]) ** 2
    d2 = np.concatenate([d2, d2.sum(axis=1, keepdims=True)], axis=1)  # [F,4,E]
    E = r.shape[2]
    msd_all = np.column_stack([np.repeat(times, E)] + [np.tile(v, F) for v in ident] + [d2[:, k].reshape(-1) for k in range(4)])
    out = (np.column_stack([times] + [d2[:, k][:, g].mean(axis=1) for g in groups for k in range(4)]), msd_all)
    if avg_interval:
        kept = r[::tao_coeff]
        w2 = ((kept[1:] - kept[:-1]) ** 2).sum(axis=0)  # [3,E]
        out += (np.column_stack(ident + [w2[k] / (len(kept) - 1) for k in range(3)] + [w2.sum(axis=0) / len(kept)]),)
    return out


@pytest.fixture(scope="module")
def msd_dirs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("msd"))
    return {"unwrapped": write_case(os.path.join(tmp, "u"), UNWRAPPED_COLS),
            "wrapped": write_case(os.path.join(tmp, "w"), WRAPPED_COLS),
            "shuffled": write_case(os.path.join(tmp, "s"), UNWRAPPED_COLS, steps=SHUFFLED)}


@pytest.mark.parametrize("case", sorted(MSD_CASES))
def test_msd_general_route_every_reader_and_coordinate_form(msd_dirs, monkeypatch, case):
    """Dumped xu yu zu, x + ix * L of wrapped dumps, files out of time order, native and pandas reader: the same
    DataFrames to the bit, and the definitions' values."""
    log = []
    install(monkeypatch, log)
    kw = MSD_CASES[case]
    base = msd(msd_dirs["unwrapped"], monkeypatch, True, **kw)
    assert len(base) == (3 if kw.get("avg_interval") else 2)
    # a coordinate |r| <= 60e-10 m carries a few ulp of error (8 eps |r| covers the weighted mean of three atoms), a
    # displacement d the same, its square 2 d times that; sums of up to 80 squares add 80 eps relative
    eps = np.finfo(np.float64).eps
    for got, want in zip(base, expected_msd(trajectory(), **kw)):
        assert got.shape == want.shape
        np.testing.assert_allclose(got.to_numpy(dtype=np.float64), want, rtol=100 * eps,
                                   atol=2 * np.sqrt(want[:, -1].max()) * 8 * eps * 60e-10)
    head = ["id"] if kw["msd_type"] == "allatom" else ["type", "mol_id"]
    assert list(base[1].columns) == ["Time (s)"] + head + ["dx2", "dy2", "dz2", "msd"]
    assert all(base[1][c].dtype == np.int64 for c in head)
    for kind in ("unwrapped", "wrapped", "shuffled"):
        for native in (True, False):
            del log[:]
            for a, b in zip(msd(msd_dirs[kind], monkeypatch, native, **kw), base):
                _same_frame(a, b)
            calls = [n for n, _ in log]  # one library call each: every frame in one batch
            assert calls == (["segment_com"] if kw["msd_type"] == "com" else []) + ["msd_pairs_cols"] + (
                ["msd_windows"] if kw.get("avg_interval") else [])
            assert log[0][1][0].shape == (7, 3, N)
    # the stream declines wrapped dumps (nothing to unwrap them with there): the general route serves them
    for a, b in zip(msd(msd_dirs["wrapped"], monkeypatch, True, stream=True, **kw), base):
        _same_frame(a, b)


def test_msd_reads_the_frames_in_file_order_and_unwraps_to_the_bit(msd_dirs, monkeypatch):
    """What the one segment_com call of the general route receives: the frames in file order (the time sort comes
    after), atoms by id, x + ix * L computed as written here, the first frame's masses."""
    data = trajectory()
    for native in (True, False):
        for kind, steps in (("wrapped", STEPS), ("shuffled", SHUFFLED)):
            log = []
            install(monkeypatch, log)
            msd(msd_dirs[kind], monkeypatch, native, **MSD_CASES["com"])
            name, args = log[0]
            order = [STEPS.index(s) for s in steps]
            want = np.stack([data["x"] + data["ix"] * (BOUNDS[0][1] - BOUNDS[0][0]),
                             data["y"] + data["iy"] * (BOUNDS[1][1] - BOUNDS[1][0]),
                             data["z"] + data["iz"] * (BOUNDS[2][1] - BOUNDS[2][0])], axis=1)[order]
            assert name == "segment_com" and args[0].tobytes() == want.tobytes()
            assert args[1].tobytes() == np.array(MASS)[TYPES - 1].tobytes()


# ---------------------------------------------------------------------------------------------------- the loader alone
def _batches_of(*args, **kw):
    from mdproptools_amd.common import trajectory as T

    return list(T.attribute_batches(*args, **kw)[1])


def _gather(loaded):
    """(route chosen, batch sizes, timesteps, first rows, second rows, planes) of a run of the loader, copied."""
    streamed, batches = loaded
    got = [(np.array(ts), np.array(a), np.array(b), np.array(p)) for ts, a, b, p in batches]
    return (streamed, [len(g[0]) for g in got]) + tuple(np.concatenate([g[k] for g in got]) for k in range(4))


@pytest.mark.parametrize("leading,planes", [(("q", "mass"), ("vx", "vy", "vz")), (("q", "type"), ("vx", "vy", "vz")),
                                            (("q", "mass"), ("xu", "yu", "zu")), (("id", "type"), ("xu", "yu", "zu")),
                                            (("id", "id"), ("xu", "yu", "zu"))])
def test_loader_streamed_and_general_routes_hand_out_the_same_frames(flux_dir, monkeypatch, leading, planes):
    from mdproptools_amd import io as mio
    from mdproptools_amd.common import trajectory as T

    data = trajectory()
    pattern = os.path.join(flux_dir, "dyn.*.dump")
    files = [os.path.join(flux_dir, "dyn.%d.dump" % k) for k in (100, 150, 200)]
    for share, frames in ((None, slice(0, 7)), (files, slice(2, 5))):
        want = [data[c][frames].astype(np.float64) for c in leading] + [np.stack([data[c][frames] for c in planes], axis=1)]
        for route in ("stream", "native", "pandas"):
            monkeypatch.setattr(mio, "USE_NATIVE_READER", route != "pandas")
            if route == "pandas" and share is not None:
                continue  # a share of the files goes with the native reader
            flag, sizes, steps, first, second, xyz = _gather(T.attribute_batches(
                pattern, leading, planes, n_atoms=N, files=share, stream=route == "stream", batch_bytes=TWO_FRAMES))
            n = frames.stop - frames.start
            assert flag == (route == "stream")  # which route serves, known before the first batch
            assert sizes == ([2] * (n // 2) + [1] * (n % 2) if route == "stream" else [n])
            assert steps.tolist() == STEPS[frames]
            assert first.shape == second.shape == (n, N) and xyz.shape == (n, 3, N)
            for got, ref in zip((first, second, xyz), want):
                assert got.dtype == np.float64 and got.tobytes() == ref.tobytes()


def test_loader_route_choice_unwrapping_and_the_count_check(flux_dir, msd_dirs, tmp_path, monkeypatch):
    from mdproptools_amd import io as mio
    from mdproptools_amd.common import trajectory as T

    data = trajectory()
    want = np.stack([data["xu"], data["yu"], data["zu"]], axis=1)
    lacking = []
    # wrapped dumps, and the stream switched off by the caller or with the reader: the general route, one batch
    for directory, stream, native in ((msd_dirs["wrapped"], True, True), (flux_dir, False, True), (flux_dir, True, False)):
        monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
        flag, sizes, steps, first, second, xyz = _gather(T.attribute_batches(
            os.path.join(directory, "dyn.*.dump"), ("q", "type"), T.UNWRAPPED, stream=stream, batch_bytes=TWO_FRAMES,
            missing=lambda cols, names: lacking.append(cols)))
        assert (flag, sizes, steps.tolist()) == (False, [7], STEPS) and xyz.tobytes() == want.tobytes()
        assert first.tobytes() == data["q"].tobytes() and second.tobytes() == data["type"].astype(np.float64).tobytes()
    assert lacking == []
    # the pandas reader takes the caller's own parsed dumps
    monkeypatch.setattr(mio, "USE_NATIVE_READER", False)
    dumps = list(mio.parse_lammps_dumps(os.path.join(flux_dir, "dyn.*.dump")))[:3]
    _, sizes, steps, _, _, xyz = _gather(T.attribute_batches("nothing.*", ("q", "mass"), T.UNWRAPPED, dumps=iter(dumps)))
    assert sizes == [3] and steps.tolist() == STEPS[:3] and xyz.tobytes() == want[:3].tobytes()
    monkeypatch.setattr(mio, "USE_NATIVE_READER", True)
    # no file, and no frame: nothing is handed out
    streamed, batches = T.attribute_batches(str(tmp_path / "none.*.dump"), ("q", "mass"), T.UNWRAPPED)
    assert not streamed and list(batches) == []
    # the atom count is checked on every route, on every frame
    for stream in (True, False):
        with pytest.raises(ValueError) as e:
            _batches_of(os.path.join(flux_dir, "dyn.*.dump"), ("q", "mass"), T.UNWRAPPED, n_atoms=81, stream=stream)
        assert str(e.value) == "Length of values (81) does not match length of index (80)"
    # what the dump lacks is handed to the caller's callback, in the order id, leading columns, coordinates
    seen = []
    with pytest.raises(ValueError):  # (the callback returned: the reader names the first one itself)
        _batches_of(os.path.join(flux_dir, "dyn.*.dump"), ("charge", "mass"), ("x", "y", "z"),
                    missing=lambda cols, names: seen.append((cols, "id" in names)))
    assert seen and all(s == (["charge", "x", "y", "z"], True) for s in seen)  # (once or more per frame)
    del seen[:]
    no_images = write_case(str(tmp_path / "no_images"), ["id", "type", "x", "y", "z"])
    with pytest.raises(ValueError):
        _batches_of(os.path.join(no_images, "dyn.*.dump"), ("id", "mass"), T.UNWRAPPED,
                    missing=lambda cols, names: seen.append(cols), decide_on=("zu",))
    assert seen and all(s == ["mass", "ix", "iy", "iz"] for s in seen)


# ---------------------------------------------------------------------------------------------------- error texts
def test_error_texts_of_diffusion(msd_dirs, tmp_path, monkeypatch):
    """The texts are the parent commit's (and the reference's), copied as literals."""
    install(monkeypatch)
    com = MSD_CASES["com_dump_mass"]

    def raised(kind, columns, native, data=None, **kw):
        d = write_case(str(tmp_path / ("%s_%d" % ("_".join(columns), data is not None))), columns, data=data)
        with pytest.raises(kind) as e:
            msd(d, monkeypatch, native, **kw)
        return e.value

    for native in (True, False):
        for stream in (True, False):
            with pytest.raises(ValueError) as e:
                msd(msd_dirs["unwrapped"], monkeypatch, native, stream=stream, msd_type="atoms")
            assert str(e.value) == "msd_type must be 'allatom' or 'com'."
        e = raised(AssertionError, ["type", "mass", "xu", "yu", "zu"], native, **com)
        assert str(e) == "Missing atom id's in dump file."
        e = raised(AssertionError, ["id", "type", "xu", "yu", "zu"], native, **com)
        assert str(e) == "Missing atom masses in dump file."
        e = raised(AssertionError, ["id", "type", "q", "mass"], native, **com)
        assert str(e) == "Missing wrapped and unwrapped coordinates (x y z xu yu zu)"
        e = raised(AssertionError, ["id", "type", "q"], native, **com)  # neither coordinates nor masses: the former
        assert str(e) == "Missing wrapped and unwrapped coordinates (x y z xu yu zu)"
        e = raised(AssertionError, ["id", "type", "mass", "x", "y", "z"], native, msd_type="allatom")
        assert str(e) == ("Missing unwrapped coordinates (xu yu zu) and box location (ix iy iz) for converting "
                          "wrapped coordinates (x y z) into unwrapped coordinates. ")
        changed = trajectory()
        changed["mass"] = changed["mass"].copy()
        changed["mass"][4, 17] = 3.0
        e = raised(ValueError, ["id", "type", "mass", "xu", "yu", "zu"], native, data=changed, **com)
        assert str(e) == "atom masses change between frames"
        e = raised(ValueError, ["id", "type", "xu", "yu", "zu"], native, msd_type="com", num_mols=[20, 11],
                   num_atoms_per_mol=ATOMS_PER_MOL, mass=MASS)
        assert str(e) == "Length of values (82) does not match length of index (80)"
        no_origin = write_case(str(tmp_path / "late"), UNWRAPPED_COLS, steps=STEPS[1:])
        with pytest.raises(KeyError) as e:
            msd(no_origin, monkeypatch, native, msd_type="allatom")
        assert e.value.args == (0,)


def test_error_texts_of_conductivity_einstein(tmp_path, monkeypatch):
    """Conductivity names the first column it lacks in its own words; all of them are raised before the GPU is asked for
    anything, on either reader, with the stream on or off. (One case differs from the commit before the shared loader:
    a dump without `id` read through pandas failed in sort_values with KeyError('id'); it now gets the same text as on
    the native reader.)"""
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical import conductivity as cm

    install(monkeypatch)
    cases = ((["id", "type", "mass", "xu", "yu", "zu"], "Missing column 'q' in dump file."),
             (["type", "q", "mass", "xu", "yu", "zu"], "Missing column 'id' in dump file."),
             (["id", "type", "q", "xu", "yu", "zu"], "Missing column 'mass' in dump file."),
             (["id", "type", "q"], "Missing column 'mass' in dump file."),
             (["id", "type", "q", "mass"], "Missing column 'x' in dump file (no xu yu zu to use instead)."),
             (["id", "type", "q", "mass", "xu", "yu"], "Missing column 'x' in dump file (no xu yu zu to use instead)."),
             (["id", "type", "q", "mass", "x", "y", "z"], "Missing column 'ix' in dump file (no xu yu zu to use instead)."))
    for columns, text in cases:
        d = write_case(str(tmp_path / "_".join(columns)), columns)
        for stream, native in ((True, True), (False, True), (False, False)):
            monkeypatch.setattr(cm, "STREAM", stream)
            monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
            c = cm.Conductivity("dyn.*.dump", NUM_MOLS, ATOMS_PER_MOL, 8000.0, working_dir=d)
            with pytest.raises(ValueError) as e:
                c.einstein(max_lag=3)
            assert str(e.value) == text
    d = write_case(str(tmp_path / "wrong_count"), WRAPPED_COLS)
    c = cm.Conductivity("dyn.*.dump", [20, 11], ATOMS_PER_MOL, 8000.0, working_dir=d)
    with pytest.raises(ValueError) as e:
        c.nernst(max_lag=3)
    assert str(e.value) == "Length of values (82) does not match length of index (80)"


# ---------------------------------------------------------------------------------------------------- no file at all
def test_a_pattern_without_files(tmp_path, monkeypatch):
    """Pinned at the parent commit: the flux is an empty array and no time is recorded, get_msd_from_dump fails in
    numpy's words for an empty stack, einstein and nernst say that no frames match — on every route and reader."""
    from mdproptools_amd import io as mio
    from mdproptools_amd.dynamical import conductivity as cm

    log = []
    install(monkeypatch, log)
    for stream, native in ((True, True), (False, True), (False, False)):
        j, time = charge_flux(str(tmp_path), monkeypatch, log, stream, native, MASS, filename="none.*.dump")
        assert j.shape == (3, 2, 0) and j.dtype == np.float64 and time.shape == (0,)
        for case in ("allatom", "com"):
            with pytest.raises(ValueError) as e:
                msd(str(tmp_path), monkeypatch, native, stream=stream, **MSD_CASES[case])
            assert str(e.value) == "need at least one array to stack"
        monkeypatch.setattr(cm, "STREAM", stream)
        monkeypatch.setattr(mio, "USE_NATIVE_READER", native)
        c = cm.Conductivity("none.*.dump", NUM_MOLS, ATOMS_PER_MOL, 8000.0, mass=MASS, working_dir=str(tmp_path))
        for method in (c.einstein, c.nernst):
            with pytest.raises(ValueError) as e:
                method()
            assert str(e.value) == "no frames match %s/none.*.dump" % tmp_path
    assert log == []


# ---------------------------------------------------------------------------------------------------- the call record
def record_calls(tmp_dir):
    """{key: array} of every backend call of the cases above: 'k<case>_c<call>_<name>_a<k>' holds argument k of a call,
    'k<case>_r<k>' a returned array."""
    rec = {}
    dirs = {"unwrapped": write_case(os.path.join(tmp_dir, "u"), UNWRAPPED_COLS),
            "wrapped": write_case(os.path.join(tmp_dir, "w"), WRAPPED_COLS),
            "shuffled": write_case(os.path.join(tmp_dir, "s"), UNWRAPPED_COLS, steps=SHUFFLED)}
    packed = os.path.join(tmp_dir, "z")
    shutil.copytree(dirs["unwrapped"], packed)
    with open(os.path.join(packed, "dyn.150.dump"), "rb") as src, \
            gzip.open(os.path.join(packed, "dyn.150.dump.gz"), "wb") as dst:
        shutil.copyfileobj(src, dst)
    os.remove(os.path.join(packed, "dyn.150.dump"))

    def keep(case, log, results):
        for c, (name, args) in enumerate(log):
            for j, a in enumerate(args):
                rec["k%s_c%03d_%s_a%d" % (case, c, name, j)] = a
        for k, r in enumerate(results):
            rec["k%s_r%d" % (case, k)] = np.asarray(r)

    with pytest.MonkeyPatch.context() as mp:
        log = []
        install(mp, log)
        two_frame_batches(mp)
        for stream, native in ((True, True), (False, True), (False, False)):
            for mass in (MASS, None):
                case = "flux_s%d_n%d_m%d" % (stream, native, mass is None)
                keep(case, log, charge_flux(dirs["unwrapped"], mp, log, stream, native, mass))
        keep("flux_gz", log, charge_flux(packed, mp, log, True, True, MASS, filename="dyn.*"))
        for kind in sorted(dirs):
            for native in (True, False):
                for name in sorted(MSD_CASES):
                    del log[:]
                    frames = msd(dirs[kind], mp, native, **MSD_CASES[name])
                    keep("msd_%s_n%d_%s" % (kind, native, name), log, [df.to_numpy() for df in frames])
    return rec


def compare_records(got, want):
    """Asserts two records equal — keys (so: number, order and names of the calls), dtypes, shapes and bytes — and
    returns (number of backend calls, number of argument arrays, number of returned arrays) compared."""
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), key
    arrays = [k for k in want if "_c" in k and k.rsplit("_a", 1)[-1].isdigit()]
    return len({k.rsplit("_a", 1)[0] for k in arrays}), len(arrays), len(want) - len(arrays)


def test_the_call_record_repeats(tmp_path):
    """Two recordings of the same commit are equal: what `compare` reports between two commits is theirs."""
    a = record_calls(str(tmp_path / "a"))
    b = record_calls(str(tmp_path / "b"))
    n_calls, n_arrays, n_results = compare_records(a, b)
    assert n_calls >= 7 * 1 + 6 * (4 + 1) and n_arrays > 4 * n_calls and n_results >= 14 + 36 * 2


if __name__ == "__main__":
    import tempfile

    mode, path = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        record = record_calls(tmp)
    if mode == "dump":
        np.savez(path, **record)
        print("wrote", len(record), "arrays to", path)
    else:
        print("identical: %d backend calls, %d argument arrays, %d returned arrays" %
              compare_records(record, dict(np.load(path))))
