"""
mdproptools_amd/common/trajectory.py on the host: the native reader and the frame stream need no GPU. Dumps of 7 atoms
(two molecule types: 2 x 2 atoms, 1 x 3 atoms), 5 frames, one frame per file, rows shuffled; every comparison is by
equality.
"""
import gzip
import os
import shutil

import numpy as np
import pytest

from mdproptools_amd import io as mio
from mdproptools_amd.common import trajectory as T
from mdproptools_amd.common.com_mols import atom_masses

N, NUM_MOLS, ATOMS_PER_MOL = 7, [2, 1], [2, 3]
TYPES = np.array([1, 2, 1, 2, 3, 4, 4])
MASS = [12.0, 1.0, 16.0, 2.0]
BOUNDS = [(-1.5, 8.25), (0.5, 9.0), (2.0, 13.0)]  # non-zero lo on every axis
FILE_NO = [2, 9, 10, 11, 100]      # numeric order is not the lexicographic one ...
STEPS = [300, 0, 200, 100, 400]    # ... and not the time order either
WRAPPED_COLS = ["id", "type", "q", "mass", "x", "y", "z", "ix", "iy", "iz"]
UNWRAPPED_COLS = ["id", "type", "q", "mass", "xu", "yu", "zu"]


def _tables(seed=0, n=N):
    rng = np.random.default_rng(seed)
    out = []
    for _ in FILE_NO:
        ids = np.arange(1, n + 1)
        lo, hi = np.array(BOUNDS).T
        xyz = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
        img = rng.integers(-2, 3, (n, 3))
        out.append({"id": ids, "type": TYPES[:n], "q": rng.uniform(-1, 1, n), "mass": np.array(MASS)[TYPES[:n] - 1],
                    "x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "ix": img[:, 0], "iy": img[:, 1], "iz": img[:, 2],
                    "xu": xyz[:, 0] + 3.0, "yu": xyz[:, 1] - 7.0, "zu": xyz[:, 2] * 2.0})
    return out


def _write(path, columns, tables=None, sizes=None):
    rng = np.random.default_rng(9)
    tables = tables or _tables()
    for k, (no, ts) in enumerate(zip(FILE_NO, STEPS)):
        n = N if sizes is None else sizes[k]
        tbl = np.column_stack([tables[k][c][:n] for c in columns])[rng.permutation(n)]
        mio.write_dump(os.path.join(str(path), "dump.%d.dump" % no), ts, BOUNDS, columns, tbl)
    return os.path.join(str(path), "dump.*.dump")


@pytest.fixture(scope="module")
def wrapped(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("wrapped"), WRAPPED_COLS)


@pytest.fixture(scope="module")
def unwrapped(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("unwrapped"), UNWRAPPED_COLS)


# ---- streamable_files ------------------------------------------------------------------------------------------------

def test_streamable_files(unwrapped, tmp_path):
    want = [unwrapped.replace("*", str(no)) for no in FILE_NO]
    assert T.streamable_files(unwrapped, ("id", "q", "mass", "xu", "yu", "zu")) == want
    assert T.streamable_files(unwrapped, ("id", "xu"), files=want[1:3]) == want[1:3]
    assert T.streamable_files(unwrapped, ("id", "q", "mass", "vx")) is None  # a missing column: no error from here
    assert T.streamable_files(str(tmp_path / "nothing.*.dump"), ("id",)) is None
    assert T.streamable_files(unwrapped, ("id",), files=[]) is None
    packed = str(tmp_path / "dump.3.dump.gz")
    with open(want[0], "rb") as src, gzip.open(packed, "wb") as dst:
        shutil.copyfileobj(src, dst)
    assert T.streamable_files(unwrapped, ("id",), files=want + [packed]) is None


# ---- unwrap, unwrapped_columns ---------------------------------------------------------------------------------------

def test_unwrap_is_x_plus_image_times_length_in_that_order():
    t = _tables()[0]
    cols = {c: t[c].astype(np.float64) for c in ("id", "x", "y", "z", "ix", "iy", "iz")}
    bounds = np.array(BOUNDS)
    got = T.unwrap(dict(cols), bounds)
    for k, axis in enumerate("xyz"):
        want = cols[axis] + cols["i" + axis] * (BOUNDS[k][1] - BOUNDS[k][0])
        assert got[axis + "u"].tobytes() == want.tobytes()
    assert got["x"] is cols["x"] and got["id"] is cols["id"]


def test_unwrap_leaves_dumped_unwrapped_coordinates_alone():
    t = _tables()[0]
    cols = {c: t[c].astype(np.float64) for c in ("id", "xu", "yu", "zu")}
    got = T.unwrap(dict(cols), np.array(BOUNDS))
    assert list(got) == list(cols) and all(got[c] is cols[c] for c in cols)


def test_unwrapped_columns_selection_and_the_callers_raise():
    calls = []

    def missing(c, have):
        calls.append((c, have))

    assert T.unwrapped_columns(UNWRAPPED_COLS, ["q", "mass"], missing) == ["q", "mass", "xu", "yu", "zu"]
    assert T.unwrapped_columns(WRAPPED_COLS, ["id"], missing) == ["id", "x", "y", "z", "ix", "iy", "iz"]
    assert calls == []
    no_iy = [c for c in WRAPPED_COLS if c != "iy"]
    assert T.unwrapped_columns(no_iy, [], missing) == ["x", "y", "z", "ix", "iy", "iz"]
    assert calls == [("iy", False)]
    # the reference's quirk, kept by Diffusion: only zu decides; a lacking companion is reported as such
    calls.clear()
    assert T.unwrapped_columns(["id", "zu", "x", "y", "z"], ["id"], missing, decide_on=("zu",)) == ["id", "xu", "yu", "zu"]
    assert calls == [("xu", True), ("yu", True)]
    calls.clear()
    assert T.unwrapped_columns(["id", "xu", "yu"] + list(T.WRAPPED), [], missing) == list(T.WRAPPED)
    assert calls == []


def test_no_coordinates_at_all_raises_each_callers_own_error(tmp_path):
    """The texts are the parent commit's, copied as literals; both callers raise them from the callback they hand to
    `attribute_batches`, before anything is asked of a GPU."""
    from mdproptools_amd.dynamical.conductivity import Conductivity
    from mdproptools_amd.dynamical.diffusion import Diffusion

    _write(tmp_path, ["id", "type", "q", "mass"])
    d = Diffusion(outputs_dir=str(tmp_path), diff_dir=str(tmp_path))
    with pytest.raises(AssertionError) as e:
        d.get_msd_from_dump("dump.*.dump", msd_type="com", num_mols=NUM_MOLS, num_atoms_per_mol=ATOMS_PER_MOL)
    assert str(e.value) == "Missing wrapped and unwrapped coordinates (x y z xu yu zu)"
    c = Conductivity("dump.*.dump", NUM_MOLS, ATOMS_PER_MOL, 1000.0, working_dir=str(tmp_path))
    with pytest.raises(ValueError) as e:
        c.einstein()
    assert str(e.value) == "Missing column 'x' in dump file (no xu yu zu to use instead)."
    # z without the image flags: Diffusion's second text; Conductivity names the first column it lacks
    sub = tmp_path / "no_images"
    sub.mkdir()
    _write(sub, ["id", "type", "q", "mass", "x", "y", "z"])
    with pytest.raises(AssertionError) as e:
        Diffusion(outputs_dir=str(sub), diff_dir=str(sub)).get_msd_from_dump("dump.*.dump", msd_type="allatom")
    assert str(e.value) == ("Missing unwrapped coordinates (xu yu zu) and box location (ix iy iz) for converting "
                            "wrapped coordinates (x y z) into unwrapped coordinates. ")
    with pytest.raises(ValueError) as e:
        Conductivity("dump.*.dump", NUM_MOLS, ATOMS_PER_MOL, 1000.0, working_dir=str(sub)).nernst()
    assert str(e.value) == "Missing column 'ix' in dump file (no xu yu zu to use instead)."


def test_adapters_unwrap_wrapped_dumps_like_dumped_unwrapped_ones(wrapped):
    """`attribute_batches` as Diffusion calls it, on the native route: xu yu zu of a wrapped dump are x + ix * L of its
    id-sorted rows, every frame in one batch of the general route."""
    tables = _tables()
    streamed, batches = T.attribute_batches(wrapped, ("id", "type"), T.UNWRAPPED, n_atoms=N, decide_on=("zu",))
    ((steps, ids, types, planes),) = batches
    assert not streamed and steps.tolist() == STEPS and planes.shape == (5, 3, N)
    assert np.array_equal(ids, np.tile(np.arange(1.0, N + 1), (5, 1))) and np.array_equal(types, np.tile(TYPES, (5, 1)))
    for f, t in enumerate(tables):
        for k, axis in enumerate("xyz"):
            want = t[axis] + t["i" + axis].astype(np.float64) * (BOUNDS[k][1] - BOUNDS[k][0])
            assert planes[f, k].tobytes() == want.tobytes()


# ---- masses ----------------------------------------------------------------------------------------------------------

def test_masses_by_list_and_by_column():
    import pandas as pd

    types = TYPES.astype(np.float64)
    column = np.array(MASS)[TYPES - 1] * 1.5
    by_list = T.masses(types, MASS)
    assert by_list is not types and np.array_equal(by_list, np.array(MASS)[TYPES - 1]) and by_list.dtype == np.float64
    for falsy in (None, [], ()):
        assert T.masses(column, falsy) is column  # the column itself, as the load-everything routes always took it
    both = np.stack([types, types[::-1]])  # a batch [B, N], as the streamed Diffusion route hands it over
    assert np.array_equal(T.masses(both, MASS), np.array(MASS)[both.astype(np.int64) - 1])
    data = pd.DataFrame({"type": TYPES, "mass": column})
    assert np.array_equal(atom_masses(data, MASS), by_list) and np.array_equal(atom_masses(data, None), column)
    with pytest.raises(AssertionError) as e:
        atom_masses(data[["type"]], None)
    assert str(e.value) == "Missing atom masses in dump file."


# ---- frame_batches ---------------------------------------------------------------------------------------------------

COLS = ["id", "type", "x", "z"]
FRAME_BYTES = len(COLS) * N * 8


def _gather(batches):
    batches = list(batches)
    return ([len(b[0]) for b in batches], [ts for b in batches for ts in b[0]],
            np.concatenate([b[1] for b in batches]), np.concatenate([b[2] for b in batches]))


def test_frame_batches_cuts_show_in_no_value(wrapped):
    sizes, steps, lengths, planes = _gather(T.frame_batches(wrapped, COLS, float("inf")))
    assert sizes == [5] and steps == STEPS  # numeric file order, not time order, not lexicographic
    assert planes.shape == (5, 4, N) and lengths.shape == (5, 3)
    assert np.array_equal(lengths, np.tile([hi - lo for lo, hi in BOUNDS], (5, 1)))
    for f, t in enumerate(_tables()):  # atoms by id
        assert np.array_equal(planes[f], np.stack([t[c].astype(np.float64) for c in COLS]))
    for cap, want_sizes in ((FRAME_BYTES, [1] * 5), (2 * FRAME_BYTES, [2, 2, 1]), (3 * FRAME_BYTES - 1, [2, 2, 1]),
                            (1, [1] * 5), (1 << 62, [5])):
        s, st, le, pl = _gather(T.frame_batches(wrapped, COLS, cap))
        assert s == want_sizes and st == steps
        assert le.tobytes() == lengths.tobytes() and pl.tobytes() == planes.tobytes()
    # an explicit share of the files takes the place of the pattern
    files = T.streamable_files(wrapped, COLS)
    s, st, le, pl = _gather(T.frame_batches(wrapped, COLS, float("inf"), files=files[3:]))
    assert st == STEPS[3:] and pl.tobytes() == planes[3:].tobytes()


def test_frame_batches_new_batch_at_another_atom_count_and_the_count_check(wrapped, tmp_path):
    pattern = _write(tmp_path, WRAPPED_COLS, sizes=[7, 7, 6, 6, 7])
    got = list(T.frame_batches(pattern, COLS, float("inf")))
    assert [b[2].shape for b in got] == [(2, 4, 7), (2, 4, 6), (1, 4, 7)]
    assert [b[0] for b in got] == [STEPS[:2], STEPS[2:4], STEPS[4:]]
    assert len(list(T.frame_batches(wrapped, COLS, float("inf"), n_atoms=N))) == 1
    with pytest.raises(ValueError) as e:
        list(T.frame_batches(wrapped, COLS, float("inf"), n_atoms=8))
    assert str(e.value) == "Length of values (8) does not match length of index (7)"
    with pytest.raises(ValueError) as e:
        list(T.frame_batches(pattern, COLS, float("inf"), n_atoms=7))  # raised at the third frame
    assert str(e.value) == "Length of values (7) does not match length of index (6)"


# ---- stream_reduced --------------------------------------------------------------------------------------------------

def test_stream_reduced_hands_out_the_same_frames(unwrapped):
    cols = ("q", "mass", "xu", "yu", "zu")
    _, steps, _, planes = _gather(T.frame_batches(unwrapped, list(cols), float("inf")))
    files = T.streamable_files(unwrapped, ("id",) + cols)
    got_steps, got = [], []
    n_batches = 0
    for batch in T.stream_reduced(unwrapped, files, cols, N, batch_bytes=2 * 24 * N):
        assert len(batch) <= 2
        n_batches += 1
        got_steps += batch.timesteps.tolist()
        got.append(np.concatenate([batch.ids[:, None], batch.types[:, None], batch.xyz], axis=1))  # (copies)
    assert n_batches == 3 and got_steps == steps
    assert np.concatenate(got).tobytes() == planes.tobytes()
    with pytest.raises(ValueError) as e:
        list(T.stream_reduced(unwrapped, files, cols, 9))
    assert str(e.value) == "Length of values (9) does not match length of index (7)"
    assert len(list(T.stream_reduced(unwrapped, files, cols, None))) >= 1  # None: not checked


# ---- same_labels -----------------------------------------------------------------------------------------------------

def test_same_labels():
    a = TYPES.astype(np.float64)
    one = T.same_labels([a, a.copy(), a.copy()])
    assert one.shape == (N,) and np.array_equal(one, a)
    assert T.same_labels(np.stack([a, a])).shape == (N,)
    b = a.copy()
    b[3] = 9.0
    two = T.same_labels([a, a, b])
    assert two.shape == (3, N) and np.array_equal(two, np.stack([a, a, b]))
    assert T.same_labels([a]).shape == (N,)


def test_load_frames_reports_frames_to_on_frame_only(tmp_path, capsys):
    """The whole-frame loader prints nothing itself, whatever a module's VERBOSE says: the progress line is the caller's
    `on_frame`, called once per frame in frame order (list route; the stream calls it from its reader)."""
    from mdproptools_amd import io as mio
    from mdproptools_amd.structural import rdf_cn

    rng = np.random.default_rng(2)
    for step in (0, 300, 20):
        tbl = np.column_stack([rng.permutation(6) + 1, np.ones(6), rng.uniform(0, 5, (6, 3))])
        mio.write_dump(str(tmp_path / ("d.%d.dump" % step)), step, [[0, 5.0]] * 3, ["id", "type", "x", "y", "z"], tbl)
    rdf_cn.VERBOSE = True
    try:
        frames = T.load_frames(str(tmp_path / "d.*.dump"))
        assert capsys.readouterr().out == ""
        seen = []
        again = T.load_frames(str(tmp_path / "d.*.dump"), on_frame=seen.append)
    finally:
        rdf_cn.VERBOSE = False
    assert seen == [0, 20, 300] == [f.timestep for f in frames] == [f.timestep for f in again]
    assert [len(b) for b in T.batches(frames, 2 * 24 * 6)] == [2, 1] and frames[0].ids.tolist() == [1, 2, 3, 4, 5, 6]
