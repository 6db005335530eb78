"""
CPU-only: the six public functions of structural/rdf_cn.py end to end — text dumps in, DataFrames and CSV files out —
with the C oracle standing in for the six backend calls they make. Four parts: the reference's goldens on the two
mg_tfsi_dme frames, every ingest route and batch size on a small NPT trajectory, types that change inside a batch,
and a record of every backend call (name, shapes, dtypes, bytes) that two commits can be compared by:

    python tests/test_rdf_cn_dropin_cpu.py dump    calls.npz     # at one commit
    python tests/test_rdf_cn_dropin_cpu.py compare calls.npz     # at the other
"""
import hashlib
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from test_dist_gloo import _dropin_case

MASS = [16.000, 12.010, 1.008, 14.010, 32.060, 16.000, 12.010, 19.000, 24.305]  # of the mg_tfsi_dme frames' nine types
BACKEND_NAMES = ("rdf_loop", "cn_loop", "rdf_cn_loop", "rdf_mol_loop", "cn_mol_loop", "segment_com")
_MEMO = {}  # a stand-in's result by the bytes of its arguments: the C1 sweeps cost a second per frame


def _signatures():
    from mdproptools_amd import backend

    return {name: inspect.signature(getattr(backend, name)) for name in BACKEND_NAMES}


_SIGNATURES = _signatures()  # of the real functions, before any test replaces them


def _cached(fn):
    def call(*args):
        h = hashlib.blake2b(fn.__name__.encode())
        for a in args:
            a = np.ascontiguousarray(a)
            h.update(str((a.shape, a.dtype)).encode() + a.tobytes())
        key = h.digest()
        if key not in _MEMO:
            _MEMO[key] = fn(*args)
        return _MEMO[key]

    return call


def _oracle_backend():
    """{name: stand-in} for the six functions of mdproptools_amd.backend that rdf_cn.py calls, same signatures, the C
    oracle (pair loops) and the numpy restatement of calc_com (segment sums) behind them."""
    from oracle import cpu_ref, cref

    def per_type(types, f):
        return types if np.ndim(types) == 1 else types[f]

    rdf_pairs, cn_pairs = _cached(cref.rdf_pairs), _cached(cref.cn_pairs)
    rdf_rect, cn_rect = _cached(cref.rdf_rect), _cached(cref.cn_rect)

    def rdf_loop(xyz, types, box, rel, r_cut, ddr, nbins, per_frame=True):
        res = [rdf_pairs(xyz[f], per_type(types, f), rel, box[f], float(r_cut) ** 2, ddr, nbins) for f in range(len(xyz))]
        return np.stack([q[0] for q in res]), np.stack([q[1] for q in res]), sum(q[2] for q in res)

    def cn_loop(xyz, types, box, rel, cuts, per_frame=True):
        return np.stack([cn_pairs(xyz[f], per_type(types, f), rel, box[f], [float(c) ** 2 for c in cuts])
                         for f in range(len(xyz))])

    def rdf_cn_loop(xyz, types, box, rel, r_cut, ddr, nbins, cuts, per_frame=True):
        return rdf_loop(xyz, types, box, rel, r_cut, ddr, nbins) + (cn_loop(xyz, types, box, rel, cuts),)

    def rdf_mol_loop(xyz, types, sites, site_types, box, rel, r_cut, ddr, nbins, per_frame=True):
        assert np.ndim(types) == 1 and len(xyz) == len(sites) == len(box)
        res = [rdf_rect(xyz[f], types, sites[f], site_types, rel, box[f], float(r_cut) ** 2, ddr, nbins)
               for f in range(len(xyz))]
        return np.stack([q[0] for q in res]), sum(q[1] for q in res)

    def cn_mol_loop(xyz, types, sites, site_types, box, rel, cuts, per_frame=True):
        assert np.ndim(types) == 1 and len(xyz) == len(sites) == len(box)
        return np.stack([cn_rect(xyz[f], types, sites[f], site_types, rel, box[f], [float(c) ** 2 for c in cuts])
                         for f in range(len(xyz))])

    def segment_com(attr, atom_mass, seg_off):
        mass, off = np.asarray(atom_mass, dtype=np.float64), np.asarray(seg_off, dtype=np.int64)
        res = [cpu_ref.calc_com(np.asarray(a).T, mass, off) for a in attr]
        return np.stack([q[0].T for q in res]), res[0][1], None

    fns = (rdf_loop, cn_loop, rdf_cn_loop, rdf_mol_loop, cn_mol_loop, segment_com)
    return dict(zip(BACKEND_NAMES, fns))


def _install(monkeypatch, log=None):
    """Puts the stand-ins into mdproptools_amd.backend; with `log` (a list) every call is appended to it first, as
    (name, [copies of its arguments as arrays]): the arguments as the real function's signature binds them, defaults
    filled in and the ones left at None (ctx, out, ...) omitted — copies, because a streamed batch's buffer is reused."""
    from mdproptools_amd import backend

    for name, fn in _oracle_backend().items():
        def recorded(*args, _name=name, _fn=fn, _sig=_SIGNATURES[name], **kw):
            if log is not None:
                bound = _sig.bind(*args, **kw)
                bound.apply_defaults()
                log.append((_name, [np.array(v) for v in bound.arguments.values() if v is not None]))
            return _fn(*args, **kw)

        monkeypatch.setattr(backend, name, recorded)


def _frames_per_call(log):
    """{backend function: tuple of the frame counts of its calls, in call order}."""
    out = {}
    for name, args in log:
        out.setdefault(name, []).append(len(args[0]))
    return {k: tuple(v) for k, v in out.items()}


def _same_frame(a, b):
    assert list(a.columns) == list(b.columns)
    np.testing.assert_array_equal(a.to_numpy(), b.to_numpy())


# ------------------------------------------------------------------------------------ the reference's goldens
@pytest.fixture(scope="module")
def c1_dir(tmp_path_factory):
    from mdproptools_amd import io as mio

    g = load_golden("c1_rdf.npz")
    tmp = str(tmp_path_factory.mktemp("c1"))
    for s, b, t in zip(g["steps"], g["bounds"], g["frames"]):
        mio.write_dump(os.path.join(tmp, "dump.nvt.%d.dump" % s), s, b, list(g["columns"]), t)
    return g, os.path.join(tmp, "dump.nvt.*.dump"), tmp


def test_atomic_rdf_and_cn_are_the_reference_frames_bit_for_bit(c1_dir, monkeypatch):
    """What tests/test_gpu_dropin.py::test_calc_atomic_rdf_and_cn asserts, without a GPU."""
    import pandas as pd

    from mdproptools_amd.structural.rdf_cn import calc_atomic_cn, calc_atomic_rdf

    _install(monkeypatch)
    g, pat, tmp = c1_dir
    alt = dict(num_mols=g["num_mols"].tolist(), num_atoms_per_mol=g["num_atoms_per_mol"].tolist())
    out = os.path.join(tmp, "rdf.csv")
    df = calc_atomic_rdf(20, 0.05, 9, MASS, g["rdf_def_rel"].tolist(), pat, path_or_buff=out)
    assert list(df.columns) == list(g["rdf_def_df_columns"])
    np.testing.assert_array_equal(df.to_numpy(), g["rdf_def_df"])
    np.testing.assert_allclose(pd.read_csv(out).to_numpy(), g["rdf_def_df"], rtol=1e-13)
    df = calc_atomic_rdf(20, 0.05, 9, MASS, g["rdf_alt_rel"].tolist(), pat, save_mode=False, **alt)
    np.testing.assert_array_equal(df.to_numpy(), g["rdf_alt_df"])
    assert list(df.columns)[2:] == ["g_32-17", "g_32-32"]
    cn = calc_atomic_cn(g["cn_def_cut"].tolist(), 0.05, 9, MASS, g["cn_def_rel"].tolist(), pat, save_mode=False)
    np.testing.assert_array_equal(cn.to_numpy(), g["cn_def_df"])
    assert list(cn.columns) == ["cn_9-1", "cn_9-4", "cn_9-6", "cn_9-9"]
    cn = calc_atomic_cn(g["cn_alt_cut"].tolist(), 0.05, 9, MASS, g["rdf_alt_rel"].tolist(), pat, save_mode=False, **alt)
    np.testing.assert_array_equal(cn.to_numpy(), g["cn_alt_df"])
    assert list(cn.columns) == ["cn_32-17", "cn_32-32"]
    with pytest.raises(ValueError):
        calc_atomic_rdf(20, 0.05, 8, MASS[:8], [[9], [1]], pat, save_mode=False)  # wrong num_types


def test_molecular_and_intermolecular_are_the_reference_frames(c1_dir, monkeypatch):
    """test_calc_molecular_rdf_and_cn and test_calc_intermolecular_rdf of tests/test_gpu_dropin.py, at their tolerance
    (the centres of mass are summed in another order than the reference's, here as on the GPU)."""
    from mdproptools_amd.structural.rdf_cn import calc_intermolecular_rdf, calc_molecular_cn, calc_molecular_rdf

    _install(monkeypatch)
    g, pat, tmp = c1_dir
    nm, na = g["num_mols"].tolist(), g["num_atoms_per_mol"].tolist()
    df = calc_molecular_rdf(20, 0.05, 9, MASS, g["mol_rel"].tolist(), pat, nm, na, save_mode=False)
    np.testing.assert_allclose(df.to_numpy(), g["mol_rdf_df"], rtol=1e-12, atol=0)
    assert list(df.columns) == ["r ($\\AA$)", "g_9-1", "g_9-2", "g_4-3"]
    cn = calc_molecular_cn(g["mol_cn_cut"].tolist(), 0.05, 9, MASS, g["mol_rel"].tolist(), pat, nm, na, save_mode=False)
    np.testing.assert_allclose(cn.to_numpy(), g["mol_cn_df"], rtol=1e-12, atol=0)
    assert list(cn.columns) == ["cn_9-1", "cn_9-2", "cn_4-3"]
    ref = load_golden("inter_rdf.npz")
    df = calc_intermolecular_rdf(20, 0.05, 3, MASS, ref["rel"].tolist(), pat, nm, na, save_mode=False)
    assert list(df.columns) == [str(c) for c in ref["columns"]]
    np.testing.assert_allclose(df.to_numpy(), ref["df"], rtol=1e-12, atol=0)


def test_one_pass_is_the_two_separate_calls_bit_for_bit(c1_dir, tmp_path, monkeypatch):
    """tests/test_gpu_dropin.py::test_calc_atomic_rdf_cn_one_pass: DataFrames bit for bit, CSV files byte for byte."""
    from mdproptools_amd.structural.rdf_cn import calc_atomic_cn, calc_atomic_rdf, calc_atomic_rdf_cn

    _install(monkeypatch)
    g, pat, tmp = c1_dir
    rel = [[9, 9, 9, 9, 1], [1, 4, 6, 9, 3]]
    cuts = [2.3, 2.3, 3.1, 6.0, 1.5]
    for kw in ({}, dict(num_mols=g["num_mols"].tolist(), num_atoms_per_mol=g["num_atoms_per_mol"].tolist())):
        r = rel if not kw else [[32, 32], [17, 32]]
        c = cuts if not kw else [2.4, 5.5]
        a = calc_atomic_rdf(20, 0.05, 9, MASS, r, pat, path_or_buff=str(tmp_path / "a.csv"), **kw)
        b = calc_atomic_cn(c, 0.05, 9, MASS, r, pat, path_or_buff=str(tmp_path / "b.csv"), **kw)
        g2, c2 = calc_atomic_rdf_cn(20, c, 0.05, 9, MASS, r, pat, rdf_path_or_buff=str(tmp_path / "g.csv"),
                                    cn_path_or_buff=str(tmp_path / "c.csv"), **kw)
        _same_frame(g2, a)
        _same_frame(c2, b)
        assert open(tmp_path / "g.csv", "rb").read() == open(tmp_path / "a.csv", "rb").read()
        assert open(tmp_path / "c.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    with pytest.raises(ValueError, match="one coordination cutoff per relation is required"):
        calc_atomic_rdf_cn(20, cuts[:2], 0.05, 9, MASS, rel, pat, save_mode=False)


# ------------------------------------------------------------------------------------ routes and batch sizes
N_ROUTES, ROUTES_MOLS, ROUTES_ATOMS = 240, [40, 24], [3, 5]  # the NPT case of test_dist_gloo: 5 files, a growing box
ROUTES_MASS = [1.0, 2.0, 3.0]


def _six(pattern, out_dir):
    """Every public function once (calc_atomic_rdf with plain and with altered ids) -> {name: DataFrame}; the CSV files
    go to out_dir under the same names."""
    from mdproptools_amd.structural import rdf_cn as R

    os.makedirs(out_dir, exist_ok=True)
    csv = lambda name: os.path.join(out_dir, name + ".csv")  # noqa: E731
    rel, cuts = [[1, 1, 2], [1, 2, 3]], [2.0, 3.0, 4.5]
    mol_rel, alt_rel = [[1, 2, 3], [1, 2, 2]], [[1, 4, 8], [2, 4, 5]]
    nm, na, mass = ROUTES_MOLS, ROUTES_ATOMS, ROUTES_MASS
    res = {
        "rdf": R.calc_atomic_rdf(5.0, 0.1, 3, mass, rel, pattern, path_or_buff=csv("rdf")),
        "rdf_alt": R.calc_atomic_rdf(5.0, 0.1, 3, mass, alt_rel, pattern, nm, na, path_or_buff=csv("rdf_alt")),
        "cn": R.calc_atomic_cn(cuts, 0.1, 3, mass, rel, pattern, path_or_buff=csv("cn")),
        "mol_rdf": R.calc_molecular_rdf(5.0, 0.1, 3, mass, mol_rel, pattern, nm, na, path_or_buff=csv("mol_rdf")),
        "mol_cn": R.calc_molecular_cn(cuts, 0.1, 3, mass, mol_rel, pattern, nm, na, path_or_buff=csv("mol_cn")),
        "inter": R.calc_intermolecular_rdf(6.0, 0.1, 2, mass, [[1, 1, 2], [1, 2, 2]], pattern, nm, na,
                                           path_or_buff=csv("inter")),
    }
    res["one_rdf"], res["one_cn"] = R.calc_atomic_rdf_cn(5.0, cuts, 0.1, 3, mass, rel, pattern,
                                                         rdf_path_or_buff=csv("one_rdf"), cn_path_or_buff=csv("one_cn"))
    return res


ROUTES = [(True, 1 << 30)] + [(False, frames * 24 * N_ROUTES) for frames in (1, 2, 5)]


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{(STREAM, MAX_BATCH_BYTES): ({name: DataFrame}, directory of the CSV files, call log)} of the NPT case."""
    from mdproptools_amd.structural import rdf_cn as R

    tmp = str(tmp_path_factory.mktemp("routes"))
    pattern = _dropin_case(tmp, 5)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for k, (stream, cap) in enumerate(ROUTES):
            log = []
            _install(mp, log)
            mp.setattr(R, "STREAM", stream)
            mp.setattr(R, "MAX_BATCH_BYTES", cap)
            d = os.path.join(tmp, "out%d" % k)
            out[(stream, cap)] = (_six(pattern, d), d, log)
    return out


def test_every_route_and_batch_size_gives_the_same_frames_and_files(routes):
    """STREAM on and off, and MAX_BATCH_BYTES of one frame, two frames and everything: identical DataFrames and CSV
    bytes from all six functions; the one-pass function equals the two separate ones on every route."""
    base, base_dir, _ = routes[ROUTES[-1]]
    assert abs(base["rdf"]["g_full(r)"].to_numpy()[20:].mean() - 1.0) < 0.2  # an ideal gas, and not all zeros
    assert (base["mol_cn"].to_numpy() > 0).all() and (base["inter"].to_numpy()[:, 1:].sum(axis=0) > 0).all()
    for key in ROUTES:
        res, d, _ = routes[key]
        for name, df in res.items():
            _same_frame(df, base[name])
            assert open(os.path.join(d, name + ".csv"), "rb").read() == \
                open(os.path.join(base_dir, name + ".csv"), "rb").read(), (key, name)
        _same_frame(res["one_rdf"], res["rdf"])
        _same_frame(res["one_cn"], res["cn"])


def test_batches_hold_the_frames_the_cap_allows(routes):
    """Load-all route: one backend call per batch of MAX_BATCH_BYTES. The types of this case differ from file to file,
    so the molecular calls (one per run of equal types) take one frame each."""
    for frames, want in ((1, (1, 1, 1, 1, 1)), (2, (2, 2, 1)), (5, (5,))):
        got = _frames_per_call(routes[(False, frames * 24 * N_ROUTES)][2])
        assert got["rdf_loop"] == want * 2 and got["cn_loop"] == want and got["rdf_cn_loop"] == want
        assert got["cn_mol_loop"] == (1,) * 5
        assert got["rdf_mol_loop"] == (1,) * 5 + want  # calc_molecular_rdf, then calc_intermolecular_rdf (no types)


def test_a_pattern_without_frames(tmp_path, monkeypatch):
    """No file matches: no backend call, and the mean over zero frames — a DataFrame of NaN under the usual columns
    (numpy warns of the division) — is returned and written."""
    from mdproptools_amd.structural import rdf_cn as R

    log = []
    _install(monkeypatch, log)
    for stream in (True, False):
        monkeypatch.setattr(R, "STREAM", stream)
        with pytest.warns(RuntimeWarning):
            df = R.calc_atomic_rdf(5.0, 0.1, 3, ROUTES_MASS, [[1], [2]], str(tmp_path / "none.*.dump"),
                                   path_or_buff=str(tmp_path / "rdf.csv"))
        with pytest.warns(RuntimeWarning):
            cn = R.calc_molecular_cn([2.0], 0.1, 3, ROUTES_MASS, [[1], [2]], str(tmp_path / "none.*.dump"),
                                     ROUTES_MOLS, ROUTES_ATOMS, save_mode=False)
        assert list(df.columns) == [R._R_LABEL, "g_full(r)", "g_1-2"] and df.shape == (50, 3)
        assert np.isnan(df.to_numpy()[:, 1:]).all() and np.isnan(cn.to_numpy()).all() and cn.shape == (1, 1)
        assert open(tmp_path / "rdf.csv").readline() == "r ($\\AA$),g_full(r),g_1-2\n"
    assert log == []


def test_progress_lines_and_their_order(tmp_path, monkeypatch, capsys):
    """VERBOSE, load-all route, two frames per batch: the lines of calc_atomic_rdf and calc_molecular_cn in order."""
    from mdproptools_amd.structural import rdf_cn as R

    _install(monkeypatch)
    pattern = _dropin_case(str(tmp_path), 3)
    monkeypatch.setattr(R, "VERBOSE", True)
    monkeypatch.setattr(R, "STREAM", False)
    monkeypatch.setattr(R, "MAX_BATCH_BYTES", 2 * 24 * N_ROUTES)
    R.calc_atomic_rdf(5.0, 0.1, 3, ROUTES_MASS, [[1], [2]], pattern, path_or_buff=str(tmp_path / "rdf.csv"))
    lines = [ln.split("=")[0].split(" took")[0].rstrip(" 0123456789") for ln in capsys.readouterr().out.splitlines()]
    step, rho, done = "The timestep of the current file is:", "Average density", "Finished computing RDF for timestep"
    assert lines == [step] * 3 + [rho, rho, done, done, "Trajectory loop", rho, done, "Trajectory loop",
                                  "Results are written to pd.DataFrame and csv file"]
    R.calc_molecular_cn([2.0], 0.1, 3, ROUTES_MASS, [[1], [2]], pattern, ROUTES_MOLS, ROUTES_ATOMS, save_mode=False)
    lines = capsys.readouterr().out.splitlines()
    done = "Finished computing CN for timestep %d"
    assert [ln.split("=")[0] for ln in lines[:10]] == [step + " 0", step + " 100", step + " 200", rho, rho, done % 0,
                                                       done % 100, rho, done % 200, "   cn_1-2"]


# ------------------------------------------------------------------------------------ types that change inside a batch
RUNS_MOLS, RUNS_ATOMS = [20, 30], [3, 5]


def type_runs_case(tmp_dir):
    """Four one-frame files of 210 atoms (20 molecules of 3 atoms, 30 of 5) in a growing box; the atoms carry other types
    in files 3 and 4 than in files 1 and 2. Returns (pattern, [the four files])."""
    from mdproptools_amd import io as mio

    rng = np.random.default_rng(21)
    n = 210
    types = [1 + (np.arange(n) % 3), 1 + ((np.arange(n) // 2) % 3)]
    paths = []
    for k in range(4):
        L = 12.0 + 0.25 * k
        perm = rng.permutation(n)  # rows in another order in every file; an atom's type goes with its id
        tbl = np.column_stack([perm + 1, types[k // 2][perm], rng.uniform(0, L, (n, 3))])
        paths.append(os.path.join(tmp_dir, "dump.npt.%d.dump" % (k * 50)))
        mio.write_dump(paths[-1], k * 50, [[0, L]] * 3, ["id", "type", "x", "y", "z"], tbl)
    return os.path.join(tmp_dir, "dump.npt.*.dump"), paths


def check_type_runs(tmp_dir):
    """calc_molecular_rdf and calc_molecular_cn over the four files == the frame-order sum of the four single-file
    calls divided by 4, bit for bit (the backend in place decides what computes them)."""
    from mdproptools_amd.structural import rdf_cn as R

    pattern, paths = type_runs_case(tmp_dir)
    rel, mass = [[1, 2, 3, 3], [1, 1, 2, 1]], [12.0, 1.0, 16.0]
    calls = {
        "rdf": lambda fn: R.calc_molecular_rdf(5.5, 0.1, 3, mass, rel, fn, RUNS_MOLS, RUNS_ATOMS, save_mode=False),
        "cn": lambda fn: R.calc_molecular_cn([2.5, 3.0, 4.0, 5.5], 0.1, 3, mass, rel, fn, RUNS_MOLS, RUNS_ATOMS,
                                             save_mode=False),
    }
    for name, call in calls.items():
        whole = call(pattern)
        acc = np.zeros(whole.shape)
        for p in paths:
            acc += call(p).to_numpy()
        want = acc / 4
        if name == "rdf":  # (the radii column is no mean)
            want[:, 0] = whole.to_numpy()[:, 0]
        assert want[:, -1].sum() > 0
        np.testing.assert_array_equal(whole.to_numpy(), want)


@pytest.mark.parametrize("stream", [True, False])
def test_types_that_change_inside_a_batch(tmp_path, monkeypatch, stream):
    from mdproptools_amd.structural import rdf_cn as R

    _install(monkeypatch)
    monkeypatch.setattr(R, "STREAM", stream)
    check_type_runs(str(tmp_path))


@pytest.mark.parametrize("stream", [True, False])
def test_a_run_of_equal_types_is_one_backend_call(tmp_path, monkeypatch, stream):
    """The four frames above are two runs of two: one segment_com and one pair call per run, on either route. (Before the
    type runs, a batch whose types changed anywhere went through the backend frame by frame: four calls of one frame.)"""
    from mdproptools_amd.structural import rdf_cn as R

    log = []
    _install(monkeypatch, log)
    monkeypatch.setattr(R, "STREAM", stream)
    pattern, _ = type_runs_case(str(tmp_path))
    rel, mass = [[1, 2, 3, 3], [1, 1, 2, 1]], [12.0, 1.0, 16.0]
    R.calc_molecular_rdf(5.5, 0.1, 3, mass, rel, pattern, RUNS_MOLS, RUNS_ATOMS, save_mode=False)
    assert _frames_per_call(log) == {"segment_com": (2, 2), "rdf_mol_loop": (2, 2)}
    del log[:]
    R.calc_molecular_cn([2.5, 3.0, 4.0, 5.5], 0.1, 3, mass, rel, pattern, RUNS_MOLS, RUNS_ATOMS, save_mode=False)
    assert _frames_per_call(log) == {"segment_com": (2, 2), "cn_mol_loop": (2, 2)}
    del log[:]
    R.calc_intermolecular_rdf(5.5, 0.1, 2, mass, [[1, 2], [2, 2]], pattern, RUNS_MOLS, RUNS_ATOMS, save_mode=False)
    assert _frames_per_call(log) == {"segment_com": (2, 2), "rdf_mol_loop": (4,)}  # (no atom types in that sweep)


# ------------------------------------------------------------------------------------ the record of the backend calls
def record_routes_calls(tmp_dir):
    """{key: array} of every backend call of the routes case on every route: 'r<route>_c<call>_<name>_a<k>' holds
    argument k, and 'r<route>_<function>' / 'r<route>_<function>_csv' the returned frame and the bytes written."""
    from mdproptools_amd.structural import rdf_cn as R

    os.makedirs(tmp_dir, exist_ok=True)
    pattern = _dropin_case(tmp_dir, 5)
    rec = {}
    with pytest.MonkeyPatch.context() as mp:
        for k, (stream, cap) in enumerate(ROUTES):
            log = []
            _install(mp, log)
            mp.setattr(R, "STREAM", stream)
            mp.setattr(R, "MAX_BATCH_BYTES", cap)
            d = os.path.join(tmp_dir, "out%d" % k)
            for name, df in _six(pattern, d).items():
                rec["r%d_%s" % (k, name)] = df.to_numpy()
                rec["r%d_%s_columns" % (k, name)] = np.array(list(df.columns))
                rec["r%d_%s_csv" % (k, name)] = np.frombuffer(open(os.path.join(d, name + ".csv"), "rb").read(), np.uint8)
            for c, (name, args) in enumerate(log):
                for j, a in enumerate(args):
                    rec["r%d_c%03d_%s_a%d" % (k, c, name, j)] = a
    return rec


def compare_records(got, want):
    """Asserts two records equal — keys (so: number, order and names of the calls), dtypes, shapes and bytes — and
    returns (number of backend calls, number of argument arrays) compared."""
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), key
    arrays = [k for k in want if "_c" in k and k.rsplit("_a", 1)[-1].isdigit()]
    return len({k.rsplit("_a", 1)[0] for k in arrays}), len(arrays)


def test_the_call_record_repeats(tmp_path):
    """Two recordings of the same commit are equal: what `compare` reports between two commits is theirs."""
    a = record_routes_calls(str(tmp_path / "a"))
    b = record_routes_calls(str(tmp_path / "b"))
    n_calls, n_arrays = compare_records(a, b)
    assert n_calls >= 4 * 8 and n_arrays > 5 * n_calls


if __name__ == "__main__":
    import tempfile

    mode, path = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        record = record_routes_calls(tmp)
    if mode == "dump":
        np.savez(path, **record)
        print("wrote", len(record), "arrays to", path)
    else:
        print("identical: %d backend calls, %d argument arrays" % compare_records(record, dict(np.load(path))),
              "and %d returned frames / CSV files" % sum(k.endswith("_csv") for k in record))
