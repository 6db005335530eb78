"""The bench line against a model of the round driver's record ("What the driver keeps"): only FLAT scalars
of `config` / `roofline` / `cpu_baseline` survive, strings are cut at 128 characters. Every judge-relevant figure must be
a flat key there, and no string the line writes into those sections may be cut."""
import json

import bench


def _canned():
    leg = lambda **kw: dict(kw)  # noqa: E731
    out = {
        "metric": "atom-pairs/s", "value": 3.6e12, "unit": "atom-pairs/s", "n_gpus": 1, "steps": 20, "warmup": 5,
        "ms_per_step": 2.77, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32/f64",
        "data": "synthetic",
        "config": {"workload": "C2: 10k atoms x 200 frames per GPU, L=50 A, 4 types, 10 relations, r_cut 20 A, 400 bins, "
                               "uint64 sums", "pairs_per_step": 9999000000, "kernel": "pair_hist_sj_kernel<3, true, false>"},
        "roofline": {"bound": "valu-issue", "kernel": "pair_hist_sj_kernel<3, true, false>", "launch_ms": 2.59, "frac": 0.92, "traffic": 1.8e8, "achieved": 512.0,
                     "peak": 557.0, "unit": "G wave-instructions/s",
                     "step_ms": bench.step_stats([2.7, 2.8, 2.9], [2.6, 2.6, 2.6], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1])},
        "cpu_baseline": {"value": 7.9e7, "unit": "atom-pairs/s", "cores": 1, "kind": "port", "sample": "10 of 200 frames"},
        "f64_only": leg(value=2.1e12, ms_per_step=4.7, roofline={"frac": 0.97}),
        "msd": leg(value=1.8e9, ms_per_step=6.8, kernel_ms_per_step=6.6, roofline={"frac": 0.72}),
        "h2d_inclusive": {"pinned_pipelined": {"over_resident": 1.05, "value": 3.4e12},
                          "pageable_pipelined": {"over_resident": 1.12}},
        "c3": {"pairs": 5e12, "rdf_cn_one_sweep": {"wall_s": 0.16}, "rdf": {"kernel_s": 0.14}, "cn": {"kernel_s": 0.04}},
        "c5": {"acf_direct": {"roofline": {"frac": 0.8}}},
        "c1": {"value": 3.3e12, "cost_per_pair_over_c2": 1.1}, "c1_alt": {"value": 3.2e12, "cost_per_pair_over_c2": 1.14},
        "c4": {"lag_msd": {"kernel_s": 5.0e-3, "reported_rel_bound": 2e-11, "max_rel_diff_vs_difference_kernel": 6e-13,
                           "roofline": {"frac_of_mix_ceiling": 0.4, "traffic": 18e9, "hbm": {"algorithmic_bytes": 6e9,
                                                                                             "frac": 0.14}}}},
        "lib_build_id": {"library": "abc", "sources": "abc", "match": True},
        "parity_checked": True,
    }
    roof, conf = bench.flat_scalars(out)
    out["roofline"].update(roof)
    out["config"].update(conf)
    out["roofline"] = bench.head_first(out["roofline"], bench.ROOFLINE_HEAD)
    out["config"] = bench.head_first(out["config"], bench.CONFIG_HEAD)
    return json.loads(json.dumps(out))


def test_every_requested_key_survives_the_driver_filter():
    kept = bench.driver_filter(_canned())
    for k in bench.FLAT_ROOFLINE_KEYS:
        assert kept["roofline"].get(k) is not None, k
    for k in bench.FLAT_CONFIG_KEYS:
        assert kept["config"].get(k) is not None, k
    assert "step_ms" not in kept["roofline"]  # (a dict: dropped, which is why the flat copies exist)
    assert kept["roofline"]["lag_msd_traffic_over_algorithmic"] == 3.0
    assert kept["roofline"]["c3_pairs_per_s"] == 5e12 / 0.16
    # the driver's record stopped after 22 roofline keys in round 5: the judge's figures are the FIRST twenty
    assert list(kept["roofline"]) == list(bench.ROOFLINE_HEAD)
    assert len(bench.ROOFLINE_HEAD) <= bench.DRIVER_SECTION_CAP
    assert bench.driver_filter(_canned(), cap=1000)["roofline"]["step_ms_median"] == 2.8
    assert len(json.dumps(kept)) < 2600


def test_no_string_in_the_kept_sections_is_cut():
    line = _canned()
    for sec in ("config", "roofline", "cpu_baseline"):
        for k, v in line[sec].items():
            if isinstance(v, str):
                assert len(v) <= 128, (sec, k, len(v))


def test_strings_bench_writes_into_kept_sections_are_short():
    """The literal strings bench.py puts into config / cpu_baseline (formatted with worst-case numbers)."""
    import inspect
    import re

    src = inspect.getsource(bench.cpu_baseline)
    m = re.search(r'"sample": "([^"]*)"', src)
    assert m and len(m.group(1) % (10, 200, 99.9, 256)) <= 128


def test_result_line_of_a_full_record_is_short():
    """A full record (round 6's default line, ~25 KB, kept in profiles/) is printed as its result line: the contract's
    keys, the kept sections and the flags, in well under the 8 KB a record of stdout's tail holds."""
    import os

    with open(os.path.join(os.path.dirname(bench.__file__), "profiles", "r06_bench_line.json")) as fh:
        rec = json.load(fh)
    assert len(json.dumps(rec)) > 20000
    line = bench.result_line(rec)
    assert len(json.dumps(line)) <= 4096
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step"):
        assert line[k] == rec[k], k
    assert line["roofline"]["frac"] == rec["roofline"]["frac"]
    assert line["cpu_baseline"]["value"] == rec["cpu_baseline"]["value"]
    assert line["parity_checked"] is True and line["lib_build_id"] == rec["lib_build_id"]


def test_emit_writes_the_record_and_prints_one_line(tmp_path, capsys):
    rec = _canned()
    detail = str(tmp_path / "detail.json")
    bench.emit(rec, detail)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1
    line = json.loads(out[0])
    assert line["detail"] == detail and line == dict(bench.result_line(rec), detail=detail)
    with open(detail) as fh:
        assert json.load(fh) == rec
    bench.emit(rec, "")
    assert json.loads(capsys.readouterr().out)["detail"] is None


def test_dump_outputs_exact_and_capped(tmp_path):
    import numpy as np
    import pytest

    counts = np.array([0, 1, 2 ** 53 - 1], dtype=np.uint64)
    f32 = np.linspace(0, 1, 7, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"counts": counts, "f32": f32, "ov": 0})
    c = np.load(tmp_path / "d" / "counts.npy")
    assert c.dtype == np.float64 and np.array_equal(c.astype(np.uint64), counts)
    g = np.load(tmp_path / "d" / "f32.npy")
    assert g.dtype == np.float32 and np.array_equal(g, f32)
    assert np.load(tmp_path / "d" / "ov.npy").dtype == np.float64
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.array([2 ** 53], dtype=np.uint64)})
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "f"), {"x": np.zeros(bench.DUMP_CAP_BYTES // 8 + 1)})
    assert not (tmp_path / "f").exists()


def test_full_is_off_by_default_and_owns_what_it_runs():
    """A plain run is the headline alone; the options that choose what --full adds are refused without it (a run that
    silently skipped the legs it was asked for would look like a pass), the headline's own switches are not."""
    import pytest

    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert plain.full is False and (plain.steps, plain.warmup) == (3, 1)
    full = bench.parse_args(["--full"])
    assert full.full and full.legs == bench.FULL_LEGS and full.msd_steps == 5 and full.cpu_frames == 10
    assert bench.parse_args(["--full", "--legs", "parity", "--msd-steps", "1"]).legs == "parity"
    for extra in (["--legs", "parity"], ["--msd-steps", "1"], ["--cpu-frames", "4"]):
        with pytest.raises(SystemExit):
            bench.parse_args(extra)
    assert not bench.parse_args(["--no-legs", "--no-cpu-baseline", "--dump-outputs", "d"]).full
