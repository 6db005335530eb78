"""
The work tables of the full-lag MSD plan (csrc/lag_plan.h: lag_choose, lag_fused_items, lag_residue_items) under
AddressSanitizer + UBSan on the CPU: tests/native/lag_plan_main.cpp includes nothing but that header and walks the case
table of tests/lag_plan_cases.py plus a few thousand seeded random shapes (F <= 30 000, E <= 300, up to 24 groups with
empty ones, 16 / 128 / 256 / 304 CUs) — every column covered exactly once, offsets monotone, clusters all handed out,
folds inside their batches, no index out of range.
"""
import os
import shutil
import subprocess

import pytest

import lag_plan_cases as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = (("lag_variant", 3), ("lag_w1", 1), ("lag_w12_min_f", 1536), ("lag_fft_kernel", 3), ("lag_direct", -1), ("lag_residue", 1),
        ("lag_overlap", 0), ("lag_batch_mb", 4096), ("lag_batched_fuse", 2))  # the order lag_plan_main.cpp reads, the defaults


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lag_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "lag_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "lag_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    table = tmp_path / "cases.txt"
    with open(table, "w") as fh:
        for case in P.CASES.values():
            assert set(case["opts"]) <= {k for k, _ in OPTS}
            fh.write(" ".join(str(int(v)) for v in [case["F"], case["E"], case["max_lag"], len(case["go"]) - 1, *case["go"],
                                                    *[case["opts"].get(k, d) for k, d in OPTS]]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(table), "3000"], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    words = run.stdout.split()
    assert int(words[1]) == 3000 + len(P.CASES) and words[2] == "(%d" % len(P.CASES)
    paths = {words[k]: int(words[k + 1]) for k in range(7, 17, 2)}
    assert all(v > 500 for v in paths.values()), paths  # every path was walked, many times
    assert words[-2:] == ["failures", "0"]
