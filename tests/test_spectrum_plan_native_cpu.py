"""
The row table and batches of mdhip_velocity_spectrum (csrc/spectrum_plan.h: spectrum_plan) under
AddressSanitizer + UBSan on the CPU: tests/native/spectrum_plan_main.cpp includes nothing but that header and walks fixed
tables (interleaved atom types with entities in no group and a group without entities at byte bounds either side of one
and two rows, no entity at all, sixteen groups, F + max_lag equal to L and one lag more, every rule of refusal with the
bad entity at the front, in the middle and at the end) plus a few thousand seeded random ones: the rows of an axis a
permutation of the grouped entities, ascending inside each group, none for group -1; the batches (one axis of a range of
consecutive entities each) whole rows, covering every row once and within the byte bound, every group a contiguous
segment of the batch; every invalid table refused with its rule.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 3000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_spectrum_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "spectrum_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "spectrum_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-300:])
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: int(words[k + 1]) for k in range(0, 10, 2)}
    assert got["plans"] >= N_RANDOM and got["rejected"] > 300 and got["batches"] > 100000 and got["rows"] > 4000000, got
    assert got["failures"] == 0
