"""
The run plan of mdhip_mol_shape (csrc/shape_plan.h: shape_plan, shape_mass_sums) under AddressSanitizer + UBSan on the
CPU: tests/native/shape_plan_main.cpp includes nothing but that header and walks fixed tables (255 / 256 / 257 molecules
of 3 atoms, 64 / 65 of 16, lengths 1, 1024 and 1025, jobs without molecules, every rule of refusal at the first, a middle
and the last job, the run limit from either side) plus a few thousand seeded random ones: the runs of a job contiguous,
ascending and covering its molecules once, none across a job, a staged run within 256 molecules and 1024 atoms and as
long as they allow, walk runs for the jobs longer than a stage, series0 the prefix sum, the first offending job named.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 3000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "shape_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "shape_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
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
    assert got["plans"] >= N_RANDOM and got["rejected"] > 300 and got["walk"] > 1000 and got["runs"] > 4000000, got
    assert got["failures"] == 0
