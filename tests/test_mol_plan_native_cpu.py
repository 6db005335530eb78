"""
The job plan of the per-molecule series calls (csrc/mol_tile.h: mol_plan, behind mdhip_axis_vectors and
mdhip_dihedral_angles) under AddressSanitizer + UBSan on the CPU: tests/native/mol_plan_main.cpp includes nothing but
that header — g++ sees only its host part — and walks fixed tables (jobs without molecules at the front, in the middle
and at the end; keys A, B, A; a class that fills to a lowered max_class_jobs and opens again; 63 / 64 / 65 / 128
molecules; every rule of refusal at the first, a middle and the last job) plus a few thousand seeded random ones, pooled
and not: every job in exactly one class, the jobs of a class contiguous and in call order, tile0 in steps of
ceil(mols / 64), series0 the prefix sum of job_mols, one class per job without pooling, the first offending job named.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 4000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mol_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "mol_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "mol_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-300:])
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: int(words[k + 1]) for k in range(0, 8, 2)}
    assert got["plans"] >= 2 * N_RANDOM and got["rejected"] > 500 and got["reopened"] > 500, got
    assert got["failures"] == 0
