"""
The unit plan of the two-group pair sweeps (csrc/group_pairs.h: gp_plan and gp_band, behind mdhip_van_hove_distinct and
mdhip_vector_pair_hist) under AddressSanitizer + UBSan on the CPU: tests/native/group_pairs_plan_main.cpp includes
nothing but that header — g++ sees only its host part — and walks fixed tables (na, nb in {0, 1, 63, 64, 65, 128, 2^20,
2^20 + 1}, a equal to b, 0 / 1 / 70 001 origins, nbins 1 / 4096 / 16128 / 16129, sizes at the entry points' 2^40 limits)
plus a few thousand seeded random jobs, under both kernels' rule records and chunks of 3, 64 and 2^20 uniform entities:
the lanes rule and its ends, the unit and workgroup counts, the wrap cap upb * 64 * min(nu, chunk) <= max_pairs,
upb >= waves, the pair count, and every (origin, lane entity, uniform entity) of the small jobs visited exactly once.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 4000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_group_pairs_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "group_pairs_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "group_pairs_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-300:])
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}
    assert got["jobs"] >= N_RANDOM + 5000, got
    # every class of case was reached: lanes holding b, a equal to b, jobs without units, more than one chunk, upb held
    # down by max_pairs, jobs decoded unit by unit, the 2^40 limits
    for key, least in (("lanes_b", 1000), ("same", 500), ("empty", 500), ("chunked", 1000), ("capped", 20),
                       ("walked", 1000), ("limit", 7)):
        assert got[key] >= least, (key, got)
    assert got["failures"] == 0
