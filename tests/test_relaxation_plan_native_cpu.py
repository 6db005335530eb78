"""
The host side of mdhip_self_relaxation (csrc/relaxation_plan.h: tile geometry, launch slices, the 2^30 size guard and the
sinc evaluation) under AddressSanitizer + UBSan on the CPU: tests/native/relaxation_plan_main.cpp includes nothing but
that header. For 17 frame counts around the tile sizes, 12 lag limits and 10 origin strides each, every cell (origin,
lag) with t0 + lag <= F - 1 is in exactly one (launch, tile, lane, slot) and no other cell is; at sizes up to 2^29 - 1
frames every launch dimension is within 65 535 and the slices partition the tile ranges; the guard sits at
origins * size = 2^30 and does not overflow; the sinc is within 2^-34 of the long double sine's over three million
arguments (below the far cut within 2^-43, as the header derives).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_relaxation_plan_under_asan(tmp_path):
    exe = str(tmp_path / "relaxation_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "relaxation_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-300:])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: float(words[k + 1]) for k in range(0, 14, 2)}
    assert got["cells"] > 900000 and got["launches"] > 40000 and got["guard"] > 5000 and got["sinc"] > 3000000, got
    assert got["sinc_err_log2"] <= -34.0 and got["below_far_log2"] <= -43.0, got
    assert got["failures"] == 0
