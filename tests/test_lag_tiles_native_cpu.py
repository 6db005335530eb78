"""
The host part of csrc/lag_tiles.h — the slab and chunk plans behind xcorr_direct (mdhip_xcorr*, mdhip_green_kubo),
mdhip_cross_msd and mdhip_orient_corr, and the geometry helpers their kernels share — under
AddressSanitizer + UBSan on the CPU: tests/native/lag_tiles_main.cpp includes nothing but that header and walks fixed
edge tables (n from 1 to 2^29 - 1, 1 / 256 / 37 CUs, 1 and 16 groups with and without the |term| sums, 0 / 1 / 32768
molecule slabs, lag ranges that begin behind 0, a forced slab count, budgets from 4 KiB to 16 GiB) plus a few thousand
seeded random ones: every plan equals the three formulas the entry points used before the header existed (written out
in the program), n_slabs in [1, 65535], every grid dimension within its launch limit, a chunk's partial sums within the
budget unless it is ONE unit, the chunks covering the units once and in order — many chunks, under the small budgets.
For the three kernels' geometries at the sizes the GPU tests use (1, 2, TT +- 1, KT +- 1, KT + TT + 1, 2 KT +- 1,
3 KT - 5) and three tiny ones at every n up to 70: every tile in exactly one (workgroup, half), every lag in exactly one
(tile, lane, j), the slab ranges of a tile a partition of [0, n - K0) — more slabs than stages, K0 = n - 1 — at the
kernel's alignment, the stages of a slab adding up to it, the stage slot map a bijection into the row blocks; at every
stage and for every wave, the fast-step count (Tiles::fast_steps, the rule of the unpredicated loops) never above the
stage's steps and T0 + tt + K0 + wave_hi - 1 <= n - 1 at every fast step, and the lines cross_msd_kernel and
orient_corr_kernel type out equal to it.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 3000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lag_tiles_plans_and_walker_under_asan(tmp_path):
    exe = str(tmp_path / "lag_tiles_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "lag_tiles_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-300:])
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: int(words[k + 1]) for k in range(0, 14, 2)}
    assert got["plans"] >= 3 * N_RANDOM + 20000 and got["many_chunk_plans"] > 5000 and got["geometries"] == 6, got
    assert got["chunks"] > 10000000 and got["slab_ranges"] > 10000000 and got["fast_steps"] > 400000, got
    assert got["failures"] == 0
