"""
The table packer of the per-molecule job calls and mdhip_free_volume (csrc/call_tables.h: CallTables, behind
mdhip_axis_vectors, mdhip_mol_moments, mdhip_dihedral_angles, mdhip_mol_shape and mdhip_free_volume) under
AddressSanitizer + UBSan on the CPU: tests/native/call_tables_main.cpp includes nothing but that header — g++ sees only
its host part — and walks fixed layouts (elements of 1, 2, 4, 8, 40 and 48 bytes with counts 0, 1 and odd; optional
segments, absent and present, at the front, in the middle and at the end; zeroed segments) plus a few thousand seeded
random ones, each resolved on a real buffer: every offset a multiple of 8, no two segments overlapping, the total the
end of the last segment, a null pointer for an absent segment, no room for an empty one. The layouts of the five entry
points come out at the offsets their hand-written sums gave, typed in as numbers for one small call each.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 4000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_call_tables_layouts_under_asan(tmp_path):
    exe = str(tmp_path / "call_tables_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "call_tables_main.cpp"), "-o", exe], capture_output=True, text=True)
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
    assert got["layouts"] >= N_RANDOM + 200 and got["absent"] > 1000 and got["empty"] > 1000, got
    assert got["failures"] == 0
