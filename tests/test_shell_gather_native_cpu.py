"""
The host part of csrc/shell_gather.h (the integer table packer shell::IntTable and shell::shares_an_atom, behind
mdhip_angle_hist, mdhip_bond_order, mdhip_sdf_hist, mdhip_body_frames, mdhip_contact_components and the two hydrogen-bond
calls) under AddressSanitizer + UBSan on the CPU: tests/native/shell_gather_main.cpp includes nothing but that header —
g++ sees only its host part — and packs fixed tables in the shapes of those entry points (two to six segments of
lengths 0, 1, 2, 63, 4096, 4097, NULL + 0 segments, generated segments, the optional last segment given and absent)
plus seeded random ones: every offset, every value read through the resolved pointers of a copy of the table that is
exactly as long as the table, the total, the null pointer of an absent segment, and the pointer of an empty present one
(where the next segment begins). shares_an_atom runs on disjoint, identical, one-shared-at-each-end and empty lists and
on random short ones, against the brute-force answer.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 2000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shell_gather_host_part_under_asan(tmp_path):
    exe = str(tmp_path / "shell_gather_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "shell_gather_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    print(run.stdout[-500:])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    words = run.stdout.split()
    got = {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}
    # every class of case was reached
    assert got["tables"] >= N_RANDOM + 200, got  # (the random ones and 36 x 6 + 4 fixed ones)
    assert got["shares"] >= N_RANDOM + 17, got   # (the random ones and the 17 fixed ones)
    for key, least in (("len0", 100), ("len1", 100), ("len4097", 100), ("null0", 100), ("absent", 100),
                       ("generated", 100), ("six", 100), ("disjoint", 2), ("identical", 2), ("first_end", 2),
                       ("last_end", 2), ("empty_list", 3)):
        assert got[key] >= least, (key, got)
    assert got["failures"] == 0
