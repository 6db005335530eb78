"""
The helper threads of the host-to-device ring (csrc/copy_pool.h: CopyPool, which mdhip_h2d_any fills its page-locked
chunks with) as a stand-alone program under the sanitizers, on the CPU: tests/native/copy_pool_main.cpp includes nothing
of the project but that header. It copies every size around the 64-byte split of a chunk over the four helpers (0 bytes
to 8 MiB + 40, the size of test_gpu_host_staging's one-chunk-and-40-bytes batch) at source and destination offsets 0, 1,
8 and 63, compares contents and the guard bytes around the destination, sends a few thousand copies of seeded random
sizes through one pool, constructs and destroys 200 pools (most without a copy), and drives two pools from two threads.
Built and run twice: -fsanitize=thread (the hand-off between copy() and the helpers, the destructor against helpers
that have not started waiting yet) and -fsanitize=address,undefined (the ranges a helper is given).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COPIES = 14 * 16 + 4000 + 50 + 4 + 2 * 1500  # fixed sizes x offsets, one pool, the short-lived pools, two callers


def _build_and_run(tmp_path, tag, sanitize, env):
    exe = str(tmp_path / ("copy_pool_" + tag))
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=" + sanitize, "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "copy_pool_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and any(lib in (build.stderr or "").lower() for lib in ("asan", "tsan", "ubsan")):
        pytest.skip("sanitizer runtime not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
    lines = run.stdout.splitlines()
    print("\n".join(lines[-5:]))
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert not run.stderr.strip(), run.stderr[-3000:]  # (a sanitizer report that did not end the program)
    assert lines and lines[-1].split() == ["copies", str(N_COPIES), "failures", "0"], lines[-3:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_copy_pool_under_tsan(tmp_path):
    _build_and_run(tmp_path, "tsan", "thread", {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_copy_pool_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "asan", "address,undefined",
                   {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"})
