"""
The plan of the per-molecule COM and charge-flux calls (csrc/seg_plan.h: seg_plan, build_seg_blocks, pick_seg_cap,
seg_sums) under AddressSanitizer + UBSan on the CPU: tests/native/seg_plan_main.cpp includes nothing but that header and
walks every table of tests/segment_exact.py under every option set of its CONFIGS — the COM with each plane count of
N_ATTR, and the flux — plus a few thousand seeded random tables (segments of 1..1100 atoms, runs of one-atom segments
around the 64 / 256 segments-per-run limits, 16 / 128 / 256 / 304 CUs): every segment in exactly one run, the runs in
order and inside their stage, the grid in range, the sums bit for bit, the walk form exactly past 1024 atoms. The kernel
each fixed case picks is held against segment_exact.expected_kernel, which tests/test_gpu_segment_exact.py holds
against the real call.
"""
import os
import shutil
import subprocess

import pytest

import segment_exact as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 4000


def _cases():
    """(flux, cfg, name, sizes, K, F) in the order of the file's lines."""
    tables = dict(X.segment_tables())
    tables["types"] = X.type_table()[0]
    for name, sizes in sorted(tables.items()):
        for F in (X.FRAMES, X.MANY_FRAMES) if name in X.MANY_TABLES else (X.FRAMES,):
            for cfg in X.CONFIGS:
                for K in X.N_ATTR:
                    yield False, cfg, name, sizes, K, F
                yield True, cfg, name, sizes, 3, F


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_seg_plan_tables_under_asan(tmp_path):
    exe = str(tmp_path / "seg_plan_main")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         os.path.join(REPO, "tests", "native", "seg_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in (build.stderr or "").lower():
        pytest.skip("libasan not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    assert not build.stderr.strip(), build.stderr[-2000:]  # (-Wall: no warning)
    cases = list(_cases())
    table = tmp_path / "cases.txt"
    with open(table, "w") as fh:
        for flux, (frame, cap, vec, gy), _, sizes, K, F in cases:
            fh.write(" ".join(str(int(v)) for v in [flux, frame, cap, vec, gy, K, F, len(sizes), *sizes]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(table), str(N_RANDOM)], capture_output=True, text=True, env=env, timeout=600)
    lines = run.stdout.splitlines()
    print("\n".join(lines[-3:]))
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    picks = [ln[5:] for ln in lines if ln.startswith("pick ")]
    assert len(picks) == len(cases)
    listed, seen = 0, set()
    for got, (flux, cfg, name, sizes, K, F) in zip(picks, cases):
        want = X.expected_kernel(flux, cfg, sizes, name, K)
        seen.add(got)
        if want is not None:
            listed += 1
            assert got == want, (name, "flux" if flux else "COM", cfg, K, F)
    assert listed > 0.8 * len(cases)  # (None only for pick_seg_cap's choice on the tables picked_cap does not list)
    assert len(seen) == 12, sorted(seen)  # every instance of either call
    words = lines[-1].split()
    assert int(words[1]) == 4 * (N_RANDOM + len(cases)) and words[2] == "(%d" % len(cases)
    forms = {words[k]: int(words[k + 1]) for k in (7, 9, 11)}
    assert set(forms) == {"walk", "staged", "frame"} and all(v > 1000 for v in forms.values()), forms
    assert words[-2:] == ["failures", "0"]
