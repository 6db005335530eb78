"""CPU-only checks of the boundary: the library builds, loads, exports every symbol the header
declares, its host-side edge table is exact, and the product fails loudly without a GPU."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from mdproptools_amd import _lib


def test_header_symbols_are_exported():
    text = open(os.path.join(REPO, "include", "mdhip.h")).read()
    declared = set(re.findall(r"\b(mdhip_[a-z_0-9]+)\s*\(", text))
    declared.discard("mdhip_ctx")
    assert declared, "no declarations found"
    lib = _lib.load()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    assert lib.mdhip_version() == 610


def _ref_bin(rsq, ddr):
    return (np.sqrt(rsq) / ddr).astype(np.int64)


@pytest.mark.parametrize("r_cut,ddr", [(20.0, 0.05), (13.0, 0.05), (10.0, 0.1), (12.0, 0.02), (20.0, 0.01),
                                       (7.3, 0.173)])
def test_bin_edges_are_exact(r_cut, ddr):
    nb = int(r_cut / ddr)
    e = _lib.bin_edges(ddr, nb)
    assert e[0] == 0.0 and np.all(np.diff(e) > 0)
    k = np.arange(1, nb + 1)
    # e[k] is in bin k and the double just below it is in bin k-1
    np.testing.assert_array_equal(_ref_bin(e[1:], ddr), k)
    np.testing.assert_array_equal(_ref_bin(np.nextafter(e[1:], 0.0), ddr), k - 1)
    # the reference rule agrees with table binning on random rsq, including values next to edges
    rng = np.random.default_rng(7)
    rsq = np.concatenate([rng.uniform(0, r_cut ** 2, 20000), e, np.nextafter(e[1:], 0), np.nextafter(e, np.inf)])
    rsq = rsq[rsq < e[-1]]
    np.testing.assert_array_equal(np.searchsorted(e, rsq, side="right") - 1, _ref_bin(rsq, ddr))


def test_edges_are_not_the_naive_squares():
    """(k*ddr)**2 is the wrong edge for most bins, and bin 400 is reachable below 20**2."""
    e = _lib.bin_edges(0.05, 400)
    naive = (np.arange(401) * 0.05) ** 2
    assert int((e != naive).sum()) == 242
    assert e[400] < 400.0  # overflow bin reachable for (20, 0.05)
    e13 = _lib.bin_edges(0.05, 260)
    assert e13[260] == 169.0  # not reachable for (13, 0.05)


def test_no_cpu_fallback():
    """Without a GPU the product must fail loudly, not compute on the host."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.MdhipError):
        _lib.Context(0)
    from mdproptools_amd import backend

    with pytest.raises(_lib.MdhipError):
        backend.cumtrapz(np.arange(8.0), 1.0)


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "mdproptools_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                hits = re.findall(r"^\s*(?:from|import)\s+oracle\b|__import__\([\"']oracle|import_module\([\"']oracle",
                                  src, flags=re.M)
                assert not hits, (os.path.join(root, f), hits)
    # tools/ holds product-side measurement scripts: no oracle there either (oracle-based ones live in tests/bench/)
    for f in os.listdir(os.path.join(REPO, "tools")):
        if f.endswith(".py"):
            src = open(os.path.join(REPO, "tools", f)).read()
            assert not re.findall(r"^\s*(?:from|import)\s+oracle\b", src, flags=re.M), f
    # bench.py: only inside the cpu_baseline_* (the timed CPU sample) and cpu_check_* (the checker of a leg's result)
    # functions — never in the code that produces a measured value
    src = open(os.path.join(REPO, "bench.py")).read()
    for m in re.finditer(r"^\s*(?:from|import)\s+oracle\b", src, flags=re.M):
        enclosing = re.findall(r"^def (\w+)\(", src[: m.start()], flags=re.M)[-1]
        assert enclosing.startswith("cpu_baseline") or enclosing.startswith("cpu_check"), enclosing


def test_header_is_plain_c(tmp_path):
    """include/mdhip.h is the drop-in boundary: it must compile as C99 (no C++-isms, no torch / HIP types) and
    link against libmdhip.so from a C program."""
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = tmp_path / "use_mdhip.c"
    src.write_text(
        '#include "mdhip.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  double e[5];\n"
        "  if (mdhip_version() <= 0) return 1;\n"
        "  if (mdhip_bin_edges(0.05, 4, e) != MDHIP_OK || e[0] != 0.0) return 2;\n"
        '  printf("%d %.17g\\n", mdhip_version(), e[4]);\n'
        "  return 0;\n}\n")
    exe = tmp_path / "use_mdhip"
    lib_dir = os.path.join(REPO, "mdproptools_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"),
                        str(src), "-L", lib_dir, "-l:libmdhip.so", "-Wl,-rpath," + lib_dir, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert float(run.stdout.split()[1]) > 0.039  # edges[4] ~ (4 * 0.05)^2


def _f32_guess_emulation(rng, n, L, r_cut, bin_size, s_cap, wrap):
    """Emulates, pair by pair in IEEE float32, what pair_hist_sj_kernel<3> computes for the bin guess (DESIGN.md
    4.1b): tile-relative coordinates rounded to f32, the packed difference / product / two fused multiply-adds,
    an (exactly rounded) square root, 1/ddr rounded to f32 and the final fma — next to the reference's f64 value."""
    f32 = np.float32
    Lv = np.array(L, dtype=np.float64)
    c = rng.uniform(0, 1, 3) * Lv                               # tile centre
    xj = c + rng.uniform(-1, 1, (n, 3)) * 0.25 * (s_cap - r_cut)  # j atoms around the centre
    # i atoms anywhere within reach of the j atoms, possibly across the periodic boundary
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    xi = xj + u * rng.uniform(0, 1.02 * r_cut, (n, 1)) + rng.integers(-1, 2, (n, 3)) * Lv
    # the reference (rdf_cn.py:35-69): single wrap, f64
    d = xi - xj
    d = np.where(np.abs(d) > Lv / 2, d - np.sign(d) * Lv, d)
    rsq_ref = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    g_ref = np.sqrt(rsq_ref) / bin_size
    # the device chain; it only covers lanes with |x_i - c| + h < 1.49 L (the reference's single wrap is the nearest
    # image there) — anything else is swept by the f64 chain
    q = xi - c
    h = np.abs(xj - c).max(axis=0)
    cov = np.all(np.abs(q) + h < 1.49 * Lv, axis=1)
    xi, xj, q, g_ref, rsq_ref = xi[cov], xj[cov], q[cov], g_ref[cov], rsq_ref[cov]
    xr_i = (q - Lv * np.rint(q / Lv)).astype(f32)               # f64 per lane, then one rounding to f32
    xr_j = (xj - c).astype(f32)
    dd = xr_i - xr_j                                            # f32 subtraction
    if wrap:
        L32, iL32 = Lv.astype(f32), (1.0 / Lv).astype(f32)
        nn = np.rint(dd * iL32)                                 # f32 product, round to even
        dd = (dd.astype(np.float64) - nn.astype(np.float64) * L32.astype(np.float64)).astype(f32)  # one fma rounding
    else:
        # where the kernel takes the plain difference: |d'| <= L - r_cut - margin on every axis (axis_plain)
        margin = 1.0e-3 * Lv + 1.0e-3
        keep = np.all(np.abs(dd.astype(np.float64)) <= Lv - r_cut - margin, axis=1)
        dd, g_ref, rsq_ref = dd[keep], g_ref[keep], rsq_ref[keep]
        # d' is the nearest image unless some |d'| > L/2 — and then BOTH d' and the nearest image are beyond the
        # cutoff on that axis alone, so the pair is out of the cutoff for the reference and for the f32 chain alike
        far = np.any(np.abs(dd.astype(np.float64)) > Lv / 2, axis=1)
        assert np.all(rsq_ref[far] > r_cut * r_cut * (1 + 1e-6))
        assert np.all(np.max(np.abs(dd[far].astype(np.float64)), axis=1) > r_cut * (1 + 1e-6))
        dd, g_ref, rsq_ref = dd[~far], g_ref[~far], rsq_ref[~far]
    r = dd[:, 0] * dd[:, 0]                                     # f32 product
    r = (dd[:, 1].astype(np.float64) ** 2 + r.astype(np.float64)).astype(f32)  # fma: exact in f64, one rounding
    r = (dd[:, 2].astype(np.float64) ** 2 + r.astype(np.float64)).astype(f32)
    s = np.sqrt(r.astype(np.float64)).astype(f32)               # <= 0.5 ulp; the bound allows 1 ulp (v_sqrt_f32)
    gs = f32(1.0 / bin_size)
    g32 = (s.astype(np.float64) * np.float64(gs)).astype(f32)   # fma with a zero addend
    inside = rsq_ref < (1.02 * r_cut) ** 2
    return np.abs(g32.astype(np.float64) - g_ref)[inside]


@pytest.mark.parametrize("L,r_cut,bin_size", [((50.0, 50.0, 50.0), 20.0, 0.05), ((104.0, 104.0, 104.0), 20.0, 0.05),
                                              ((31.0, 44.0, 37.5), 15.4, 0.1), ((26.0, 26.0, 26.0), 12.5, 0.025)])
def test_packed_f32_error_bound_covers_emulation(L, r_cut, bin_size):
    """The exactness of the packed-f32 sweep rests on mdhip_pk_error_bound: every pair whose f32 guess is farther
    than that from an integer is binned without the f64 chain. Emulate the device's f32 operations on 400k random
    pairs per case (with and without the per-pair wrap) and compare the worst observed deviation with the bound."""
    lib = _lib.load()
    nbins = int(round(r_cut / bin_size))
    edge = (256 * L[0] * L[1] * L[2] / 10000.0) ** (1 / 3)
    s_cap = r_cut + 3.5 * edge
    bound = lib.mdhip_pk_error_bound(r_cut, bin_size, nbins, 1, s_cap, max(L))
    assert 0 < bound < 0.01
    rng = np.random.default_rng(4242)
    for wrap in (False, True):
        err = _f32_guess_emulation(rng, 400_000, L, r_cut, bin_size, s_cap, wrap)
        assert len(err) > 100_000
        # the emulated chain has an exactly rounded sqrt (the device: 1 ulp), so it must sit well inside
        assert err.max() < 0.8 * bound, (wrap, err.max(), bound)
        assert err.max() > 0.02 * bound, "the bound is vacuous"


def _displace(cls):
    import ctypes as C

    lib = _lib.load()
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    n_ti, n_tj = cls.shape
    a = np.full(n_ti, -1, np.int32)
    b = np.full(n_tj, -1, np.int32)
    rc = np.full(n_ti * n_tj + 8, -7, np.int32)
    rows = C.c_int(-1)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    assert lib.mdhip_row_displacement(n_ti, n_tj, ip(cls), ip(a), ip(b), ip(rc), C.byref(rows)) == 0
    return rows.value, a, b, rc


def _tri_classes(n, rels):
    cls = np.full((n, n), len(rels), np.int32)
    for k, (x, y) in enumerate(rels):
        cls[x, y] = cls[y, x] = k
    return cls


def test_row_displacement_never_mixes_classes():
    """mdhip_row_displacement: row(ti, tj) = a[ti] + b[tj] may merge type pairs only within one class, every
    row's class is what row_cls says, fewer rows than n_ti * n_tj — for the reference's own example (nine atom types, the
    five relations 9-1, 9-4, 9-6, 9-9, 1-3 -> six type indices, 36 plain rows), star-shaped and random relation sets,
    and rectangular (atoms x sites) tables."""
    rng = np.random.default_rng(5)
    cases = [_tri_classes(6, [(4, 0), (4, 2), (4, 3), (4, 4), (0, 1)]),  # C1: indices of 1, 3, 4, 6, 9, other
             _tri_classes(3, [(1, 0), (1, 1)]),                            # altered ids: 32-17, 32-32
             _tri_classes(10, [(9, j) for j in range(1, 10)]),
             _tri_classes(9, [(i, j) for i in range(9) for j in range(i, 9)])]  # every pair named: nothing to gain
    for _ in range(30):
        n = int(rng.integers(3, 13))
        pairs = [(i, j) for i in range(n) for j in range(i, n)]
        pick = rng.permutation(len(pairs))[: int(rng.integers(1, min(len(pairs), 12) + 1))]
        cases.append(_tri_classes(n, [pairs[k] for k in pick]))
    for _ in range(10):  # rectangular: ordered (atom type, site type) classes
        n_ti, n_tj = int(rng.integers(2, 9)), int(rng.integers(2, 6))
        cls = np.full((n_ti, n_tj), 0, np.int32)
        k = int(rng.integers(1, 6))
        cls[:] = k
        for c in range(k):
            cls[rng.integers(0, n_ti), rng.integers(0, n_tj)] = c
        cases.append(cls)
    gained = 0
    for cls in cases:
        rows, a, b, rc = _displace(cls)
        n_ti, n_tj = cls.shape
        if rows == 0:
            continue
        gained += 1
        assert 0 < rows < n_ti * n_tj
        assert a.min() >= 0 and b.min() >= 0 and a.max() + b.max() + 1 == rows
        seen = {}
        for i in range(n_ti):
            for j in range(n_tj):
                r = int(a[i] + b[j])
                assert rc[r] == cls[i, j], (cls, a, b, i, j)
                seen[r] = True
        assert all(rc[r] == -1 for r in range(rows) if r not in seen)
        again = _displace(cls)
        assert again[0] == rows and np.array_equal(again[1], a) and np.array_equal(again[2], b)  # deterministic
    rows_c1 = _displace(cases[0])[0]
    assert 0 < rows_c1 <= 18, rows_c1  # 36 plain rows; <= 33 needed to fit a third of LDS at 400 bins
    assert _displace(cases[3])[0] == 0
    assert gained >= 20


# What the MI355X ran for every case of tests/pair_plan_cases.py at the commit BEFORE the plan was split from the batch
# runner (f070edf, "Add number_density.calc_number_density with a HIP axis-profile kernel"): last_kernel_name() and the
# launch count of last_kernel_ms() after the real call. A call that takes two sweeps leaves the second sweep's (CN) kernel.
RECORDED_AT_F070EDF = {
    "C2":                          ('pair_hist_sj_kernel<3, true, false>', 1),
    "C1":                          ('pair_hist_sj_kernel<3, true, false>', 1),
    "C1alt":                       ('pair_hist_sj_kernel<3, true, false>', 1),
    "C1full":                      ('pair_hist_sj_kernel<3, true, false, true>', 1),
    "C3_rdf":                      ('pair_hist_sj_kernel<3, true, false>', 1),
    "C3_cn":                       ('pair_hist_sj_kernel<3, true, true>', 1),
    "C3_rdf_cn":                   ('pair_hist_sj_kernel<3, true, true>', 1),
    "sites_rdf":                   ('pair_hist_sj_kernel<3, true, false>', 1),
    "sites_cn":                    ('pair_hist_sj_kernel<1, true, false>', 1),
    "base":                        ('pair_hist_sj_kernel<3, true, false>', 1),
    "base_cn":                     ('pair_hist_sj_kernel<3, true, true>', 1),
    "base_rdf_cn":                 ('pair_hist_sj_kernel<3, true, true>', 1),
    "dense_small_frame":           ('pair_hist_fast_kernel<true, 8, 0, false>', 1),
    "few_bins_edge_table":         ('pair_hist_kernel<true>', 1),
    "cn_70_cutoffs":               ('pair_hist_kernel<true>', 1),
    "cutoff_inside_bin":           ('pair_hist_sj_kernel<4, true, false>', 1),
    "cutoff_inside_bin_rows":      ('pair_hist_sj_kernel<6, true, false>', 1),
    "per_frame":                   ('pair_hist_sj_kernel<3, false, false>', 1),
    "device_result":               ('pair_hist_sj_kernel<3, true, false>', 1),
    "device_result_small_frame":   ('pair_hist_fast_kernel<true, 8, 0, false>', 1),
    "twelve_types_all_pairs":      ('pair_hist_sj_kernel<5, true, false>', 4),
    "box_4000":                    ('pair_hist_sj_kernel<2, true, false>', 1),
    "cn_beyond_r_cut":             ('pair_hist_sj_kernel<3, true, true>', 1),
    "cn_two_cutoffs_one_class":    ('pair_hist_sj_kernel<1, true, false>', 1),
    "host_batches":                ('pair_hist_sj_kernel<3, true, false>', 2),
    "rdf_pk_0":                    ('pair_hist_sj_kernel<2, true, false>', 1),
    "rdf_pk_2":                    ('pair_hist_sj_kernel<2, true, false>', 1),
    "rdf_sj_0":                    ('pair_hist_fast_kernel<true, 8, 0, true>', 1),
    "rdf_sj_2":                    ('pair_hist_sj_kernel<3, false, false>', 1),
    "rdf_cull_0":                  ('pair_hist_fast_kernel<true, 8, 0, false>', 1),
    "dense_box":                   ('pair_hist_fast_kernel<true, 8, 0, false>', 1),
    "rdf_cull_1":                  ('pair_hist_sj_kernel<3, true, false>', 1),
    "rdf_rows_0":                  ('pair_hist_sj_kernel<5, true, false>', 1),
    "c1_small":                    ('pair_hist_sj_kernel<3, true, false>', 1),
    "rdf_disp_0":                  ('pair_hist_sj_kernel<5, true, false>', 1),
    "star5":                       ('pair_hist_sj_kernel<3, true, false>', 1),
    "rdf_disp_2":                  ('pair_hist_sj_kernel<3, true, false>', 1),
    "c1full_small":                ('pair_hist_sj_kernel<3, true, false, true>', 1),
    "rdf_big_0":                   ('pair_hist_sj_kernel<5, true, false>', 2),
    "rdf_pk_passes_0":             ('pair_hist_sj_kernel<0, true, false>', 3),
    "rdf_variant_0":               ('pair_hist_kernel<true>', 1),
    "cn_pk_0":                     ('pair_hist_sj_kernel<1, true, false>', 1),
}


def test_pair_plan_picks_what_the_device_ran():
    """mdhip_pair_plan with the MI355X's two limits (256 CUs, 160 KB of LDS) names, for every branch of the decision,
    the kernel instance and the number of launches recorded from real calls on that device at the parent commit."""
    import pair_plan_cases as P

    assert set(RECORDED_AT_F070EDF) == set(P.CASES)
    got = {name: P.plan(case) for name, case in P.CASES.items()}
    two_sweeps = {"cn_beyond_r_cut", "cn_two_cutoffs_one_class"}
    for name, (kernel, launches) in RECORDED_AT_F070EDF.items():
        g = got[name]
        if name in two_sweeps:
            # the RDF sweep (described by the plan) and then the CN call of the same shape, whose kernel was recorded
            assert g["status"] == P.TWO_SWEEPS, (name, g)
            assert g["kernel"] == got["base"]["kernel"], (name, g)
            g = P.plan(dict(P.CASES[name], op="cn"))
        assert g["status"] == 0 and (g["kernel"], g["launches"]) == (kernel, launches), (name, g, kernel, launches)
    # what the name alone does not show
    flags = lambda name: tuple(got[name][k] for k in ("sj_mode", "n_pass", "ord_rows", "displaced", "big", "packed"))  # noqa: E731
    assert flags("C2") == (3, 1, 16, 0, 0, 1)
    assert flags("C1")[2:] == (15, 1, 0, 1) and flags("c1_small") == flags("C1")   # 36 plain rows do not fit, 15 displaced do
    assert flags("rdf_disp_0") == (5, 1, 0, 0, 0, 1)                                # ... without them: class rows
    assert flags("C1full") == (3, 1, 81, 0, 1, 1)                                   # one 16-wave block per CU
    assert flags("rdf_big_0") == (5, 2, 0, 0, 0, 1)                                 # ... without it: two passes
    assert flags("star5")[2:4] == (36, 0) and flags("rdf_disp_2")[3] == 1 and flags("rdf_disp_2")[2] < 36
    assert flags("twelve_types_all_pairs")[:2] == (5, 4) and flags("rdf_pk_passes_0")[0] == 0
    assert flags("cutoff_inside_bin")[0] == 4 and flags("cutoff_inside_bin_rows")[0] == 6
    assert flags("box_4000") == (2, 1, 9, 0, 0, 0) and flags("rdf_pk_0") == flags("box_4000")
    assert flags("rdf_rows_0")[0] == 5 and flags("rdf_pk_2")[0] == 2
    assert got["host_batches"]["launches"] == 2 and got["base"]["launches"] == 1
    for name in ("dense_small_frame", "few_bins_edge_table", "cn_70_cutoffs", "rdf_sj_0", "rdf_cull_0", "dense_box",
                 "rdf_variant_0"):
        assert got[name]["sj_mode"] == -1, name
    # the two limit errors come back as the plan's status, with the library's message
    too_many_bins = P.plan(dict(P.CASES["base"], bin=0.0002, nbins=50000))
    assert too_many_bins["status"] == -5 and "50000 bins do not fit LDS" in too_many_bins["kernel"]
    # ... and the limits are read: a device with 64 KB of LDS cannot hold C1full's 81 rows in one block
    assert P.plan(P.CASES["C1full"], lds_bytes=65536)["big"] == 0


# What the parent commit (e1b4349, "Sharded MSD: one shard plan and a step object replace the closures") reports in
# last_kernel_name() and as the launch count of last_kernel_ms() for every case of tests/lag_plan_cases.py. NOT a device
# record: no MI355X could be had while the plan was split off, so the table was derived by reading that commit's
# mdhip_lag_msd_fft (every spectral path starts ONE KernelTimer: one launch run) and transcribing its path choice by hand,
# independently of csrc/lag_plan.h. tests/test_gpu_lag_plan.py holds the plan against the real call on a device; a record
# of P.run() at e1b4349 should replace this table when a device is at hand.
PARENT_E1B4349_REPORTS = {
    "w1_2":                 ('msd_power_w1_kernel', 1),
    "w1_300":               ('msd_power_w1_kernel', 1),
    "w1_1024":              ('msd_power_w1_kernel', 1),
    "w1_1025":              ('msd_power_w1_kernel', 1),
    "w1_1535":              ('msd_power_w1_kernel', 1),
    "w1_ends_1536":         ('msd_power_w12_kernel', 1),
    "w1_off":               ('msd_power_lds_kernel', 1),
    "w1_17_groups":         ('msd_power_lds_kernel', 1),
    "w12_short_1600":       ('msd_power_w12_kernel', 1),
    "w12_short_3071":       ('msd_power_w12_kernel', 1),
    "w12_qe4_3072":         ('msd_power_w12_kernel', 1),
    "w12_qe5_4097":         ('msd_power_w12_kernel', 1),
    "w12_qe5_5000":         ('msd_power_w12_kernel', 1),
    "w12_qe5_5120":         ('msd_power_w12_kernel', 1),
    "w12_qe6_5121":         ('msd_power_w12_kernel', 1),
    "w12_qe6_6144":         ('msd_power_w12_kernel', 1),
    "w12_short_src0":       ('msd_power_w12_kernel', 1),
    "w12_qe4_src0":         ('msd_power_w12_kernel', 1),
    "w12_qe6_src0":         ('msd_power_w12_kernel', 1),
    "w12_min_f_0":          ('msd_power_lds_kernel', 1),
    "pow2_6145":            ('msd_power_lds_kernel', 1),
    "pow2_8192":            ('msd_power_lds_kernel', 1),
    "k0_2100":              ('msd_power_lds_kernel', 1),
    "k1_2100":              ('msd_power_lds_kernel', 1),
    "k2_2100":              ('msd_power_lds_kernel', 1),
    "k0_qr1":               ('msd_power_lds_kernel', 1),
    "k0_qr2":               ('msd_power_lds_kernel', 1),
    "k0_qr4":               ('msd_power_lds_kernel', 1),
    "k0_qr10":              ('msd_power_lds_kernel', 1),
    "k0_qr12":              ('msd_power_lds_kernel', 1),
    "k0_qr16":              ('msd_power_lds_kernel', 1),
    "k0_qr24":              ('msd_power_lds_kernel', 1),
    "k0_qr32":              ('msd_power_lds_kernel', 1),
    "k1_qr2_1":             ('msd_power_lds_kernel', 1),
    "k1_qr2_2":             ('msd_power_lds_kernel', 1),
    "k1_qr2_5":             ('msd_power_lds_kernel', 1),
    "k1_qr2_8":             ('msd_power_lds_kernel', 1),
    "k1_qr2_16":            ('msd_power_lds_kernel', 1),
    "k2_jj1_qe4":           ('msd_power_lds_kernel', 1),
    "k2_jj1_qe8":           ('msd_power_lds_kernel', 1),
    "k2_units5_5120":       ('msd_power_lds_kernel', 1),
    "k2_units8_5121":       ('msd_power_lds_kernel', 1),
    "k2_jj2_qe8":           ('msd_power_lds_kernel', 1),
    "k2_src1":              ('msd_power_lds_kernel', 1),
    "k2_src1_m13":          ('msd_power_lds_kernel', 1),
    "k2_src0":              ('msd_power_lds_kernel', 1),
    "direct_0":             ('msd_power_w12_kernel', 1),
    "direct_1":             ('msd_power_w12_kernel', 1),
    "direct_2":             ('msd_power_w12_kernel', 1),
    "direct_3":             ('msd_power_w12_kernel', 1),
    "cols_240":             ('msd_power_w12_kernel', 1),
    "empty_group":          ('msd_power_w12_kernel', 1),
    "segments_18":          ('msd_power_w12_kernel', 1),
    "d4_8193":              ('msd_power_w12p_kernel', 1),
    "d4_12288":             ('msd_power_w12p_kernel', 1),
    "d8_12289":             ('msd_power_w12p_kernel + msd_power_w12o_kernel', 1),
    "d8_24576":             ('msd_power_w12p_kernel + msd_power_w12o_kernel', 1),
    "residue_0":            ('lag_msd_fft', 1),
    "residue_2":            ('msd_power_w12r_kernel', 1),
    "residue_3_batches":    ('msd_power_w12p_kernel', 1),
    "overlap_2":            ('msd_power_w12p_kernel', 1),
    "batched_24577":        ('lag_msd_fft', 1),
    "batched_fuse_0":       ('lag_msd_fft', 1),
    "batched_fuse_1":       ('lag_msd_fft', 1),
    "batched_3_batches":    ('lag_msd_fft', 1),
    "variant_4":            ('lag_msd_fft', 1),
}


def test_lag_plan_picks_what_the_device_ran():
    """mdhip_lag_plan with the MI355X's two limits (256 CUs, 160 KB of LDS) names, for every branch of lag_choose and
    every template instance the launch code names, the kernel and the launch count the parent commit reports (see the
    table's own comment for where it comes from)."""
    import lag_plan_cases as P

    assert set(PARENT_E1B4349_REPORTS) == set(P.CASES)
    got = {name: P.plan(case) for name, case in P.CASES.items()}
    for name, (kernel, launches) in PARENT_E1B4349_REPORTS.items():
        g = got[name]
        assert g["status"] == 0 and (g["kernel"], g["launches"]) == (kernel, launches), (name, g, kernel, launches)
    # what the name alone does not show: path, generation | D | fuse level, m, source, rows per member, staging units,
    # the template instance
    f = lambda name: tuple(got[name][k] for k in ("path", "gen", "m", "source", "Fc", "units", "inst_a", "inst_b"))  # noqa: E731
    for name, d2 in (("w1_2", 1), ("w1_300", 1), ("w1_1024", 2), ("w1_1025", 3), ("w1_1535", 3)):
        assert f(name)[:2] == (P.W1, d2) and got[name]["L"] == 1024 * d2 and f(name)[6] == d2, name
    assert f("w1_ends_1536") == (P.W12, 0, 11, 2, 96, 4, 4, 1)        # SHORT, staged
    assert f("w1_off")[:4] == (P.POW2, 2, 9, 0) and f("w1_17_groups")[:4] == (P.POW2, 2, 9, 0)
    assert f("w12_short_1600")[6:] == (4, 1) and f("w12_short_3071")[6:] == (4, 1) and f("w12_qe4_3072")[6:] == (4, 0)
    assert f("w12_qe5_4097")[6:] == (5, 0) and f("w12_qe5_5000")[6:] == (5, 0) and f("w12_qe5_5120")[4:] == (320, 4, 5, 0)
    assert f("w12_qe6_5121")[4:] == (336, 4, 6, 0) and f("w12_qe6_6144")[4:] == (384, 4, 6, 0)
    for name in ("w12_short_src0", "w12_qe4_src0", "w12_qe6_src0", "direct_0", "direct_1", "cols_240", "segments_18"):
        assert f(name)[0] == P.W12 and f(name)[3] == 0 and f(name)[5] == 0, name
    assert f("direct_2")[3] == 2 and f("direct_3")[3] == 3 and f("empty_group")[3] == 2
    assert got["empty_group"]["n_items"] == 256 and got["segments_18"]["n_items"] < 256 and got["cols_240"]["n_items"] == 240
    assert f("w12_min_f_0") == (P.POW2, 3, 12, 2, 144, 5, 1, 3)
    assert f("pow2_6145") == (P.POW2, 3, 13, 2, 400, 8, 2, 4) and f("pow2_8192") == (P.POW2, 3, 13, 2, 512, 8, 2, 4)
    assert f("k0_2100")[:3] == (P.POW2, 1, 12) and f("k1_2100")[:3] == (P.POW2, 2, 12) and f("k2_2100")[:3] == (P.POW2, 3, 12)
    for name, qr in (("k0_qr1", 1), ("k0_qr2", 2), ("k0_qr4", 4), ("k0_2100", 8), ("k0_qr10", 10), ("k0_qr12", 12),
                     ("k0_qr16", 16), ("k0_qr24", 24), ("k0_qr32", 32)):
        assert f(name)[1] == 1 and f(name)[3] == 0 and f(name)[6] == qr, name
    for name, qr2 in (("k1_qr2_1", 1), ("k1_qr2_2", 2), ("k1_2100", 3), ("k1_qr2_5", 5), ("k1_qr2_8", 8), ("k1_qr2_16", 16)):
        assert f(name)[1] == 2 and f(name)[3] == 0 and f(name)[6] == qr2, name
    assert f("k2_2100")[3:] == (2, 144, 5, 1, 3) and f("k2_jj1_qe4")[3:] == (2, 256, 5, 1, 4)
    assert f("k2_jj1_qe8")[3:] == (2, 320, 5, 1, 8)
    assert f("k2_units5_5120")[3:] == (2, 320, 5, 2, 3) and f("k2_units8_5121")[3:] == (2, 336, 8, 2, 3)
    assert f("k2_jj2_qe8")[3:] == (0, 576, 0, 2, 8)
    assert f("k2_src1")[3:] == (1, 256, 0, 1, 4) and f("k2_src1_m13")[3:] == (1, 512, 0, 2, 4) and f("k2_src0")[3] == 0
    assert f("d4_8193")[:2] == (P.RESIDUE, 4) and f("d4_12288")[:2] == (P.RESIDUE, 4) and f("d4_8193")[6:] == (5, 1)
    assert f("d8_12289")[:2] == (P.RESIDUE, 8) and f("d8_24576")[:2] == (P.RESIDUE, 8) and f("d8_24576")[6:] == (6, 1)
    assert f("residue_2")[6:] == (4, 0) and f("residue_0")[:2] == (P.BATCHED, 2)
    assert got["residue_3_batches"]["n_batches"] == 3 and got["overlap_2"]["n_batches"] == 6 and got["d4_8193"]["n_batches"] == 1
    assert f("batched_24577")[:2] == (P.BATCHED, 2) and got["batched_24577"]["L"] == 65536
    assert f("batched_fuse_0")[1] == 0 and f("batched_fuse_1")[1] == 1 and got["batched_3_batches"]["n_batches"] == 3
    assert f("variant_4")[0] == P.BATCHED and got["variant_4"]["L"] == 1024
    # an unaligned trajectory cannot be staged (16-byte loads); 304 CUs are 19 clusters of 16 (288 columns are too few for
    # them, 384 are enough) but no multiple of 128
    assert P.plan(P.CASES["w12_qe5_4097"], aligned=False)["source"] == 0
    wide = lambda name: dict(P.CASES[name], E=128, go=np.array([0, 128]))  # noqa: E731
    assert P.plan(P.CASES["w12_qe5_4097"], cu_count=304)["source"] == 0 and P.plan(wide("w12_qe5_4097"), cu_count=304)["source"] == 2
    assert P.plan(wide("k2_src1"))["source"] == 1 and P.plan(wide("k2_src1"), cu_count=304)["source"] == 0
    # ... and the limits are read: a device with 64 KB of LDS loses every path whose kernels need more
    small = {name: P.plan(case, lds_bytes=65536) for name, case in P.CASES.items()}
    for name in ("w1_300", "w1_1535"):
        assert small[name]["path"] == P.POW2, name               # the one-wave kernel's 3072-point instance: 155 KB
    assert (small["w12_short_1600"]["path"], small["w12_short_1600"]["m"]) == (P.POW2, 11)  # no 12 288 points; N = 2048: 39 KB
    for name in ("w12_qe4_3072", "w12_qe5_4097", "w12_qe6_6144", "pow2_8192", "k0_qr16", "d4_8193", "d8_24576"):
        assert small[name]["path"] == P.BATCHED, (name, small[name])    # (N = 4096 needs 74 KB, the residue kernels 156 KB)
    assert small["w1_off"]["path"] == P.POW2 and small["w1_off"]["gen"] == 2   # N = 512: 12.6 KB
    # nothing spectral to plan: no frames, no entities in any group, or the exact kernels asked for
    assert P.plan(dict(P.CASES["w1_300"], F=0, max_lag=0))["path"] == -1
    assert P.plan(dict(P.CASES["w1_300"], go=np.array([0, 0])))["path"] == -1
    assert P.plan(dict(P.CASES["w1_300"], opts={"lag_variant": 1}))["path"] == -1
    unknown = P.plan(dict(P.CASES["w1_300"], opts={"no_such_option": 1}))
    assert unknown["status"] < 0 and unknown["kernel"]


def test_bench_lag_fft_plan_agrees_with_the_library():
    """bench.lag_fft_plan (the roofline's idea of the fused path: padded length and kernel) against mdhip_lag_plan for
    every fused case of the table that runs with the default kernel choice. bench.py predates the rule that sends
    2048 < F + max_lag <= 8192 with F >= 1536 to the 12 288-point kernel (lag_w12_min_f): it still prices those shapes
    as power-of-two transforms. That set is pinned here, shape by shape, so that neither side can drift unnoticed."""
    import sys

    import lag_plan_cases as P

    sys.path.insert(0, REPO)
    import bench

    name_of = {(P.W12, 0): "msd_power_w12_kernel", (P.POW2, 3): "msd_power_lds3_kernel", (P.POW2, 2): "msd_power_lds2_kernel",
               (P.POW2, 1): "msd_power_lds_kernel"}
    differ = {}
    n = 0
    for name, case in P.CASES.items():
        g = P.plan(case)
        if g["path"] not in P.FUSED or set(case["opts"]) - {"lag_direct"}:
            continue
        n += 1
        L, _, kernel = bench.lag_fft_plan(case["F"], case["max_lag"])
        if (L, kernel) != (g["L"], name_of[(g["path"], g["gen"])]):
            differ[name] = (L, kernel)
    assert n >= 20
    assert differ == {
        "w1_ends_1536": (4096, "msd_power_lds2_kernel"),
        "w12_short_1600": (4096, "msd_power_lds2_kernel"),
        "w12_short_3071": (8192, "msd_power_lds3_kernel"),
        "w12_qe4_3072": (8192, "msd_power_lds3_kernel"),
        "w12_short_src0": (4096, "msd_power_lds2_kernel"),
        "w12_qe4_src0": (8192, "msd_power_lds3_kernel"),
    }, differ


def test_row_displacement_is_the_same_in_every_process():
    """Two fresh interpreters return the same layout (no in-process cache between them, and no clock in the search):
    the nine-type reference shape and a 20-type random table (budget-limited: DESIGN 4.1f)."""
    import subprocess
    import sys

    code = ("import sys, json, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import test_abi_cpu as T\n"
            "rng = np.random.default_rng(20)\n"
            "arms = [(19, int(j)) for j in rng.permutation(19)[:12]]  # twelve random partners of one type, two random pairs\n"
            "t20 = T._tri_classes(20, arms + [(int(a), int(b)) for a, b in rng.integers(0, 19, (2, 2))])\n"
            "c1 = T._tri_classes(6, [(4, 0), (4, 2), (4, 3), (4, 4), (0, 1)])\n"
            "print(json.dumps([[r[0]] + [v.tolist() for v in r[1:]] for r in (T._displace(c1), T._displace(t20))]))\n"
            % os.path.join(REPO, "tests"))
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1]
    import json

    c1, t20 = json.loads(outs[0])
    assert 0 < c1[0] <= 18 and t20[0] > 0
