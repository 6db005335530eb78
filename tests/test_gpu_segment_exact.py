"""
Per-molecule COM (mdhip_segment_com) and charge flux (mdhip_charge_flux) bit for bit against the stated arithmetic
(tests/segment_exact.py) on every kernel variant the dispatch can pick: each segment table of segment_exact.py under
every option set below, host and device input (a device view 8 bytes off 16-byte alignment among them), host and
device output, and the asynchronous twin the first time a kernel is met. The set of kernels reached is asserted, not
assumed; so is the load form (16-byte or 8-byte loads) each staged / by-frame instantiation met.

Then the molecular histograms on the device COM: the library's route (segment_com, then rdf_mol_loop / cn_mol_loop) gives
the C oracle's integers for sites computed by the restatement, on a geometry whose sites sit within ulps of bin edges
and CN cutoffs, and on the C1 golden frame.
"""
import numpy as np
import pytest

import segment_exact as X
from conftest import sorted_frame
from oracle import cpu_ref as O
from oracle import cref as C

pytestmark = pytest.mark.gpu

FALLBACK = X.FALLBACK
ALL_KERNELS = {FALLBACK[False], FALLBACK[True]} | {
    "segment_frame_kernel<%s, %d>" % (fl, cap) for fl in ("false", "true") for cap in (512, 1024)} | {
    "segment_staged_kernel<%s, %s>" % (fl, g) for fl in ("false", "true") for g in ("256, 64", "512, 256", "1024, 256")}
DEFAULTS = dict(seg_frame=1, seg_cap=0, seg_vec=1, seg_gy=0)
CONFIGS = X.CONFIGS
FORMS = ("host", "dev", "dev_odd")


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


def _on(x, form):
    """x as the library receives it: the host array, a device tensor, or a contiguous device view at storage offset 1
    (data pointer 8 bytes off 16-byte alignment)."""
    if form == "host":
        return x
    import torch

    t = torch.from_numpy(np.ascontiguousarray(x))
    if form == "dev":
        return t.cuda()
    buf = torch.empty(x.size + 1, dtype=torch.float64, device="cuda")
    v = buf[1:].view(x.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 == 8
    return v


def _host(r):
    return r.cpu().numpy() if hasattr(r, "cpu") else r


def _loads16(kernel, n_atoms, form, seg_vec):
    """Whether some block of the call takes 16-byte loads: an even atom count (the first run starts at atom 0) and a
    16-byte aligned input; the staged kernel also needs seg_vec. None: the one-lane-per-segment fallbacks."""
    if kernel in FALLBACK.values():
        return None
    ok = n_atoms % 2 == 0 and form != "dev_odd"
    return ok and (bool(seg_vec) or kernel.startswith("segment_frame_kernel"))


def test_segment_com_and_flux_bit_exact_on_every_variant(B):
    import torch

    ctx = B.default_context()
    tables = dict(X.segment_tables())
    t_sizes, t_st, t_T = X.type_table()
    tables["types"] = t_sizes
    seen, loads, twins, bad = set(), set(), set(), []

    def check(got, want, what):
        if not np.array_equal(got, want):
            d = np.nonzero(got != want)
            bad.append("%s: %d of %d differ, first at %s: %r != %r" % (
                what, len(d[0]), want.size, tuple(int(i[0]) for i in d), got[d][0], want[d][0]))

    def note(kernel, want_kernel, n_atoms, form, cfg, what):
        seen.add(kernel)
        if want_kernel is not None and kernel != want_kernel:
            bad.append("%s: kernel %s, the dispatch should have picked %s" % (what, kernel, want_kernel))
        lf = _loads16(kernel, n_atoms, form, cfg[2])
        if lf is not None:
            loads.add((kernel, lf))

    try:
        for ti, (name, sizes) in enumerate(sorted(tables.items())):
            off = X.offsets(sizes)
            N, M = int(off[-1]), len(sizes)
            m, q = X.case_masses(name, off)
            st, T = (t_st, t_T) if name == "types" else X.seg_types(M)
            w_mass, w_q = X.seg_sums(m, q, off)
            for F in (X.FRAMES, X.MANY_FRAMES) if name in X.MANY_TABLES else (X.FRAMES,):
                Ks = X.N_ATTR if F == X.FRAMES else (3,)
                com_cases = {K: X.case_attr(name, off, F, K) for K in Ks}
                com_want = {K: X.com(a, m, off) for K, a in com_cases.items()}
                vel = X.case_vel(name, off, F)
                flux_want = X.flux(vel, m, q, off, st, T)
                for ci, cfg in enumerate(CONFIGS):
                    for key, val in zip(("seg_frame", "seg_cap", "seg_vec", "seg_gy"), cfg):
                        ctx.set_option(key, val)
                    for ki, K in enumerate(Ks):
                        form = FORMS[(ti + ci + ki) % 3]
                        out_dev = (ci + ki) % 2 == 1
                        what = "COM %s F=%d K=%d %s %s out=%s" % (name, F, K, cfg, form, "dev" if out_dev else "host")
                        want_kernel = X.expected_kernel(False, cfg, sizes, name, K)
                        for async_ in (False, True):
                            out = torch.empty((F, K, M), dtype=torch.float64, device="cuda") if out_dev else None
                            r = B.segment_com(_on(com_cases[K], form), m, off, atom_q=q, out=out, ctx=ctx, async_=async_)
                            if async_:
                                r, kernel = r.wait(), r.stats()[3]
                            else:
                                kernel = ctx.last_kernel_name()
                            com, seg_mass, seg_q = r
                            tag = what + (" async" if async_ else "")
                            note(kernel, want_kernel, N, form, cfg, tag)
                            check(_host(com), com_want[K], tag)
                            check(seg_mass, w_mass, tag + " seg_mass")
                            check(seg_q, w_q, tag + " seg_q")
                            if kernel in twins:
                                break
                            twins.add(kernel)
                    form = FORMS[(ti + ci + 1) % 3]
                    out_dev = ci % 2 == 0
                    what = "flux %s F=%d %s %s out=%s" % (name, F, cfg, form, "dev" if out_dev else "host")
                    want_kernel = X.expected_kernel(True, cfg, sizes, name, 3)
                    for async_ in (False, True):
                        out = torch.empty((3, T, F), dtype=torch.float64, device="cuda") if out_dev else None
                        r = B.charge_flux(_on(vel, form), m, q, off, st, T, X.VEL_CONV, X.CHARGE_CONV, ctx=ctx, out=out,
                                          async_=async_)
                        if async_:
                            r, kernel = r.wait(), r.stats()[3]
                        else:
                            kernel = ctx.last_kernel_name()
                        tag = what + (" async" if async_ else "")
                        note(kernel, want_kernel, N, form, cfg, tag)
                        check(_host(r), flux_want, tag)
                        if kernel in twins:
                            break
                        twins.add(kernel)
    finally:
        for key, val in DEFAULTS.items():
            ctx.set_option(key, val)
    assert not bad, "%d mismatches:\n" % len(bad) + "\n".join(bad[:40])
    assert seen == ALL_KERNELS, (sorted(ALL_KERNELS - seen), sorted(seen - ALL_KERNELS))
    assert twins == ALL_KERNELS
    staged_or_frame = ALL_KERNELS - set(FALLBACK.values())
    assert loads == {(k, lf) for k in staged_or_frame for lf in (False, True)}, sorted(
        {(k, lf) for k in staged_or_frame for lf in (False, True)} - loads)


def _device_route(B, g):
    """Library: COM on the device into a device tensor, then the atoms x sites histogram and CN from it."""
    import torch

    F, _, _ = g["attr"].shape
    sites = torch.empty((F, 3, len(g["off"]) - 1), dtype=torch.float64, device="cuda")
    B.segment_com(g["attr"], g["mass"], g["off"], out=sites)
    L = np.asarray(g["lengths"])[None]
    part, ov = B.rdf_mol_loop(g["xyz"], g["types"], sites, g["site_types"], L, g["rel"], g["r_cut"], g["ddr"],
                              g["nbins"])
    cn = B.cn_mol_loop(g["xyz"], g["types"], sites, g["site_types"], L, g["rel"], g["cn_cut"])
    return part[0], int(np.asarray(ov).sum()), cn[0], sites.cpu().numpy()


def _oracle_route(g):
    """C oracle on the sites of the stated arithmetic."""
    sites = X.com(g["attr"], g["mass"], g["off"])
    part, ov = C.rdf_rect(g["xyz"][0], g["types"], sites[0], g["site_types"], g["rel"], g["lengths"],
                          g["r_cut"] * g["r_cut"], g["ddr"], g["nbins"])
    cn = C.cn_rect(g["xyz"][0], g["types"], sites[0], g["site_types"], g["rel"], g["lengths"],
                   [c * c for c in g["cn_cut"]])
    return part, ov, cn, sites


def _c1(g_c1):
    g = g_c1
    fr = sorted_frame(g["frames"][0])
    _, _, off, seg_type = O.molecule_layout(g["num_mols"], g["num_atoms_per_mol"])
    xyz = np.ascontiguousarray(fr[:, 2:5].T)[None]
    return dict(xyz=xyz, types=fr[:, 1].astype(np.int32), attr=xyz, mass=g["mass"][fr[:, 1].astype(np.int64) - 1],
                off=off, site_types=seg_type.astype(np.int32), lengths=g["bounds"][0][:, 1] - g["bounds"][0][:, 0],
                rel=g["mol_rel"].T, r_cut=20.0, ddr=0.05, nbins=400, cn_cut=list(g["mol_cn_cut"]))


@pytest.mark.parametrize("case", ["edges", "c1"])
def test_molecular_histograms_on_device_com_exact(B, g_c1, case):
    """Sites within ulps of bin edges and CN cutoffs (tests/test_segment_exact_cpu.py shows that they move when the COM
    is summed in another order): the device-COM route gives the oracle's integers for the restatement's sites."""
    g = X.edge_geometry() if case == "edges" else _c1(g_c1)
    part, ov, cn, sites = _device_route(B, g)
    w_part, w_ov, w_cn, w_sites = _oracle_route(g)
    np.testing.assert_array_equal(sites, w_sites)
    assert ov == w_ov
    np.testing.assert_array_equal(part.astype(np.int64), w_part.astype(np.int64))
    np.testing.assert_array_equal(cn.astype(np.int64), w_cn.astype(np.int64))
