"""
The shapes the pair-plan tests walk through (tests/test_abi_cpu.py: mdhip_pair_plan against kernel names recorded on
the device; tests/test_gpu_hardening.py: the plan against what a real call leaves in last_kernel_name()).

A case is a dict: op ("rdf", "rdf_dev", "cn", "rdf_cn", "rdf_sites", "cn_sites"), frames F, atoms n, box length L,
the type column `types`, relations `rel`, r_cut / bin / nbins, coordination cutoffs `cuts`, per_frame, sites m and
their types `site_types`, option overrides `opts`, `dev` (coordinates handed over as a device tensor).
`plan(case, ...)` asks the library what it would launch; `run(case, B)` makes the call on random positions.
"""
import ctypes as C

import numpy as np

from mdproptools_amd import _lib, synth

OPS = {"rdf": 0, "rdf_dev": 0, "rdf_sites": 0, "cn": 1, "cn_sites": 1, "rdf_cn": 2}
INFO = ("status", "sj_mode", "n_pass", "launches", "ord_rows", "displaced", "big", "packed")
TWO_SWEEPS = 1  # status: an RDF + CN call that does not run as one sweep


def _case(op, F, n, L, types, rel, r_cut=10.0, bin=0.05, nbins=None, cuts=None, per_frame=False, m=0, site_types=None,
          opts=None, dev=False):
    rel = np.array(rel, dtype=np.int32).reshape(-1, 2)
    if op in ("cn", "cn_sites", "rdf_cn") and cuts is None:
        cuts = synth.cn_cutoffs(len(rel))
    return dict(op=op, F=F, n=n, L=float(L), types=np.asarray(types, np.int32), rel=rel, r_cut=r_cut, bin=bin,
                nbins=int(r_cut / bin) if nbins is None else nbins, cuts=cuts, per_frame=per_frame, m=m,
                site_types=None if site_types is None else np.asarray(site_types, np.int32), opts=dict(opts or {}),
                dev=dev)


def _types(n, k):
    return synth.rdf_types(n, k)


def _all_pairs(k):
    return [(a, b) for a in range(1, k + 1) for b in range(a, k + 1)]


P3 = [(1, 1), (1, 2), (2, 3), (3, 3)]
C1N, C1L = synth.C1_ATOMS, synth.C1_BOX
STAR5 = [(5, 1), (5, 2), (5, 3), (5, 4)]  # five named types, four relations: displaced rows have fewer rows


def _base(op="rdf", **kw):
    """4000 atoms of three types in a 40 A box, r_cut 10 A: 16 tiles, culled, packed ordered rows."""
    a = dict(F=4, n=4000, L=40.0, types=_types(4000, 3), rel=P3)
    a.update(kw)
    return _case(op, **a)


def _c1(rel, F=8, **kw):
    return _case("rdf", F, C1N, C1L, synth.c1_types(False), rel, 20.0, **kw)


CASES = {
    # bench.py's headline and its --shape variants
    "C2": _case("rdf_dev", 200, 10_000, 50.0, _types(10_000, 4), synth.ALL_PAIRS_4, 20.0, dev=True),
    "C1": _c1(synth.C1_RELATIONS, F=200, dev=True),
    "C1alt": _case("rdf", 200, C1N, C1L, synth.c1_types(True), synth.C1_ALT_RELATIONS, 20.0, dev=True),
    "C1full": _c1(_all_pairs(9), F=200, dev=True),
    # the C3 leg (fewer frames: the decision reads sizes per frame, the batch stays one)
    "C3_rdf": _case("rdf", 32, 100_000, 104.0, _types(100_000, 4), synth.ALL_PAIRS_4, 20.0, dev=True),
    "C3_cn": _case("cn", 32, 100_000, 104.0, _types(100_000, 4), synth.ALL_PAIRS_4, 20.0, dev=True),
    "C3_rdf_cn": _case("rdf_cn", 32, 100_000, 104.0, _types(100_000, 4), synth.ALL_PAIRS_4, 20.0, dev=True),
    # atoms x sites
    "sites_rdf": _base("rdf_sites", m=2000, site_types=_types(2000, 2), rel=[(1, 1), (2, 2), (3, 1)]),
    "sites_cn": _base("cn_sites", m=2000, site_types=_types(2000, 2), rel=[(1, 1), (2, 2), (3, 1)]),
    # the branches of the decision
    "base": _base(),
    "base_cn": _base("cn"),
    "base_rdf_cn": _base("rdf_cn"),
    "dense_small_frame": _base(n=1500, types=_types(1500, 3)),
    "few_bins_edge_table": _base(nbins=150),
    "cn_70_cutoffs": _base("cn", rel=[P3[k % 4] for k in range(70)], cuts=[2.0 + 0.1 * k for k in range(70)]),
    "cutoff_inside_bin": _base(r_cut=10.02, nbins=200),
    "cutoff_inside_bin_rows": _base(r_cut=10.02, nbins=200, opts={"rdf_rows": 0}),
    "per_frame": _base(per_frame=True),
    "device_result": _base("rdf_dev", dev=True),
    "device_result_small_frame": _base("rdf_dev", dev=True, n=1500, types=_types(1500, 3)),
    "twelve_types_all_pairs": _base(L=50.0, r_cut=16.0, bin=0.04, types=_types(4000, 12), rel=_all_pairs(12)),
    "box_4000": _base(L=4000.0),
    "cn_beyond_r_cut": _base("rdf_cn", cuts=[3.0, 4.0, 12.0, 5.0]),
    "cn_two_cutoffs_one_class": _base("rdf_cn", rel=P3 + [(2, 1)], cuts=[3.0, 4.0, 5.0, 6.0, 4.5]),
    "host_batches": _base(F=40),
    # one option each, on a shape where it changes the answer
    "rdf_pk_0": _base(opts={"rdf_pk": 0}),
    "rdf_pk_2": _base(opts={"rdf_pk": 2}),
    "rdf_sj_0": _base(opts={"rdf_sj": 0}),
    "rdf_sj_2": _base(opts={"rdf_sj": 2}),
    "rdf_cull_0": _base(opts={"rdf_cull": 0}),
    "dense_box": _base(L=24.0),
    "rdf_cull_1": _base(L=24.0, opts={"rdf_cull": 1}),
    "rdf_rows_0": _base(opts={"rdf_rows": 0}),
    "c1_small": _c1(synth.C1_RELATIONS),
    "rdf_disp_0": _c1(synth.C1_RELATIONS, opts={"rdf_disp": 0}),
    "star5": _base(types=_types(4000, 7), rel=STAR5),
    "rdf_disp_2": _base(types=_types(4000, 7), rel=STAR5, opts={"rdf_disp": 2}),
    "c1full_small": _c1(_all_pairs(9)),
    "rdf_big_0": _c1(_all_pairs(9), opts={"rdf_big": 0}),
    "rdf_pk_passes_0": _base(L=50.0, r_cut=16.0, bin=0.04, types=_types(4000, 12), rel=_all_pairs(12),
                             opts={"rdf_pk_passes": 0}),
    "rdf_variant_0": _base(opts={"rdf_variant": 0}),
    "cn_pk_0": _base("cn", opts={"cn_pk": 0}),
}


def plan(case, cu_count=256, lds_bytes=163840, ctx=None):
    """mdhip_pair_plan for `case` -> dict(kernel=..., **INFO). `ctx`: a context whose options and device limits are
    used instead of the defaults, cu_count and lds_bytes (pass 0 for the two)."""
    lib = _lib.load()
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    box = np.full((case["F"], 3), case["L"])
    ty = np.unique(case["types"]).astype(np.int32)
    st = np.unique(case["site_types"]).astype(np.int32) if case["m"] else None
    rel = np.ascontiguousarray(case["rel"], dtype=np.int32)
    cuts = None if case["cuts"] is None else np.array([c * c for c in case["cuts"]], dtype=np.float64)
    keys = (C.c_char_p * max(1, len(case["opts"])))(*[k.encode() for k in case["opts"]])
    vals = (C.c_int * max(1, len(case["opts"])))(*case["opts"].values())
    name = C.create_string_buffer(512)
    info = np.zeros(len(INFO), np.int32)
    rc = lib.mdhip_pair_plan(None if ctx is None else ctx.h, OPS[case["op"]], case["F"], case["n"], ip(ty), len(ty),
                             case["m"], None if st is None else ip(st), 0 if st is None else len(st), dp(box), len(rel), ip(rel), case["r_cut"] * case["r_cut"],
                             case["bin"], case["nbins"], None if cuts is None else dp(cuts), int(case["per_frame"]),
                             int(case["op"] == "rdf_dev"), int(case["dev"]), cu_count, lds_bytes, len(case["opts"]),
                             keys, vals, name, len(name), ip(info))
    assert rc == 0, (rc, name.value)
    out = dict(zip(INFO, (int(v) for v in info)))
    out["kernel"] = name.value.decode()
    return out


def run(case, B, ctx, seed=11):
    """The real call for `case` on uniformly random positions -> (inputs, outputs); the context's options are the case's."""
    import torch

    rng = np.random.default_rng(seed)
    F, n, L = case["F"], case["n"], case["L"]
    for k, v in case["opts"].items():
        ctx.set_option(k, v)
    xyz = rng.random((F, 3, n)) * L
    box = np.full((F, 3), L)
    x_in = torch.from_numpy(xyz).cuda() if case["dev"] else xyz
    ty, rel, op = case["types"], case["rel"], case["op"]
    inp = dict(xyz=xyz, box=box)
    if op == "rdf":
        out = B.rdf_loop(x_in, ty, box, rel, case["r_cut"], case["bin"], case["nbins"], per_frame=case["per_frame"], ctx=ctx)
    elif op == "rdf_dev":
        words = (1 + len(rel)) * case["nbins"] + 1
        buf = torch.zeros(words, dtype=torch.int64, device="cuda")
        B.rdf_loop_dev(x_in, ty, box, rel, case["r_cut"], case["bin"], case["nbins"], buf, ctx=ctx)
        ctx.sync()
        out = buf.cpu().numpy().view(np.uint64)
    elif op == "cn":
        out = B.cn_loop(x_in, ty, box, rel, case["cuts"], per_frame=case["per_frame"], ctx=ctx)
    elif op == "rdf_cn":
        out = B.rdf_cn_loop(x_in, ty, box, rel, case["r_cut"], case["bin"], case["nbins"], case["cuts"],
                            per_frame=case["per_frame"], ctx=ctx)
    else:
        sites = rng.random((F, 3, case["m"])) * L
        inp["sites"] = sites
        if op == "rdf_sites":
            out = B.rdf_mol_loop(x_in, ty, sites, case["site_types"], box, rel, case["r_cut"], case["bin"], case["nbins"],
                                 per_frame=case["per_frame"], ctx=ctx)
        else:
            out = B.cn_mol_loop(x_in, ty, sites, case["site_types"], box, rel, case["cuts"], per_frame=case["per_frame"],
                                ctx=ctx)
    return inp, out


def check_against_oracle(case, inp, out, O):
    """The frame-summed result of run(case, ...) against the C oracle `O` (oracle.cref), every frame of it."""
    F, L, nb, rel, ty = case["F"], [case["L"]] * 3, case["nbins"], case["rel"], case["types"]
    rc2 = case["r_cut"] * case["r_cut"]
    assert not case["per_frame"]
    op = case["op"]
    full, part, ov = np.zeros(nb, np.uint64), np.zeros((len(rel), nb), np.uint64), 0
    cn = np.zeros(len(rel), np.uint64)
    cuts2 = None if case["cuts"] is None else [c * c for c in case["cuts"]]
    for f in range(F):
        x = inp["xyz"][f]
        if op in ("rdf", "rdf_dev", "rdf_cn"):
            cf, cp, cov = O.rdf_pairs(x, ty, rel, L, rc2, case["bin"], nb)
            full, part, ov = full + cf, part + cp, ov + int(cov)
        if op in ("cn", "rdf_cn"):
            cn = cn + O.cn_pairs(x, ty, rel, L, cuts2)
        if op == "rdf_sites":
            cp, cov = O.rdf_rect(x, ty, inp["sites"][f], case["site_types"], rel, L, rc2, case["bin"], nb)
            part, ov = part + cp, ov + int(cov)
        if op == "cn_sites":
            cn = cn + O.cn_rect(x, ty, inp["sites"][f], case["site_types"], rel, L, cuts2)
    if op == "rdf_dev":
        np.testing.assert_array_equal(out, np.concatenate([full, part.ravel(), [ov]]).astype(np.uint64))
    elif op == "rdf":
        np.testing.assert_array_equal(out[0], full)
        np.testing.assert_array_equal(out[1], part)
        assert out[2] == ov
    elif op == "rdf_cn":
        np.testing.assert_array_equal(out[0], full)
        np.testing.assert_array_equal(out[1], part)
        assert out[2] == ov
        np.testing.assert_array_equal(out[3], cn)
    elif op == "rdf_sites":
        np.testing.assert_array_equal(out[0], part)
        assert out[1] == ov
    else:
        np.testing.assert_array_equal(out, cn)
