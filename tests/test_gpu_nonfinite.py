"""
Non-finite input on the GPU: NaN, +-Inf and a finite 1e300 in a coordinate or sample, in every kernel family, against
the reference's answer (include/mdhip.h, "Non-finite input"; the patterns and placements: tests/nonfinite_cases.py; the
CPU side of the same statements: tests/test_nonfinite_cpu.py).

  * pair counts (RDF, CN, the one-sweep call, atoms x sites, shell members, shell coordination, contact components,
    shell residence): a poisoned frame gives the integers of the C oracle / the numpy restatement on that same input,
    which are the integers of the frame with the poisoned atoms DELETED (or, where indices must stay, moved out of reach);
  * sums (segment COM, charge flux, MSD, full-lag MSD, correlations, integrals): the outputs the poisoned value enters are
    non-finite exactly where plain numpy sums make them so, every other output is bit-identical to the clean call.

Every case names the kernel it ran (last_kernel_name, for the pair histograms against mdhip_pair_plan too), so that a
case cannot quietly test another kernel. The dense pair sweep runs before the culled and the packed ones.
"""
import contextlib
import warnings

import numpy as np
import pytest

import aggregates_ref as AR
import angular_ref as ANG
import cluster_ref as CR
import config_ref as CFG
import lag_exact as LX
import nonfinite_cases as NF
import pair_plan_cases as P
import residence_design as RD
import segment_exact as SX
from oracle import cref as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ctx(B):
    return B.default_context()


@pytest.fixture(autouse=True)
def _quiet():
    """inf - inf and NaN comparisons in the numpy references are the subject here."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


@contextlib.contextmanager
def options(ctx, restore=-1, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, restore[k] if isinstance(restore, dict) else restore)


def _cuda(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _mask_within(got, touched, what=""):
    """Every non-finite output lies inside `touched`, and `touched` (where there is any) holds one. Which entries exactly
    is pinned by the comparison with the numpy reference; this states where they may be."""
    bad = ~np.isfinite(got)
    assert not (bad & ~np.broadcast_to(touched, got.shape)).any(), what
    assert bad.any() == bool(np.any(touched)), what


def _untouched_equal(got, clean, touched, what):
    """Outside `touched` (bool, broadcastable) the poisoned call's output is the clean call's, bit for bit; inside it
    nothing is asserted here."""
    keep = ~np.broadcast_to(touched, got.shape)
    assert np.array_equal(got[keep], clean[keep]), what


# ================================================================================================ 1. pair histograms
N_PAIR, L_PAIR, F_PAIR = 2100, 25.0, 8  # 9 tiles of 256 (the last one partial); rdf_cull forced as test_gpu_pair_image
M_SITES = 700
CUTS3 = [3.0, 9.975, 6.2, 9.99]  # coordination cutoffs (one inside a bin next to the cutoff, as test_gpu_pair_image)


def _types(n, k):
    from mdproptools_amd import synth

    return synth.rdf_types(n, k)


def _pc(op="rdf", k_types=3, rel=P.P3, opts=None, **kw):
    o = {"rdf_cull": 1}
    o.update(opts or {})
    a = dict(F=F_PAIR, n=N_PAIR, L=L_PAIR, types=_types(N_PAIR, k_types), rel=rel, r_cut=10.0, bin=0.05, per_frame=True,
             opts=o)
    a.update(kw)
    if op in ("cn", "cn_sites", "rdf_cn"):
        a.setdefault("cuts", [CUTS3[k % 4] for k in range(len(a["rel"]))])
    return P._case(op, **a)


def _sites(**kw):
    return dict(m=M_SITES, site_types=_types(M_SITES, 2), rel=[(1, 1), (2, 2), (3, 1)], **kw)


# name -> (case, what mdhip_pair_plan must say about it). The dense cases come first.
PAIR_CASES = {
    "dense_fast": (_pc(opts={"rdf_cull": 0}), dict(sj_mode=-1, kernel="pair_hist_fast_kernel<true, 8, 0, false>")),
    "dense_plain": (_pc(opts={"rdf_cull": 0, "rdf_variant": 0}), dict(sj_mode=-1, kernel="pair_hist_kernel<true>")),
    "dense_sum": (_pc(opts={"rdf_cull": 0}, per_frame=False), dict(sj_mode=-1)),
    "dense_cn": (_pc("cn", opts={"rdf_cull": 0}), dict(sj_mode=-1)),
    "dense_rdf_cn": (_pc("rdf_cn", opts={"rdf_cull": 0}), dict(sj_mode=-1)),
    "dense_sites": (_pc("rdf_sites", opts={"rdf_cull": 0}, **_sites()), dict(sj_mode=-1)),
    "dense_cn_sites": (_pc("cn_sites", opts={"rdf_cull": 0}, **_sites()), dict(sj_mode=-1)),
    "lds_tile_culled": (_pc(opts={"rdf_sj": 0}), dict(sj_mode=-1, kernel="pair_hist_fast_kernel<true, 8, 0, true>")),
    "sj_f64_ordered": (_pc(opts={"rdf_pk": 0}), dict(sj_mode=2, packed=0)),
    "sj_f64_ordered_sj2": (_pc(opts={"rdf_sj": 2, "rdf_pk": 0}), dict(sj_mode=2, packed=0)),
    "sj_f64_class_rows": (_pc(opts={"rdf_rows": 0, "rdf_pk": 0}), dict(sj_mode=0, packed=0)),
    "sj_f64_sum": (_pc(opts={"rdf_pk": 0}, per_frame=False), dict(sj_mode=2, packed=0)),
    "packed": (_pc(), dict(sj_mode=3, packed=1, big=0, displaced=0)),
    "packed_sj2": (_pc(opts={"rdf_sj": 2}), dict(sj_mode=3, packed=1)),
    "packed_sum": (_pc(per_frame=False), dict(sj_mode=3, packed=1, kernel="pair_hist_sj_kernel<3, true, false>")),
    "packed_device_input": (_pc(dev=True), dict(sj_mode=3, packed=1)),
    "packed_frame_types": (_pc(), dict(sj_mode=3, packed=1)),
    "packed_cut_inside_bin": (_pc(r_cut=10.02, nbins=200), dict(sj_mode=4, packed=1)),
    "packed_class_rows": (_pc(opts={"rdf_rows": 0}), dict(sj_mode=5, packed=1)),
    "packed_class_rows_cut": (_pc(r_cut=10.02, nbins=200, opts={"rdf_rows": 0}), dict(sj_mode=6, packed=1)),
    "packed_displaced": (_pc(k_types=7, rel=P.STAR5, opts={"rdf_disp": 2}), dict(sj_mode=3, packed=1, displaced=1)),
    "packed_big_block": (_pc(k_types=9, rel=P._all_pairs(9), L=41.0, r_cut=20.0), dict(sj_mode=3, packed=1, big=1)),
    "packed_big_block_sum": (_pc(k_types=9, rel=P._all_pairs(9), L=41.0, r_cut=20.0, per_frame=False),
                             dict(sj_mode=3, packed=1, big=1)),
    "packed_nine_types_class_rows": (_pc(k_types=9, rel=P._all_pairs(9), opts={"rdf_big": 0}), dict(sj_mode=5, packed=1)),
    "packed_class_rows_passes": (_pc(k_types=12, rel=P._all_pairs(12), bin=0.025), dict(sj_mode=5, packed=1, n_pass=4)),
    "f64_class_rows_passes": (_pc(k_types=12, rel=P._all_pairs(12), bin=0.025, opts={"rdf_pk_passes": 0}),
                              dict(sj_mode=0, packed=0, n_pass=3)),
    "sort_global_counters": (_pc(opts={"rdf_sort": 0}), dict(sj_mode=3, packed=1)),
    "sort_one_block": (_pc(opts={"rdf_sort": 1}), dict(sj_mode=3, packed=1)),
    "sort_loop_form": (_pc(opts={"rdf_sort": 3}), dict(sj_mode=3, packed=1)),
    "cn_packed": (_pc("cn"), dict(sj_mode=3, packed=1, kernel="pair_hist_sj_kernel<3, false, true>")),
    "cn_f64": (_pc("cn", opts={"cn_pk": 0}), dict(sj_mode=1, packed=0)),
    "cn_sum": (_pc("cn", per_frame=False), dict(sj_mode=3, packed=1)),
    "rdf_cn_one_sweep": (_pc("rdf_cn"), dict(status=0, sj_mode=3, packed=1, kernel="pair_hist_sj_kernel<3, false, true>")),
    "rdf_cn_one_sweep_sum": (_pc("rdf_cn", per_frame=False), dict(status=0, sj_mode=3, packed=1)),
    "rdf_cn_two_sweeps": (_pc("rdf_cn", opts={"rdf_pk": 0}), dict(status=P.TWO_SWEEPS, sj_mode=2)),
    "sites_packed": (_pc("rdf_sites", **_sites()), dict(sj_mode=3, packed=1)),
    "sites_f64": (_pc("rdf_sites", opts={"rdf_pk": 0}, **_sites()), dict(sj_mode=2, packed=0)),
    "sites_sum": (_pc("rdf_sites", per_frame=False, **_sites()), dict(sj_mode=3, packed=1)),
    "cn_sites": (_pc("cn_sites", **_sites()), dict(sj_mode=1)),
}
_REFS = {}


def _cuts(case):
    return list(case["cuts"]) if case["cuts"] is not None else [CUTS3[k % 4] for k in range(len(case["rel"]))]


def _pair_scene(case, name, need=("rdf",)):
    """Positions, the poison plan and the references of one case; cached by what they depend on. The oracle's histograms
    ("rdf") and coordination numbers ("cn") are computed when first asked for: on the poisoned frame and on the frame
    with the poisoned atoms deleted, which must agree, and (histograms) on the clean frame, which must differ."""
    sites = case["m"] > 0
    frame_types = name == "packed_frame_types"
    key = (case["n"], case["L"], case["types"].tobytes(), case["rel"].tobytes(), case["r_cut"], case["bin"],
           case["nbins"], case["m"], tuple(_cuts(case)), frame_types)
    n, L, F = case["n"], case["L"], case["F"]
    if key not in _REFS:
        clean = NF.uniform_frames(9100 + n + int(L), F, n, L)
        plan = NF.schedule(n, F - 1) + [("nan_all_axes", NF.places(n))]  # the last frame: NaN at every placement
        assert len(plan) == F
        ty = case["types"]
        if frame_types:
            rng = np.random.default_rng(9101)
            ty = np.stack([rng.permutation(case["types"]) for _ in range(F)]).astype(np.int32)
        s = dict(box=np.full((F, 3), L), types=ty, cuts=_cuts(case), plan=plan, clean=clean)
        if sites:
            s_clean = NF.uniform_frames(9200 + n, F, case["m"], L)
            s_clean[:, :, :30] = clean[:, :, :30]  # coincident points
            # odd frames carry their poison in an atom, even frames in a site
            s["s_plan"] = [None] + [(p[0], tuple(sorted({a % case["m"] for a in p[1]}))) if f % 2 == 0 else None
                                    for f, p in enumerate(plan[1:], 1)]
            s["a_plan"] = [None] + [p if f % 2 == 1 else None for f, p in enumerate(plan[1:], 1)]
            s.update(xyz=NF.trajectory(clean, s["a_plan"]), sites=NF.trajectory(s_clean, s["s_plan"]), s_clean=s_clean)
        else:
            s["xyz"] = NF.trajectory(clean, plan)
        _REFS[key] = s
    s = _REFS[key]
    box, ty, clean, plan = s["box"], s["types"], s["clean"], s["plan"]
    ty_of = (lambda f: ty[f]) if frame_types else (lambda f: ty)
    rel, rc2, ddr, nb = case["rel"], case["r_cut"] ** 2, case["bin"], case["nbins"]
    c2 = [c * c for c in s["cuts"]]

    def deleted(f):
        """Frame f without its poisoned atoms / sites: (x, types, sites, site types)."""
        if sites:
            x, t, y, u = clean[f], ty, s["s_clean"][f], case["site_types"]
            if s["a_plan"][f]:
                x, t = NF.delete(clean[f], ty, s["a_plan"][f][1])
            if s["s_plan"][f]:
                y, u = NF.delete(s["s_clean"][f], u, s["s_plan"][f][1])
            return x, t, y, u
        t = ty_of(f)
        return ((clean[f], t) if plan[f] is None else NF.delete(clean[f], t, plan[f][1])) + (None, None)

    if "rdf" in need and "part" not in s:
        full, part, ov = [], [], 0
        for f in range(F):
            x, t, y, u = deleted(f)
            if sites:
                st = case["site_types"]
                p_bad, o_bad = C.rdf_rect(s["xyz"][f], ty, s["sites"][f], st, rel, box[f], rc2, ddr, nb)
                p_del, o_del = C.rdf_rect(x, t, y, u, rel, box[f], rc2, ddr, nb)
                f_bad = f_del = p_bad.sum(axis=0)
                f_clean = C.rdf_rect(clean[f], ty, s["s_clean"][f], st, rel, box[f], rc2, ddr, nb)[0].sum(axis=0) if f else None
            else:
                f_bad, p_bad, o_bad = C.rdf_pairs(s["xyz"][f], ty_of(f), rel, box[f], rc2, ddr, nb)
                f_del, p_del, o_del = C.rdf_pairs(x, t, rel, box[f], rc2, ddr, nb)
                f_clean = C.rdf_pairs(clean[f], ty_of(f), rel, box[f], rc2, ddr, nb)[0] if f else None
                for a in (plan[f][1] if f else ()):  # every poisoned atom had a neighbour inside the cutoff
                    r = CR.rsq(clean[f][:, a], clean[f], box[f])
                    r[a] = np.inf
                    assert (r < rc2).any(), (f, a)
            assert np.array_equal(f_bad, f_del) and np.array_equal(p_bad, p_del) and o_bad == o_del, f
            assert f == 0 or not np.array_equal(f_bad, f_clean), f  # the case tests something
            full.append(f_bad), part.append(p_bad)
            ov += o_bad
        s.update(full=np.stack(full), part=np.stack(part), ov=ov)
    if "cn" in need and "cn" not in s:
        cn = []
        for f in range(F):
            x, t, y, u = deleted(f)
            if sites:
                st = case["site_types"]
                c_bad = C.cn_rect(s["xyz"][f], ty, s["sites"][f], st, rel, box[f], c2)
                c_del = C.cn_rect(x, t, y, u, rel, box[f], c2)
                c_clean = C.cn_rect(clean[f], ty, s["s_clean"][f], st, rel, box[f], c2)
            else:
                c_bad = C.cn_pairs(s["xyz"][f], ty_of(f), rel, box[f], c2)
                c_del = C.cn_pairs(x, t, rel, box[f], c2)
                c_clean = C.cn_pairs(clean[f], ty_of(f), rel, box[f], c2)
            assert np.array_equal(c_bad, c_del), f
            assert f == 0 or not np.array_equal(c_bad, c_clean), f
            cn.append(c_bad)
        s["cn"] = np.stack(cn)
    return s


NEED = {"rdf": ("rdf",), "rdf_sites": ("rdf",), "cn": ("cn",), "cn_sites": ("cn",), "rdf_cn": ("rdf", "cn")}


@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_pair_histograms_poisoned_atoms_are_in_no_pair(B, name):
    """Every variant the pair plan can choose, on 8 frames of 2100 atoms: frame 0 clean, frames 1-6 one pattern each, each
    at another placement, frame 7 NaN at every placement (every pattern at every placement: tests/test_nonfinite_cpu.py,
    on the oracle). full, part, overflow and CN equal the C oracle on the same input, which _pair_scene has shown to
    equal the oracle on the frame with those atoms deleted and to differ from the clean frame's."""
    from mdproptools_amd._lib import Context

    case, want = PAIR_CASES[name]
    s = _pair_scene(case, name, NEED[case["op"]])
    ctx = Context(0)
    try:
        for k, v in case["opts"].items():
            ctx.set_option(k, v)
        plan = P.plan(case, 0, 0, ctx=ctx)
        for k, v in want.items():
            assert plan[k] == v, (name, k, plan)
        op, pf = case["op"], case["per_frame"]
        x = _cuda(s["xyz"]) if case["dev"] else s["xyz"]
        red = (lambda a: a) if pf else (lambda a: a.sum(axis=0))
        a = (x, s["types"], s["box"], case["rel"])
        hist = (case["r_cut"], case["bin"], case["nbins"])
        if op in ("rdf", "rdf_cn"):
            if op == "rdf":
                full, part, ov = B.rdf_loop(*a, *hist, per_frame=pf, ctx=ctx)
            else:
                full, part, ov, cn = B.rdf_cn_loop(*a, *hist, s["cuts"], per_frame=pf, ctx=ctx)
            kernel = ctx.last_kernel_name()
            np.testing.assert_array_equal(full, red(s["full"]), err_msg=name)
            np.testing.assert_array_equal(part, red(s["part"]), err_msg=name)
            assert ov == s["ov"]
            if op == "rdf_cn":
                np.testing.assert_array_equal(cn, red(s["cn"]), err_msg=name)
        elif op == "cn":
            cn = B.cn_loop(*a, s["cuts"], per_frame=pf, ctx=ctx)
            kernel = ctx.last_kernel_name()
            np.testing.assert_array_equal(cn, red(s["cn"]), err_msg=name)
        else:
            sites = _cuda(s["sites"]) if case["dev"] else s["sites"]
            b = (x, s["types"], sites, case["site_types"], s["box"], case["rel"])
            if op == "rdf_sites":
                part, ov = B.rdf_mol_loop(*b, *hist, per_frame=pf, ctx=ctx)
                kernel = ctx.last_kernel_name()
                np.testing.assert_array_equal(part, red(s["part"]), err_msg=name)
                assert ov == s["ov"]
            else:
                cn = B.cn_mol_loop(*b, s["cuts"], per_frame=pf, ctx=ctx)
                kernel = ctx.last_kernel_name()
                np.testing.assert_array_equal(cn, red(s["cn"]), err_msg=name)
        if plan["status"] == 0:  # (an RDF + CN call in two sweeps leaves the second sweep's name)
            assert kernel == plan["kernel"], (name, kernel, plan)
        print("%s: %s" % (name, kernel))
    finally:
        ctx.close()


@pytest.mark.parametrize("opts,token", [(dict(rdf_cull=0), "pair_hist_fast_kernel"), (dict(rdf_cull=1, rdf_pk=0), "<1,"),
                                        (dict(rdf_cull=1), "<3,")], ids=["dense", "f64", "packed"])
def test_pair_histograms_equal_the_call_without_the_atoms(B, opts, token):
    """The deletion identity on the device itself: the poisoned frames against the same kernel family on the frames with
    the atoms taken out (2099, 2098 or 2094 atoms: one call per frame), host and device input. (The token is the kernel the
    RDF + CN call leaves: with rdf_pk 0 it runs in two sweeps and the CN sweep, MODE 1, is the last.)"""
    from mdproptools_amd._lib import Context

    case, _ = PAIR_CASES["packed"]
    s = _pair_scene(case, "packed", ())
    ctx = Context(0)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        hist = (case["r_cut"], case["bin"], case["nbins"])
        for put in (lambda v: v, _cuda):
            full, part, ov, cn = B.rdf_cn_loop(put(s["xyz"]), s["types"], s["box"], case["rel"], *hist, s["cuts"], ctx=ctx)
            for f in range(1, case["F"]):  # one frame per pattern, and the frame with six NaN atoms
                x, t = NF.delete(s["clean"][f], s["types"], s["plan"][f][1])
                f1, p1, _, c1 = B.rdf_cn_loop(put(x[None]), t, s["box"][f:f + 1], case["rel"], *hist, s["cuts"], ctx=ctx)
                assert token in ctx.last_kernel_name(), ctx.last_kernel_name()
                np.testing.assert_array_equal(full[f], f1[0])
                np.testing.assert_array_equal(part[f], p1[0])
                np.testing.assert_array_equal(cn[f], c1[0])
    finally:
        ctx.close()


# ================================================================================= 2. shell consumers and residence
def _shell_system(seed, n_frames=3, n=4200, L=40.0):
    """n atoms in 3-atom molecules, uniform in the box; 20 centres that include the placements; the poison plan puts one
    pattern per frame on atoms NEXT to a centre (so that the poison takes a member away) and on a centre."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (n_frames, 3, n)) * L
    mol_of = (np.arange(n) // 3).astype(np.int32)
    seg_off = np.arange(0, n + 1, 3).astype(np.int64)
    centres = np.unique(np.concatenate([NF.places(n), rng.choice(n, 14, replace=False)])).astype(np.int32)
    return xyz, np.full((n_frames, 3), L), mol_of, seg_off, centres


def _nearest_other(x, box, p, mol_of):
    r = CR.rsq(x[:, p], x, box)
    r[mol_of == mol_of[p]] = np.inf
    return int(np.argmin(r))


def _far_frame(x, atoms, L):
    """Indices kept: the atoms moved to distinct points outside every cutoff used below (the cell is [0, L), the box
    handed to the library 3 L long, the atoms go to 1.5 L + 8 k)."""
    y = x.copy()
    for k, a in enumerate(atoms):
        y[:, a] = 1.5 * L + 8.0 * k
    return y


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_shell_members_and_coordination_drop_the_poisoned_atom_only(B, ctx, pattern):
    """shell_members (shell_hits_kernel) and shell_coordination (coord_hits_kernel): a poisoned neighbour of a centre in
    frame 1 leaves frame 1's rows as the restatement's on that input and as the rows of the frame with the atom moved out
    of reach; frames 0 and 2 are bit-identical to the clean call; a poisoned centre (frame 2 of the second call) has an
    empty row."""
    xyz, box, mol_of, seg_off, centres = _shell_system(31)
    L = box[0, 0]
    box = box * 3.0  # atoms fill a third of the box per axis: "out of reach" exists
    rs, rc = 4.5 ** 2, 3.2 ** 2
    n = xyz.shape[2]
    mol_type = (1 + np.arange(len(seg_off) - 1) % 3).astype(np.int32)
    cls = (np.arange(n) % 4).astype(np.uint8)
    c0 = int(centres[3])
    near = _nearest_other(xyz[1], box[1], c0, mol_of)
    atoms = (near,) if pattern != "two_plus_inf" else (near, _nearest_other(xyz[1], box[1], int(centres[7]), mol_of))
    for victims, frame in ((atoms, 1), ((c0,), 2)):
        bad, far = xyz.copy(), xyz.copy()
        bad[frame] = NF.poison(xyz[frame], pattern, victims)
        far[frame] = _far_frame(xyz[frame], victims, L)
        mols, count = B.shell_members(bad, box, centres, mol_of, rs)
        assert ctx.last_kernel_name() in ("shell_hits_kernel", "shell_sort_kernel"), ctx.last_kernel_name()
        m_far, c_far = B.shell_members(far, box, centres, mol_of, rs)
        m_clean, c_clean = B.shell_members(xyz, box, centres, mol_of, rs)
        for f in range(3):
            for ci, p in enumerate(centres):
                want = CR.shell(bad[f], box[f], p, mol_of, rs)
                assert count[f, ci] == len(want) and np.array_equal(mols[f, ci, :len(want)], want), (f, p)
                if f == frame and p in victims:
                    assert list(want) == ([mol_of[p]] if pattern == "huge_finite" else [])
                elif not (f == frame and p in victims):
                    k = c_far[f, ci]
                    assert count[f, ci] == k and np.array_equal(mols[f, ci, :k], m_far[f, ci, :k]), (f, p)
            if f != frame:
                assert np.array_equal(count[f], c_clean[f]) and np.array_equal(mols[f], m_clean[f][:, :mols.shape[2]])
        if frame == 1:
            assert not np.array_equal(count[1], c_clean[1])  # the poison took a member away
        ok = [int(p) for p in centres if p not in victims]
        rows = CFG.coordination_rows(bad, box, ok, mol_of, seg_off, mol_type, cls, rs, rc)
        rows_far = CFG.coordination_rows(far, box, ok, mol_of, seg_off, mol_type, cls, rs, rc)
        assert rows == rows_far
        gm, gw, gc = B.shell_coordination(bad, box, np.array(ok, np.int32), mol_of, seg_off, mol_type, cls, rs, rc)
        assert "coord" in ctx.last_kernel_name(), ctx.last_kernel_name()
        for f in range(3):
            for ci in range(len(ok)):
                k = gc[f, ci]
                got = [(int(m), int(w)) for m, w in zip(gm[f, ci, :k], gw[f, ci, :k])]
                assert got == rows[f][ci], (f, ok[ci])


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
def test_contact_components_link_nothing_through_a_poisoned_atom(B, ctx, pattern):
    """contact_components (agg_union_kernel): labels, component and contact counts of the poisoned frame equal the
    restatement's on that input and on the frame with the atoms out of reach; the other frame is the clean call's."""
    n, L = 600, 15.0
    xyz = NF.uniform_frames(41, 2, n, L)
    box = np.full((2, 3), 3.0 * L)
    aa, ca, ab, cb, node_of, n_nodes = AR.all_atoms(n)
    cut = np.array([[1.0 ** 2]])  # (0.8 neighbours per atom: many small components)
    clean = B.contact_components(xyz, box, aa, ca, ab, cb, cut, node_of, n_nodes)
    assert ctx.last_kernel_name() == "agg_union_kernel"
    linked = np.flatnonzero(np.bincount(clean[0][1], minlength=n) > 1)  # roots of components with several members
    assert len(linked) >= 6
    for i in range(4):
        # the poisoned atom is a member of a component of several atoms: the root itself, and a non-root member
        root = int(linked[i % len(linked)])
        member = int(np.flatnonzero(clean[0][1] == root)[-1])
        atoms = (root, member) if pattern == "two_plus_inf" else ((root,) if i % 2 else (member,))
        bad, far = xyz.copy(), xyz.copy()
        bad[1] = NF.poison(xyz[1], pattern, atoms)
        far[1] = _far_frame(xyz[1], atoms, L)
        lab, ncomp, ncon = B.contact_components(_cuda(bad) if i % 2 else bad, box, aa, ca, ab, cb, cut, node_of, n_nodes)
        want = AR.contact_components(bad, box, aa, ca, ab, cb, cut, node_of, n_nodes)
        want_far = AR.contact_components(far, box, aa, ca, ab, cb, cut, node_of, n_nodes)
        for got, w, wf, c in zip((lab, ncomp, ncon), want, want_far, clean):
            np.testing.assert_array_equal(got.astype(np.int64), w)
            np.testing.assert_array_equal(w, wf)
            np.testing.assert_array_equal(got[0], c[0])
        for a in atoms:
            assert lab[1, a] == a and (lab[1] == a).sum() == 1
        assert ncon[1] < clean[2][1]


@pytest.mark.parametrize("pattern", NF.PATTERN_NAMES)
@pytest.mark.parametrize("side", ["central", "shell"])
def test_shell_residence_clears_the_poisoned_frame_of_the_pair_only(B, ctx, pattern, side):
    """shell_residence (shell_pairs_kernel) on a designed trajectory (tests/residence_design.py): one atom of group 0
    poisoned in frame t* takes frame t* out of the presence pattern of its pairs and nothing else — the closed form."""
    F = 70  # (more than one 64-frame word of the presence masks)
    pats = RD.patterns(F, seed=3)
    groups = [(pats["always"], 2, 3), (pats["periodic"], 3, 2), (pats["random"], 1, 4)]
    d = RD.designed(groups, seed=6)
    counts, nrec = B.shell_residence(d.xi, d.xj, d.box, RD.LO ** 2, RD.HI ** 2)
    assert ctx.last_kernel_name() == "shell_pairs_kernel"
    np.testing.assert_array_equal(counts.astype(np.int64), d.counts)
    for t_star in (0, 63, 64, F - 1):
        xi, xj = d.xi.copy(), d.xj.copy()
        a, b = groups[0][1], groups[0][2]
        k = 2 if pattern == "two_plus_inf" else 1
        if side == "central":
            xi[t_star] = NF.poison(xi[t_star], pattern, (0, 1)[:k])
            lost = k * b
        else:
            xj[t_star] = NF.poison(xj[t_star], pattern, (0, 1)[:k])
            lost = k * a
        p0 = groups[0][0].copy()
        p0[t_star] = False
        want = d.counts - lost * RD.acorr(groups[0][0]) + lost * RD.acorr(p0)
        counts, nrec = B.shell_residence(xi, xj, d.box, RD.LO ** 2, RD.HI ** 2)
        np.testing.assert_array_equal(counts.astype(np.int64), want, err_msg="t*=%d" % t_star)
        assert nrec == d.n_records - lost


@pytest.mark.parametrize("pattern", ["plus_inf", "minus_inf", "two_plus_inf", "huge_finite", "nan_all_axes"])
def test_angles_and_hydration_with_infinite_and_huge_coordinates(B, ctx, pattern):
    """angle_hist (ang_search_kernel) and hydration_counts (hy_search_kernel): a neighbour or a water oxygen at +-Inf or
    1e300 is in no shell — integers of the restatement on the same input, and of the frame with it out of reach."""
    n, L = 900, 14.0
    xyz = np.round(NF.uniform_frames(51, 2, n, L), 3)
    box = np.full((2, 3), 3.0 * L)
    types = np.arange(n) % 3 + 1
    trip, rc2 = [(2, 1, 2), (2, 1, 3)], np.array([[3.5, 3.5], [3.5, 3.0]]) ** 2
    edges = B.angle_cos_edges(1.0)
    clean = B.angle_hist(xyz, box, types, trip, rc2, edges)
    assert ctx.last_kernel_name() == "ang_search_kernel"
    busiest = int(np.argmax(clean[2][1]))
    centre = int(clean[3][busiest])
    r = CR.rsq(xyz[1][:, centre], xyz[1], box[1])
    r[types == 1] = np.inf
    victims = tuple(int(v) for v in np.argsort(r)[:2 if pattern == "two_plus_inf" else 1])
    bad, far = xyz.copy(), xyz.copy()
    bad[1] = NF.poison(xyz[1], pattern, victims)
    far[1] = _far_frame(xyz[1], victims, L)
    got = B.angle_hist(bad, box, types, trip, rc2, edges)
    want = ANG.angle_hist(bad, box, types, trip, rc2, edges)
    want_far = ANG.angle_hist(far, box, types, trip, rc2, edges)
    for g, w, wf in zip(got[:3], want[:3], want_far[:3]):
        np.testing.assert_array_equal(g.astype(np.int64), w)
        np.testing.assert_array_equal(w, wf)
    assert got[2][1, busiest] == clean[2][1, busiest] - len(victims)
    np.testing.assert_array_equal(got[2][0], clean[2][0])
    # hydration: ions 0..29, then waters of three atoms (O, H1, H2)
    n_ion, n_wat = 30, 290
    ions, wat = np.arange(n_ion), n_ion + 3 * np.arange(n_wat)
    hw = B.hydration_counts(xyz, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    assert ctx.last_kernel_name().startswith("hy_search_kernel")
    ion = int(np.argmax(hw[0][1]))
    r = CR.rsq(xyz[1][:, ion], xyz[1][:, wat], box[1])
    o_victims = tuple(int(wat[v]) for v in np.argsort(r)[:2 if pattern == "two_plus_inf" else 1])
    bad, far = xyz.copy(), xyz.copy()
    bad[1] = NF.poison(xyz[1], pattern, o_victims)
    far[1] = _far_frame(xyz[1], o_victims, L)
    # (the hydrogens go with their oxygen, so that the far frame's cosines are those of the same water elsewhere)
    for k, o in enumerate(o_victims):
        far[1][:, o + 1:o + 3] += (far[1][:, o] - xyz[1][:, o])[:, None]
    g_bad = B.hydration_counts(bad, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    g_far = B.hydration_counts(far, box, ions, wat, 3.5 ** 2, -0.72, 0.02, 100)
    for u, v in zip(g_bad, g_far):
        np.testing.assert_array_equal(u, v)
    assert g_bad[0][1, ion] == hw[0][1, ion] - len(o_victims)
    np.testing.assert_array_equal(g_bad[0][0], hw[0][0])


# ========================================================================================== 3. segment COM, charge flux
SEG_CONFIGS = [(1, 0, 1, 0), (1, 512, 1, 0), (1, 1024, 0, 3), (1, 256, 1, 3), (0, 0, 1, 0), (0, 512, 0, 0), (0, 1024, 1, 3),
               (0, 256, 0, 1)]
SEG_DEFAULTS = dict(seg_frame=1, seg_cap=0, seg_vec=1, seg_gy=0)
SEG_POISON = (float("nan"), float("inf"), -float("inf"), 1e300)


@pytest.mark.parametrize("table", ["water", "four", "ragged", "types"])
def test_segment_com_and_flux_poison_one_segment_of_one_frame(B, ctx, table):
    """The variants of test_gpu_segment_exact.py (seg_frame, seg_cap, seg_vec, seg_gy; 1, 3 and 4 planes): one poisoned
    atom makes exactly its segment's COM of its plane, or its type's flux component, non-finite in its frame — the
    restatement's mask and values — and everything else is bit-identical to the clean call. The atom is the first, a
    middle and the last one of the table, in the first, a middle and the last frame."""
    tables = dict(SX.segment_tables())
    t_sizes, t_st, t_T = SX.type_table()
    tables["types"] = t_sizes
    sizes = tables[table]
    off = SX.offsets(sizes)
    N, M, F = int(off[-1]), len(sizes), SX.FRAMES
    m, q = SX.case_masses(table, off)
    st, T = (t_st, t_T) if table == "types" else SX.seg_types(M)
    vel = SX.case_vel(table, off, F)
    seen = set()
    try:
        for ci, cfg in enumerate(SEG_CONFIGS):
            for key, val in zip(("seg_frame", "seg_cap", "seg_vec", "seg_gy"), cfg):
                ctx.set_option(key, val)
            K = (1, 3, 4)[ci % 3]
            attr = SX.case_attr(table, off, F, K)
            clean = B.segment_com(attr, m, off, ctx=ctx)[0]
            clean_flux = B.charge_flux(vel, m, q, off, st, T, SX.VEL_CONV, SX.CHARGE_CONV, ctx=ctx)
            for pi, (atom, f) in enumerate(((0, 0), (N // 2, F // 2), (N - 1, F - 1))):
                v = SEG_POISON[(ci + pi) % 4]
                k = (ci + pi) % K
                seg = int(np.searchsorted(off, atom, side="right") - 1)
                bad = attr.copy()
                bad[f, k, atom] = v
                got = B.segment_com(_cuda(bad) if pi == 1 else bad, m, off, ctx=ctx)[0]
                seen.add(ctx.last_kernel_name())
                want = SX.com(bad, m, off)
                what = "%s %s atom %d frame %d plane %d value %r: %s" % (table, cfg, atom, f, k, v, ctx.last_kernel_name())
                assert NF.same_bits(got, want), what
                touched = np.zeros(got.shape, bool)
                touched[f, k, seg] = True
                assert not np.isfinite(got[f, k, seg]) or v == 1e300, what
                _untouched_equal(got, clean, touched, what)
                badv = vel.copy()
                badv[f, k % 3, atom] = v
                gf = B.charge_flux(badv, m, q, off, st, T, SX.VEL_CONV, SX.CHARGE_CONV, ctx=ctx)
                seen.add(ctx.last_kernel_name())
                wf = SX.flux(badv, m, q, off, st, T)
                assert NF.same_bits(gf, wf), "flux " + what
                touched = np.zeros(gf.shape, bool)
                touched[k % 3, st[seg], f] = True
                _untouched_equal(gf, clean_flux, touched, "flux " + what)
    finally:
        for key, val in SEG_DEFAULTS.items():
            ctx.set_option(key, val)
    print(table, sorted(seen))
    assert any(k.startswith("segment_frame_kernel") for k in seen) and any(k.startswith("segment_staged_kernel") for k in seen)


# ================================================================================================================ 4. MSD
MSD_GROUPS = {37: [0, 20, 20, 37], 1026: [0, 500, 1026]}


def _msd_ref(r, pairs, go, scale, origin=None):
    """numpy float64 of msd_pairs with every group summed on its own: sums [P, G, 4], per-entity rows [P, E, 4]."""
    r0 = origin[None] if origin is not None else r[pairs[:, 0]]
    d = r[pairs[:, 1]] * scale - r0 * scale
    d2 = d * d
    allc = np.concatenate([d2, ((d2[:, 0] + d2[:, 1]) + d2[:, 2])[:, None]], axis=1)  # [P, 4, E]
    return NF.group_sums_direct(allc, go).transpose(0, 2, 1), allc.transpose(0, 2, 1)


@pytest.mark.parametrize("E", [37, 1026])
@pytest.mark.parametrize("value", SEG_POISON)
def test_msd_pairs_origin_and_windows_poison_one_group_and_axis(B, ctx, E, value):
    """msd_pairs (sums, per-entity rows, columns, device result), msd_origin and msd_windows on exact data (k / 1024):
    one sample of one entity and axis, at frame t*, makes non-finite that entity's row, its group's sum on that axis and
    the total, at the pairs (frames, windows) that touch t*, exactly as numpy does; the rest equals the clean call bit
    for bit. E = 37: the scalar path, ragged groups with an empty one; E = 1026: the 16-byte path over two chunks."""
    import torch

    rng = np.random.default_rng(E)
    F, t_star = 40, 17
    r = NF.k1024(rng, (F, 3, E))
    go = np.array(MSD_GROUPS[E], dtype=np.int64)
    ent, ax = (go[2] + 3) if E == 37 else 1025, 1
    g = int(np.searchsorted(go, ent, side="right") - 1)
    bad = r.copy()
    bad[t_star, ax, ent] = value
    pairs = np.concatenate([np.column_stack([np.zeros(F, np.int32), np.arange(F, dtype=np.int32)]),
                            rng.integers(0, F, (60, 2)).astype(np.int32), [[t_star, t_star], [t_star, 0]]]).astype(np.int32)
    P_ = len(pairs)
    hits = (pairs == t_star).any(axis=1)
    want, want_pe = _msd_ref(bad, pairs, go, 0.5)
    clean, clean_pe = B.msd_pairs(r, pairs, go, scale=0.5, per_entity=True, ctx=ctx)
    sums, pe = B.msd_pairs(bad, pairs, go, scale=0.5, per_entity=True, ctx=ctx)
    assert ctx.last_kernel_name() == "msd_pairs_kernel"
    assert NF.same_bits(sums, want) and NF.same_bits(pe, want_pe)
    touched = np.zeros(sums.shape, bool)
    touched[np.ix_(hits, [g], [ax, 3])] = True
    _mask_within(sums, touched)  # (NaN - NaN at the pair (t*, t*) too, as numpy; the finite 2^996 gives 0 there)
    _untouched_equal(sums, clean, touched, "sums")
    t_pe = np.zeros(pe.shape, bool)
    t_pe[np.ix_(hits, [ent], [ax, 3])] = True
    _mask_within(pe, t_pe)
    _untouched_equal(pe, clean_pe, t_pe, "per-entity rows")
    block = np.full((4, P_ * E + 6), -7.0)
    s2 = B.msd_pairs_cols(bad, pairs, go, block[:, 3:3 + P_ * E], scale=0.5, ctx=ctx)
    assert NF.same_bits(s2, want) and NF.same_bits(block[:, 3:3 + P_ * E], want_pe.reshape(P_ * E, 4).T)
    assert (block[:, :3] == -7.0).all() and (block[:, 3 + P_ * E:] == -7.0).all()
    dev = torch.full((P_, len(go) - 1, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    B.msd_pairs(_cuda(bad), pairs, go, scale=0.5, out=dev, ctx=ctx)
    assert NF.same_bits(dev.cpu().numpy(), want)
    # msd_origin: every frame against a separate origin; then the origin itself poisoned (every frame is touched)
    origin = NF.k1024(rng, (3, E))
    op = np.column_stack([np.full(F, -1, np.int32), np.arange(F, dtype=np.int32)])
    w_o, w_ope = _msd_ref(bad, op, go, 1.0, origin=origin)
    cols = np.full((4, F * E), -3.0)
    got_o = B.msd_origin(bad, origin, go, cols=cols, ctx=ctx)
    assert NF.same_bits(got_o, w_o) and NF.same_bits(cols, w_ope.reshape(F * E, 4).T)
    t_o = np.zeros(got_o.shape, bool)
    t_o[t_star, g, [ax, 3]] = True
    _mask_within(got_o, t_o)
    _untouched_equal(got_o, B.msd_origin(r, origin, go, ctx=ctx), t_o, "msd_origin")
    bad_origin = origin.copy()
    bad_origin[ax, ent] = value
    got_oo = B.msd_origin(_cuda(r), _cuda(bad_origin), go, ctx=ctx)
    assert NF.same_bits(got_oo, _msd_ref(r, op, go, 1.0, origin=bad_origin)[0])
    t_oo = np.zeros(got_oo.shape, bool)
    t_oo[:, g, [ax, 3]] = True
    _mask_within(got_oo, t_oo)
    # msd_windows: the kept frames t* touches (tao 1: two windows; tao 17: t* is a kept frame; tao 3: it is not kept)
    for tao in (1, 17, 3):
        kept = bad[::tao]
        d2 = (kept[1:] - kept[:-1]) ** 2
        want_w = np.concatenate([d2.sum(axis=0).T, ((d2[:, 0] + d2[:, 1]) + d2[:, 2]).sum(axis=0)[:, None]], axis=1)
        got_w = B.msd_windows(bad, tao, ctx=ctx)
        assert ctx.last_kernel_name() == "msd_windows_kernel"
        assert NF.same_bits(got_w, want_w), tao
        t_w = np.zeros(got_w.shape, bool)
        if t_star % tao == 0:
            t_w[ent, [ax, 3]] = True
        _mask_within(got_w, t_w, tao)
        _untouched_equal(got_w, B.msd_windows(r, tao, ctx=ctx), t_w, "msd_windows")


W1, LDS, W12, W12P, W12R = ("msd_power_w1_kernel", "msd_power_lds_kernel", "msd_power_w12_kernel", "msd_power_w12p_kernel",
                            "msd_power_w12r_kernel")
W12PO, BATCHED = "msd_power_w12p_kernel + msd_power_w12o_kernel", "lag_msd_fft"
LAG_RESTORE = {"lag_fft_kernel": 3}
# (F, max_lag, generator, the spectral kernel, its padded length, the options that force it): one shape per path, from the
# tables of test_gpu_lag_exact.py
LAG_PATHS = [
    (513, 512, "white", W1, 2048, {}),
    (1500, 548, "spikes", LDS, 2048, {"lag_w1": 0, "lag_w12_min_f": 0}),
    (1536, 1535, "walk", W12, 12288, {}),
    (8193, 8192, "white", W12P, 24576, {"lag_residue": 1}),
    (8193, 8192, "white", W12R, 24576, {"lag_residue": 2}),
    (12289, 4096, "p3", W12PO, 49152, {}),
    (24577, 1000, "white", BATCHED, 32768, {}),
]
_LAG_CASES = {}


def _lag_case(F, max_lag, gen):
    """Trajectory (3 entities in groups [0, 1, 3]), exact sums and energies; computed once per shape."""
    key = (F, max_lag, gen)
    if key not in _LAG_CASES:
        goff = [0, 1, 3]
        xi = LX.GENERATORS[gen](np.random.default_rng(F * 31 + max_lag), F, 3)
        S = LX.exact_sums(xi, max_lag, goff)
        assert LX.sums_fit_double(S)
        _LAG_CASES[key] = dict(r=LX.to_float(xi), S=S, Q=LX.energy(xi, goff), goff=goff,
                               means=LX.exact_means(S, F, goff, 1.0)[0])
    return _LAG_CASES[key]


def _lag_poison(c, F, value, t_star):
    """Entity 2 (group 1), axis y, frame t*: the poisoned trajectory, and the difference form's expected result — the exact
    means with (group 1, y) and (group 1, total) non-finite at the lags k <= max(t*, F - 1 - t*), NaN or +Inf as the plain
    sum of (x[t + k] - x[t])^2 gives (lag 0 holds value - value)."""
    bad = c["r"].copy()
    bad[t_star, 1, 2] = value
    K = c["means"].shape[0]
    want = c["means"].copy()
    col = bad[:, 1, 2]
    for k in range(min(K, max(t_star, F - 1 - t_star) + 1)):
        d = col[k:] - col[:F - k]
        s = np.sum(d * d)  # non-finite: its kind (NaN / Inf) is what a sum in any order gives
        if k == 0 and np.isfinite(value):
            continue  # (1e300 - 1e300 = 0: lag 0 stays 0)
        assert not np.isfinite(s)
        want[k, 1, 1] = s
        want[k, 1, 3] = s
    return bad, want


@pytest.mark.parametrize("F,max_lag,gen,kernel,L,opts", LAG_PATHS, ids=[p[3].replace("msd_power_", "") + "-%d" % i
                                                                        for i, p in enumerate(LAG_PATHS)])
def test_lag_msd_poisoned_sample_on_every_path(B, ctx, F, max_lag, gen, kernel, L, opts):
    """One sample of one entity and axis poisoned at frame t*.
    Difference kernels (lag_variant 1, and 0 for the short shapes): non-finite at exactly the lags k <= max(t*, F - 1 - t*)
    of that (group, axis) and of its total; every other lag and column bit-exact (the correctly rounded exact means).
    The forced spectral path (lag_variant 2 + the path's options): every OTHER (group, axis) column
    meets the per-lag criterion of test_gpu_lag_exact.py against the exact sums; the reported bound is not a finite
    number <= 1e-10; the affected column may be NaN throughout.
    lag_variant 3 (the default): the whole result equals the difference kernel's — the call falls back, as for a missed
    bound."""
    c = _lag_case(F, max_lag, gen)
    goff = c["goff"]
    for value, t_star in ((float("nan"), F // 3), (float("inf"), F - 1), (1e300, 0)):
        bad, want = _lag_poison(c, F, value, t_star)
        with options(ctx, lag_variant=1):
            diff = B.lag_msd(bad, max_lag, goff, ctx=ctx)
            assert ctx.last_kernel_name() in ("lag_msd_lds_kernel", "lag_msd_kernel") and ctx.last_rel_bound() == 0.0
        assert NF.same_bits(diff, want), (value, t_star, np.argwhere(~((diff == want) | (np.isnan(diff) & np.isnan(want))))[:5])
        if F <= 2000:
            with options(ctx, lag_variant=0):
                d0 = B.lag_msd(bad, max_lag, goff, ctx=ctx)
                assert ctx.last_kernel_name() == "lag_msd_kernel"
            assert NF.same_bits(d0, want), (value, t_star)
        forced = {"lag_variant": 2, **opts}
        with options(ctx, restore={k: LAG_RESTORE.get(k, -1) for k in forced}, **forced):
            got = B.lag_msd(bad, max_lag, goff, ctx=ctx)
            name, bound = ctx.last_kernel_name(), ctx.last_rel_bound()
        assert name == kernel, (name, kernel)
        assert not (np.isfinite(bound) and bound <= 1e-10), bound
        others = got.copy()
        others[:, 1, 1] = c["means"][:, 1, 1]  # (the affected column and its total are not judged)
        others[:, 1, 3] = c["means"][:, 1, 3]
        assert np.isfinite(others).all(), (value, t_star, np.argwhere(~np.isfinite(others))[:5])
        j = LX.judge(others, c["S"], c["Q"], F, goff, L, 1.0)
        assert j["frac"] <= 1.0, (kernel, value, j)
        with options(ctx, restore={k: LAG_RESTORE.get(k, -1) for k in opts}, **opts):
            ctx.set_option("lag_variant", 3)
            try:
                dflt = B.lag_msd(bad, max_lag, goff, ctx=ctx)
                name3, bound3 = ctx.last_kernel_name(), ctx.last_rel_bound()
            finally:
                ctx.set_option("lag_variant", -1)
        assert name3 in ("lag_msd_lds_kernel", "lag_msd_kernel") and bound3 == 0.0, (name3, bound3)
        assert NF.same_bits(dflt, diff), (kernel, value)
        print("%s value %r t* %d: forced bound %r, default fell back to %s" % (kernel, value, t_star, bound, name3))


# ============================================================================================================= 5. series
HUGE = 2.0 ** 996  # ~ 6.7e299, a power of two: its products with the integer samples are exact, fused or not, so that
# "the finite lags are equal" does not depend on how a kernel rounds 1e300 * x + acc


def _plain_xcorr(a, b, lag0, n_lags):
    """c[k] = sum_t a[t + k] b[t] / (n - k), summed by numpy one lag at a time."""
    n = len(a)
    return np.array([np.sum(a[k:] * b[:n - k]) / (n - k) for k in range(lag0, lag0 + n_lags)])


@pytest.mark.parametrize("n", [257, 3000])
def test_xcorr_poisoned_series_stays_in_its_row(B, ctx, n):
    """xcorr, direct and FFT, a batch of 3 integer series with one sample of the middle one poisoned (auto and cross,
    all lags and n_lags < n): the other two rows are bit-identical to the clean batch; the poisoned row of the direct
    method has the non-finite mask of the plain sums and equal finite lags; of the FFT method, numpy's rfft / irfft mask
    (which kind of non-finite a butterfly leaves depends on the factorisation, that it is non-finite does not)."""
    rng = np.random.default_rng(n)
    a = rng.integers(-50, 51, (3, n)).astype(np.float64)
    b = rng.integers(-50, 51, (3, n)).astype(np.float64)
    nl = n // 3
    for value, t in ((float("nan"), n // 2), (float("inf"), 0), (-float("inf"), n - 1), (HUGE, 5)):
        bad = a.copy()
        bad[1, t] = value
        for method, kname in ((B.XCORR_DIRECT, "xcorr_direct_kernel"), (B.XCORR_FFT, "fft_pass_kernel<0, 0>")):
            for y, cy, lags in ((None, None, n), (b, b, n), (b, b, nl)):
                kw = {} if lags == n else {"n_lags": lags}
                clean = B.xcorr(a, cy, method=method, ctx=ctx, **kw)
                got = B.xcorr(bad, y, method=method, ctx=ctx, **kw)
                assert ctx.last_kernel_name() == kname
                what = (n, value, t, kname, y is None, lags)
                assert np.array_equal(got[[0, 2]], clean[[0, 2]]), what
                other = bad[1] if y is None else b[1]
                if method == B.XCORR_DIRECT:
                    want = _plain_xcorr(bad[1], other, 0, lags)
                    assert (np.isfinite(got[1]) == np.isfinite(want)).all(), what
                    fin = np.isfinite(want)
                    assert (np.isnan(got[1]) == np.isnan(want)).all(), what
                    assert np.array_equal(got[1][fin], want[fin]), what
                    assert not fin.all() or (value == HUGE and y is not None)  # (2^996 times an integer is finite)
                else:
                    Lp = 1 << (2 * n - 1).bit_length()
                    ref = np.fft.irfft(np.fft.rfft(bad[1], Lp) * np.conj(np.fft.rfft(other, Lp)), Lp)[:lags]
                    assert (np.isfinite(got[1]) == np.isfinite(ref)).all(), what
                    assert not np.isfinite(ref).any() or value == HUGE
    dev = _cuda(bad)
    np.testing.assert_array_equal(np.isfinite(B.xcorr(dev, method=B.XCORR_DIRECT, ctx=ctx)),
                                  np.isfinite(B.xcorr(bad, method=B.XCORR_DIRECT, ctx=ctx)))


def _cumsum_ref(y, dx):
    return np.cumsum(dx * (y[:, 1:] + y[:, :-1]) / 2.0, axis=1)


def _check_scan(B, ctx, y, dx, what, exact=True):
    """cumtrapz of y [S, n], both leading_zero forms, host and device input: the non-finite mask is numpy's cumsum of the
    increments and the finite entries are equal (bit-equal: the data is integer-valued)."""
    import torch

    want = _cumsum_ref(y, dx)
    for lead in (False, True):
        for put in (lambda v: v, _cuda):
            got = B.cumtrapz(put(y), dx, leading_zero=lead, ctx=ctx)
            assert ctx.last_kernel_name() == "trap_scan_onepass_kernel"
            if lead:
                assert not got[:, 0].any()
                got = got[:, 1:]
            assert (np.isnan(got) == np.isnan(want)).all(), (what, lead, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
            assert NF.same_bits(got, want), (what, lead)
    out = torch.full(want.shape, -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    B.cumtrapz(y, dx, out=out, ctx=ctx)
    assert NF.same_bits(out.cpu().numpy(), want), what
    return want


def test_cumtrapz_keeps_the_integrals_before_a_bad_sample(B, ctx):
    """The bad sample at every position mod 8 (a lane's run of 8 increments), at 2047 / 2048 / 2049 (a tile's edge), at
    the first and the last sample; NaN, +Inf, -Inf, +Inf followed by -Inf, and finite samples whose running sum overflows.
    Three series per call: the one before and the one after the poisoned series are untouched."""
    rng = np.random.default_rng(8)
    n = 5000
    y = rng.integers(-1000, 1001, (3, n)).astype(np.float64)
    clean = _cumsum_ref(y, 2.0)
    for value in (float("nan"), float("inf"), -float("inf")):
        for t in list(range(1016, 1024)) + [0, 1, 2047, 2048, 2049, n - 2, n - 1]:
            bad = y.copy()
            bad[1, t] = value
            want = _check_scan(B, ctx, bad, 2.0, (value, t))
            first = max(t - 1, 0)
            assert np.array_equal(want[1, :first], clean[1, :first]) and not np.isfinite(want[1, first:]).any()
            assert np.array_equal(want[[0, 2]], clean[[0, 2]])
    bad = y.copy()
    bad[1, 1019], bad[1, 3000] = float("inf"), -float("inf")  # +Inf from 1018 on, NaN from 2999 on
    want = _check_scan(B, ctx, bad, 2.0, "inf then -inf")
    assert np.isposinf(want[1, 1018:2999]).all() and np.isnan(want[1, 2999:]).all()
    # finite samples, exact increments of 2^1019: the running sum passes 2^1024 after 32 of them, inside a lane's run
    big = np.zeros((3, n))
    big[1, 1000:] = 2.0 ** 1018
    big[0], big[2] = y[0], y[2]
    want = _check_scan(B, ctx, big, 2.0, "overflow")
    assert np.isposinf(want[1]).any() and np.isfinite(want[1, :1030]).all() and not np.isnan(want).any()


def test_cumtrapz_poison_across_launch_boundaries(B, ctx):
    """Three series of 2049 tiles each (a launch takes 2048): the poisoned first series continues through the carry words
    into the second launch, the series after it start from nothing."""
    rng = np.random.default_rng(9)
    s, n = 3, 4_196_000
    y = rng.integers(-1000, 1001, (s, n)).astype(np.float64)
    clean = _cumsum_ref(y, 2.0)
    for value, t in ((float("nan"), 2048 * 2048 - 5), (float("inf"), 123_456)):
        bad = y.copy()
        bad[0, t] = value
        want = _cumsum_ref(bad, 2.0)
        for lead in (False, True):
            got = B.cumtrapz(bad, 2.0, leading_zero=lead, ctx=ctx)[:, 1 if lead else 0:]
            assert NF.same_bits(got, want), (value, t, lead)
        assert np.array_equal(want[0, :t - 1], clean[0, :t - 1]) and not np.isfinite(want[0, t - 1:]).any()
        assert np.array_equal(want[1:], clean[1:])


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_green_kubo_equals_the_chain_of_calls_on_poisoned_series(B, ctx, method):
    """green_kubo = xcorr, then cumtrapz of the scaled correlation, then the mean over the series: masks included."""
    m = B.XCORR_DIRECT if method == "direct" else B.XCORR_FFT
    rng = np.random.default_rng(10)
    n = 600
    a = rng.integers(-50, 51, (3, n)).astype(np.float64)
    for value, t in ((float("nan"), 300), (float("inf"), 0), (HUGE, n - 1)):
        bad = a.copy()
        bad[1, t] = value
        acf, integ, mean = B.green_kubo(bad, method=m, acf_scale=0.5, dx=2.0, integral_scale=4.0, want_mean=True, ctx=ctx)
        acf_c = B.xcorr(bad, method=m, ctx=ctx) * 0.5
        int_c = B.cumtrapz(acf_c, 2.0, ctx=ctx) * 4.0
        assert NF.same_bits(acf, acf_c), (method, value)
        assert (np.isfinite(integ) == np.isfinite(int_c)).all() and (np.isnan(integ) == np.isnan(int_c)).all(), (method, value)
        assert np.array_equal(integ[[0, 2]], int_c[[0, 2]])
        fin = np.isfinite(int_c[1])
        np.testing.assert_allclose(integ[1][fin], int_c[1][fin], rtol=1e-13, atol=1e-13 * np.abs(acf_c[1][np.isfinite(acf_c[1])]).max(initial=1.0))
        assert (np.isfinite(mean) == np.isfinite(int_c.mean(axis=0))).all()
        clean = B.green_kubo(a, method=m, acf_scale=0.5, dx=2.0, integral_scale=4.0, ctx=ctx)
        assert np.array_equal(acf[[0, 2]], clean[0][[0, 2]]) and np.array_equal(integ[[0, 2]], clean[1][[0, 2]])
