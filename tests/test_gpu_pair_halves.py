"""The packed sweep's results bit for bit against the C oracle around a change of its pair blocks' instruction order
(slot 1's cutoff compare as a plain v_cmp ahead of slot 0 — the path of every case here whose slots
carry no RET —, both halves' distance chains ahead of the two blocks, the skipped slot joining behind its s_andn2).
The change leaves every integer as it was, so these tests check exactly that and nothing else: they pass on the
sources before it too. Smallest sizes the culled path takes (>= 8 tiles; `rdf_cull` forced): 2048 + 37 atoms — a ragged
last tile and wave — and 2304, in cubic boxes with r_cut / L = 0.4 and 0.49 and in a slab box (an ordinary culled-path
case with whole tiles at one end of a wave's reach; the sweep has no instances for half a group). Atom-atom RDF,
RDF + CN from one sweep, class rows (nine types, the C1 relations) and atoms x sites, each frame-summed and per frame."""
import functools

import numpy as np
import pytest

from oracle import cref as C

pytestmark = pytest.mark.gpu

R_CUT, DDR, NBINS, FRAMES = 10.0, 0.05, 200, 2
BOXES = {"0.40": (25.0, 25.0, 25.0), "0.49": (R_CUT / 0.49,) * 3, "slab": (25.0, 25.0, 62.5)}
SIZES = (2048 + 37, 2304)
CASES = [(b, n) for b in BOXES for n in SIZES]
REL = np.array([[1, 1], [1, 2], [2, 3], [3, 3]])
REL9 = np.array([[9, 1], [9, 4], [9, 6], [9, 9], [1, 3]])  # synth.C1_RELATIONS
CUTS = [3.0, 9.975, 6.2, 9.99]
PACKED = ("<3,", "<4,", "<5,", "<6,")


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ctxs():
    from mdproptools_amd._lib import Context

    plain, rows = Context(0), Context(0)
    for ctx in (plain, rows):
        ctx.set_option("rdf_cull", 1)
    rows.set_option("rdf_rows", 0)  # class rows and their row table (`<5` / `<6`), where the plan would take ordered rows
    yield plain, rows
    plain.close()
    rows.close()


@functools.lru_cache(maxsize=None)
def frames(box, n):
    """(atoms [F, 3, n], sites [F, 3, n], box [F, 3]) of one case; the arrays are shared: nobody writes to them."""
    rng = np.random.default_rng([4200, sorted(BOXES).index(box), n])
    L = np.asarray(BOXES[box])
    xyz = rng.uniform(0, 1, (FRAMES, 3, n)) * L[None, :, None]
    sites = rng.uniform(0, 1, (FRAMES, 3, n)) * L[None, :, None]
    sites[:, :, :30] = xyz[:, :, :30]  # coincident atoms and sites: distance zero
    return xyz, sites, np.tile(L, (FRAMES, 1))


def types_of(n, n_types):
    return np.random.default_rng([4201, n, n_types]).integers(1, n_types + 1, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_rdf(box, n, nine):
    xyz, _, bx = frames(box, n)
    ty, rel = (types_of(n, 9), REL9) if nine else (types_of(n, 3), REL)
    out = [C.rdf_pairs(xyz[f], ty, rel, bx[f], R_CUT * R_CUT, DDR, NBINS) for f in range(FRAMES)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), sum(o[2] for o in out)


@functools.lru_cache(maxsize=None)
def oracle_cn(box, n):
    xyz, _, bx = frames(box, n)
    return np.stack([C.cn_pairs(xyz[f], types_of(n, 3), REL, bx[f], [c * c for c in CUTS]) for f in range(FRAMES)])


def packed(ctx, want=PACKED):
    name = ctx.last_kernel_name()
    assert any(t in name for t in want), name
    return name


@pytest.mark.parametrize("box,n", CASES)
def test_atom_atom_rdf(B, ctxs, box, n):
    xyz, _, bx = frames(box, n)
    full, part, ov = oracle_rdf(box, n, False)
    a = B.rdf_loop(xyz, types_of(n, 3), bx, REL, R_CUT, DDR, NBINS, ctx=ctxs[0])
    packed(ctxs[0])
    np.testing.assert_array_equal(a[0], full)
    np.testing.assert_array_equal(a[1], part)
    assert a[2] == ov
    s = B.rdf_loop(xyz, types_of(n, 3), bx, REL, R_CUT, DDR, NBINS, per_frame=False, ctx=ctxs[0])
    packed(ctxs[0])
    np.testing.assert_array_equal(s[0], full.sum(axis=0))
    np.testing.assert_array_equal(s[1], part.sum(axis=0))
    assert s[2] == ov


@pytest.mark.parametrize("box,n", CASES)
def test_rdf_and_cn_from_one_sweep(B, ctxs, box, n):
    xyz, _, bx = frames(box, n)
    full, part, ov = oracle_rdf(box, n, False)
    cn = oracle_cn(box, n)
    for per_frame in (True, False):
        a = B.rdf_cn_loop(xyz, types_of(n, 3), bx, REL, R_CUT, DDR, NBINS, CUTS, per_frame=per_frame, ctx=ctxs[0])
        assert packed(ctxs[0]).endswith(", true>")  # the CN-checking instantiation
        np.testing.assert_array_equal(a[0], full if per_frame else full.sum(axis=0))
        np.testing.assert_array_equal(a[1], part if per_frame else part.sum(axis=0))
        assert a[2] == ov
        np.testing.assert_array_equal(a[3], cn if per_frame else cn.sum(axis=0))


@pytest.mark.parametrize("box,n", CASES)
def test_class_rows_with_nine_types(B, ctxs, box, n):
    xyz, _, bx = frames(box, n)
    full, part, ov = oracle_rdf(box, n, True)
    for per_frame in (True, False):
        a = B.rdf_loop(xyz, types_of(n, 9), bx, REL9, R_CUT, DDR, NBINS, per_frame=per_frame, ctx=ctxs[1])
        packed(ctxs[1], ("<5,", "<6,"))
        np.testing.assert_array_equal(a[0], full if per_frame else full.sum(axis=0))
        np.testing.assert_array_equal(a[1], part if per_frame else part.sum(axis=0))
        assert a[2] == ov


@pytest.mark.parametrize("box,n", CASES)
def test_atoms_x_sites(B, ctxs, box, n):
    xyz, sites, bx = frames(box, n)
    ty, st = types_of(n, 3), (1 + np.arange(n) % 2).astype(np.int32)
    rel = np.array([[1, 1], [2, 2], [3, 1], [3, 2]])
    want = [C.rdf_rect(xyz[f], ty, sites[f], st, rel, bx[f], R_CUT * R_CUT, DDR, NBINS) for f in range(FRAMES)]
    part, ov = np.stack([w[0] for w in want]), sum(w[1] for w in want)
    for per_frame in (True, False):
        a = B.rdf_mol_loop(xyz, ty, sites, st, bx, rel, R_CUT, DDR, NBINS, per_frame=per_frame, ctx=ctxs[0])
        packed(ctxs[0])
        np.testing.assert_array_equal(a[0], part if per_frame else part.sum(axis=0))
        assert a[1] == ov
