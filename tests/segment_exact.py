"""
Exact host restatement of the per-molecule reductions (mdhip_segment_com, mdhip_charge_flux), no GPU and no torch.

The arithmetic include/mdhip.h and csrc/segment_com.hip state, one IEEE double operation per numpy operation (numpy never
fuses a product into an addition):

    msum[s] = ((0.0 + m[lo]) + m[lo + 1]) + ...                                   host, index order (seg_sums)
    com[f, k, s] = (((0.0 + a[lo] * m[lo]) + a[lo + 1] * m[lo + 1]) + ...) / msum[s]          every product rounded
    tmp[f, k, s] = ((com[f, k, s] * vel_conv) * (qsum[s] * charge_conv))                              (mol_flux)
    J[k, t, f] = type_sum_kernel over the molecules of type t (a contiguous run):                     (type_sum)
                 256 partial sums, lane i adding tmp[lo + i], tmp[lo + i + 256], ... in that order from 0.0,
                 then red[i] += red[i + w] for w = 128, 64, ..., 1

Every kernel variant of the dispatch (segment_frame_kernel, segment_staged_kernel in its three stage sizes,
segment_com_kernel, mol_flux_kernel) does exactly these operations, so tests/test_gpu_segment_exact.py compares them
with assert_array_equal; which of them the dispatch must pick (expected_kernel below) is held against csrc/seg_plan.h
on the CPU (tests/test_seg_plan_native_cpu.py) and against the real call there. tests/test_segment_exact_cpu.py checks this file against Fraction arithmetic, against the
oracle and the golden, and that the data below is data on which the order of the additions shows.
"""
import numpy as np

VEL_CONV = 1e5  # (not 1: the conversions are operations of their own)
CHARGE_CONV = 1.602176634e-19
TYPE_LANES = 256  # threads of type_sum_kernel

# the GPU test's shapes: every table at FRAMES frames (not a multiple of the 3 frame slices of seg_gy 3) for each plane
# count of N_ATTR (a partial plane group of three: 1, 2, 4, 7), and the MANY_TABLES at MANY_FRAMES frames
FRAMES = 7
N_ATTR = (1, 2, 3, 4, 7)
MANY_FRAMES = 257
MANY_TABLES = ("four", "ragged")


def _lengths(off):
    off = np.asarray(off, dtype=np.int64)
    n = np.diff(off)
    assert off[0] >= 0 and (n > 0).all(), "segments must be non-empty and increasing"
    return off, n


def seg_sums(mass, q, off):
    """Per-segment sums of `mass` and of `q` (None: no charges) in index order from 0.0 -> (msum [M], qsum [M] | None)."""
    off, n = _lengths(off)
    mass = np.asarray(mass, dtype=np.float64)
    msum = np.zeros(len(n))
    qsum = None if q is None else np.zeros(len(n))
    for j in range(int(n.max(initial=0))):
        s = np.nonzero(n > j)[0]
        a = off[s] + j
        msum[s] = msum[s] + mass[a]
        if q is not None:
            qsum[s] = qsum[s] + np.asarray(q, dtype=np.float64)[a]
    return msum, qsum


def com(attr, mass, off):
    """attr [F, K, N] -> [F, K, M]: products rounded one by one, added in index order from 0.0, one division by the
    index-order mass sum. Vectorised over the segments by position inside the segment, so that every segment still
    adds its atoms one after the other."""
    attr = np.asarray(attr, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    off, n = _lengths(off)
    F, K, _ = attr.shape
    acc = np.zeros((F, K, len(n)))
    for j in range(int(n.max(initial=0))):
        s = np.nonzero(n > j)[0]
        a = off[s] + j
        acc[:, :, s] = acc[:, :, s] + attr[:, :, a] * mass[a]
    return acc / seg_sums(mass, None, off)[0]


def mol_flux(vel, mass, q, off, vel_conv=VEL_CONV, charge_conv=CHARGE_CONV):
    """vel [F, 3, N] -> q_mol * v_com per molecule [F, 3, M]: ((com * vel_conv) * (qsum * charge_conv))."""
    _, qsum = seg_sums(mass, q, off)
    return (com(vel, mass, off) * vel_conv) * (qsum * charge_conv)


def type_runs(seg_type, n_types):
    """[lo, hi) of every type's molecules; seg_type must be non-decreasing in 0..n_types-1 (the library's rule)."""
    st = np.asarray(seg_type, dtype=np.int64)
    assert (np.diff(st) >= 0).all() and (len(st) == 0 or (st.min() >= 0 and st.max() < n_types))
    lo = np.searchsorted(st, np.arange(n_types), side="left")
    hi = np.searchsorted(st, np.arange(n_types), side="right")
    return lo, hi


def type_sum(tmp, seg_type, n_types):
    """tmp [F, 3, M] -> J [3, n_types, F] in type_sum_kernel's order."""
    tmp = np.asarray(tmp, dtype=np.float64)
    F = tmp.shape[0]
    out = np.zeros((3, n_types, F))
    for t, (lo, hi) in enumerate(zip(*type_runs(seg_type, n_types))):
        red = np.zeros((F, 3, TYPE_LANES))
        for i0 in range(lo, hi, TYPE_LANES):  # lane i adds tmp[lo + i + 256 r] for r = 0, 1, ...
            w = min(TYPE_LANES, hi - i0)
            red[:, :, :w] = red[:, :, :w] + tmp[:, :, i0:i0 + w]
        w = TYPE_LANES // 2
        while w:
            red[:, :, :w] = red[:, :, :w] + red[:, :, w:2 * w]
            w //= 2
        out[:, t, :] = red[:, :, 0].T
    return out


def flux(vel, mass, q, off, seg_type, n_types, vel_conv=VEL_CONV, charge_conv=CHARGE_CONV):
    """vel [F, 3, N] -> J [3, n_types, F] (mdhip_charge_flux)."""
    return type_sum(mol_flux(vel, mass, q, off, vel_conv, charge_conv), seg_type, n_types)


# ------------------------------------------------------------------------------------------------------- test data
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def segment_tables():
    """name -> segment sizes. The shapes at which the dispatch changes form (csrc/seg_plan.h): pick_seg_cap takes
    512-atom stages for 3- and 10-atom molecules (the latter with three planes) and keeps 1024 for 4 and 16 (full runs
    of 256 and 64 molecules); one segment at each stage cap and one past it (the last two past every stage:
    segment_com_kernel / mol_flux_kernel); runs of one-atom segments at the 64 / 256 segments-per-block limits; ragged
    sizes (runs that start at odd atoms); one segment in all. Odd and even atom counts both occur (the 16-byte loads
    need an even one)."""
    rng = np.random.default_rng(20261016)
    small = lambda k: rng.integers(1, 9, k)  # noqa: E731
    t = {
        "water": np.full(701, 3),                        # 2103 atoms (odd)
        "ten": np.full(200, 10),
        "four": np.full(500, 4),
        "sixteen": np.full(128, 16),
        "ragged": np.concatenate([rng.integers(1, 41, 99), [2]]),
        "ones": np.concatenate([[3], np.ones(64, int), [5], np.ones(65, int), [2], np.ones(256, int), [7],
                                np.ones(257, int), [4], small(40)]),
        "single": np.array([9]),
    }
    for L in (256, 257, 512, 513, 1024, 1025):
        t["long%d" % L] = np.concatenate([small(41), [L], small(40)])
    return {k: np.asarray(v, dtype=np.int64) for k, v in t.items()}


def type_table():
    """Molecules of 1..4 atoms whose types hold 0, 1, 255, 256, 257, 0 and 600 molecules (type_sum_kernel: no lane
    busy, one, every lane but one, every lane once, one lane twice, more than two rounds) -> (sizes, seg_type, n_types)."""
    rng = np.random.default_rng(7)
    counts = [0, 1, 255, 256, 257, 0, 600]
    st = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    return rng.integers(1, 5, len(st)).astype(np.int64), st, len(counts)


def seg_types(M):
    """A type table for any segment count: thirds of the molecules as types 0, 2, 3; types 1 and 4 hold none."""
    return np.array([0, 2, 3], dtype=np.int32)[np.arange(M) * 3 // M], 5


def gen_masses(rng, n):
    """Non-dyadic masses and charges: every mass sum and product is rounded."""
    return rng.uniform(1.0, 40.0, n), rng.normal(0.0, 1.0, n)


def gen_attr(rng, F, K, off, origin=1e4):
    """[F, K, N]: each molecule around its own point up to +-`origin` (unwrapped coordinates), atoms scattered with
    magnitudes spanning six decades inside one molecule, so that the order of the additions and fused products show."""
    off, n = _lengths(off)
    centre = np.repeat(rng.uniform(-origin, origin, (1, K, len(n))), n, axis=2)
    return centre + rng.normal(0.0, 1.0, (F, K, int(off[-1]))) * 10.0 ** rng.uniform(-3, 3, (1, K, int(off[-1])))


def gen_vel(rng, F, off):
    """[F, 3, N] velocities of both signs and six decades of magnitude (no offset: molecules' sums cancel)."""
    return gen_attr(rng, F, 3, off, origin=0.0)


def _rng(name, *key):
    return np.random.default_rng(list(name.encode()) + [int(k) for k in key])


def case_masses(name, off):
    """The (mass, charge) arrays the GPU tests use for table `name`."""
    return gen_masses(_rng(name, 0), int(off[-1]))


def case_attr(name, off, F, K):
    """The COM input the GPU tests use for table `name` with F frames and K planes."""
    return gen_attr(_rng(name, 1, F, K), F, K, off)


def case_vel(name, off, F):
    """The velocities the GPU tests use for table `name` with F frames."""
    return gen_vel(_rng(name, 2, F), F, off)


# ------------------------------------------------------------------------------------- what the dispatch must pick
FALLBACK = {False: "segment_com_kernel", True: "mol_flux_kernel"}
# (seg_frame, seg_cap, seg_vec, seg_gy): seg_frame 1 with seg_cap 0 lets pick_seg_cap choose; seg_cap 256 is the
# wave-private staged form whatever seg_frame says; seg_vec and seg_gy act on the staged forms only
CONFIGS = [
    (1, 0, 1, 0),
    (1, 512, 1, 0),
    (1, 1024, 0, 3),
    (1, 256, 1, 3),
    (0, 0, 1, 0),
    (0, 0, 0, 3),
    (0, 512, 1, 1),
    (0, 512, 0, 0),
    (0, 1024, 1, 3),
    (0, 256, 0, 1),
    (0, 256, 1, 0),
]


def picked_cap(name, K):
    """pick_seg_cap's stage for the uniform tables (csrc/seg_plan.h): 512 for 3-atom molecules (a 256-molecule run
    fills 768 of 1024 atoms) and for 10-atom ones summed three planes at a time (306 sums take two rounds of 256 lanes);
    1024 for 4- and 16-atom ones (full runs)."""
    return {"water": 512, "ten": 512 if K >= 3 else 1024, "four": 1024, "sixteen": 1024}.get(name)


def expected_kernel(flux, cfg, sizes, name, K):
    """The kernel the dispatch must report (None: pick_seg_cap's choice on a table picked_cap does not list)."""
    frame, cap, _, _ = cfg
    mx = int(sizes.max())
    if mx > 1024:
        return FALLBACK[flux]
    fl = "true" if flux else "false"
    if cap == 0 and frame:
        c = 1024 if mx > 512 else picked_cap(name, K)
        if c is None:
            return None
    else:
        c = cap if cap in (256, 512) and mx <= cap else 1024  # (a stage too small for a segment: 1024)
    if c == 256:
        return "segment_staged_kernel<%s, 256, 64>" % fl
    if frame:
        return "segment_frame_kernel<%s, %d>" % (fl, c)
    return "segment_staged_kernel<%s, %d, 256>" % (fl, c)


def edge_geometry(n_probe=40, n_mol=800, ddr=0.07, r_cut=7.0, cn_cut=(3.1, 4.7, 5.3)):
    """One frame whose molecular sites sit within a few ulps of a histogram bin edge or a CN cutoff seen from a probe
    atom: each three-atom molecule is laid around its target point T = probe + r u (r = k * ddr or a cutoff) with
    mass-weighted displacements that cancel, so its COM is T up to rounding, and which bin it falls in depends on how the
    COM was rounded.
    -> dict(xyz [1, 3, n_probe + 3 n_mol], types [N] (probes 1, molecule atoms 2), attr [1, 3, 3 n_mol] (molecule
    atoms), mass, off, site_types [M] (1, 2), lengths [3], rel, r_cut, ddr, nbins, cn_cut)."""
    rng = np.random.default_rng(11)
    L = np.array([31.0, 32.0, 33.0])
    probes = rng.uniform(0.35, 0.65, (n_probe, 3)) * L
    nbins = int(r_cut / ddr)
    k = rng.integers(10, nbins, n_mol)
    r = np.where(np.arange(n_mol) % 4 == 3, np.asarray(cn_cut)[np.arange(n_mol) % len(cn_cut)], k * ddr)
    u = rng.normal(0.0, 1.0, (n_mol, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    T = probes[np.arange(n_mol) % n_probe] + r[:, None] * u
    m = rng.uniform(1.0, 40.0, (n_mol, 3))
    d = rng.normal(0.0, 0.8, (n_mol, 3, 3))  # [mol, atom, axis]
    d[:, 2] = -(m[:, 0, None] * d[:, 0] + m[:, 1, None] * d[:, 1]) / m[:, 2, None]
    atoms = (T[:, None, :] + d).reshape(-1, 3)
    xyz = np.concatenate([probes, atoms]).T[None].copy()
    types = np.concatenate([np.ones(n_probe), np.full(3 * n_mol, 2)]).astype(np.int32)
    return dict(xyz=xyz, types=types, attr=np.ascontiguousarray(atoms.T)[None], mass=m.reshape(-1),
                off=offsets(np.full(n_mol, 3)), site_types=(1 + np.arange(n_mol) % 2).astype(np.int32), lengths=L,
                rel=np.array([[1, 1], [1, 2], [2, 1]]), r_cut=r_cut, ddr=ddr, nbins=nbins, cn_cut=list(cn_cut))
