#!/usr/bin/env python3
"""
tools/wrap_share.py [C1|C2|C3] — where the packed pair sweep's periodic wraps come from (numpy only, no GPU).

A model of the sweep's geometry on frame 0 of a bench.py shape, with the rules of the kernel: the Hilbert order of
pair_cull.hip (32^3 grid from the sampled origin), tile boxes of 256 sorted atoms, wave boxes of 64, group boxes of 4
(centre + half extents, padded as cull_boxes_kernel pads them), the group test and the per-axis image rules of
sj_item_pk (pair_sj.hip). All pairs of the frame, not the triangular half; the tile-pair lists are not modelled (a group
that passes the group test lies in a listed tile).

Per (wave, group) that is swept and per axis, the axis is
    plain   the difference d' = xr_i - xr_j is used as it is,
    shift   every pair of the group lies at the other image: d' -+ L would do, one packed add per two slots
            (modelled only: the kernel wraps these axes per pair — the three extra instances of the group sweep
            measured slower than what they save),
    wrap    the per-pair f32 wrap, three packed instructions per two slots.
"per-lane" is the rule before the wave-uniform image: every lane at its own nearest image of the tile's centre, a box
bound only where all 64 lanes chose the same one. Printed: the share of groups swept, the wrapped axes per swept group
under each rule, the split of the groups by state and the wrap instructions per swept group (a group is two packed slots).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE, WAVE, GROUP, BITS = 256, 64, 4, 5
PLAIN, SHIFT, WRAP = 0, 1, 2


def hilbert3(cx, cy, cz):
    """pair_cull.hip hilbert3 (Skilling's transpose algorithm) on arrays of cell indices."""
    X = [cx.astype(np.uint32).copy(), cy.astype(np.uint32).copy(), cz.astype(np.uint32).copy()]
    M = 1 << (BITS - 1)
    Q = M
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            hit = (X[i] & Q) != 0
            t = (X[0] ^ X[i]) & P
            x0 = np.where(hit, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = np.where(hit, X[i], X[i] ^ t)
            X[0] = x0
        Q >>= 1
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    X = [x ^ t for x in X]
    key = np.zeros_like(X[0])
    for b in range(BITS - 1, -1, -1):
        for i in range(3):
            key = (key << 1) | ((X[i] >> b) & 1)
    return key


def sort_order(x, L):
    """The order of the spatial sort for one frame x [3, n] (atoms of one cell keep their input order here)."""
    n = x.shape[1]
    stride = n // 1024 if n > 1024 else 1
    origin = x[:, : 1024 * stride : stride].min(axis=1)
    G = 1 << BITS
    c = []
    for ax in range(3):
        d = x[ax] - origin[ax]
        d = np.where((d < 0) & (d >= -L[ax] / 64.0), 0.0, d)
        s = d / L[ax]
        f = s - np.floor(s)
        f = np.where(f < 1.0, f, 0.0)
        c.append(np.clip((f * G).astype(np.int64), 0, G - 1))
    return np.argsort(hilbert3(*c), kind="stable")


def _boxes(xs, size, L):
    """(centre, half extent) [3, n_boxes] of every `size` consecutive atoms, as cull_boxes_kernel's `centred`."""
    n = xs.shape[1]
    starts = np.arange(0, n, size)
    lo = np.minimum.reduceat(xs, starts, axis=1)
    hi = np.maximum.reduceat(xs, starts, axis=1)
    pad = 1e-5 * L.sum() + 1e-6 + 2.5e-7 * np.maximum(np.abs(lo), np.abs(hi))
    c = (0.5 * (lo + hi)).astype(np.float32).astype(np.float64)
    return c, np.maximum(hi - c, c - lo) + pad


def geometry(x, L, r_cut):
    """Sorted frame and its boxes. x [3, n] as given, L [3]."""
    L = np.broadcast_to(np.asarray(L, dtype=float), (3,)).copy()
    xs = x[:, sort_order(x, L)]
    n = xs.shape[1]
    starts = np.arange(0, n, TILE)
    tlo = np.minimum.reduceat(xs, starts, axis=1)
    thi = np.maximum.reduceat(xs, starts, axis=1)
    tc = 0.5 * (tlo + thi)
    edge = np.cbrt(TILE * L.prod() / n)
    g = dict(xs=xs, L=L, r_cut=float(r_cut), tc=tc, the=np.maximum(thi - tc, tc - tlo), s_cap=r_cut + 3.5 * edge)
    g["wc"], g["wh"] = _boxes(xs, WAVE, L)
    g["gc"], g["gh"] = _boxes(xs, GROUP, L)
    return g


def classify(g, waves):
    """The kernel's tests for the waves `waves` (indices) against every group of the frame.
    Returns keep [W, G] (the group is swept by the packed path), today [W, G, 3] (axis flagged for the per-pair wrap
    under the per-lane image rule), state [W, G, 3] (PLAIN / SHIFT / WRAP under the wave-uniform image; SHIFT is the
    per-axis state: the kernel runs its shift variant only when the other two axes are plain, see `paths`),
    n [W, T, 3] (the wave's image per tile), fallback [W, T, 3], shift_sign [W, G, 3] (the sign of the added L)."""
    L, r_cut = g["L"], g["r_cut"]
    wc, wh = g["wc"][:, waves].T, g["wh"][:, waves].T  # [W, 3]
    gc, gh = g["gc"].T, g["gh"].T  # [G, 3]
    nG, nT = gc.shape[0], g["tc"].shape[1]
    tile_of = np.arange(nG) // (TILE // GROUP)
    c = g["tc"].T.astype(np.float32).astype(np.float64)  # [T, 3]
    he = g["the"].T
    th = L - r_cut - (1.0e-3 * L + 1.0e-3)
    cap = g["s_cap"] * (1.0 - 1.0e-6)
    rel = wc[:, None, :] - c[None, :, :]  # [W, T, 3]
    hw = wh[:, None, :]
    # today: every lane at its own nearest image; a box bound only when the whole box sits at one image
    n0 = np.rint((rel - hw) / L - 1.0e-3)
    n1 = np.rint((rel + hw) / L + 1.0e-3)
    same = n0 == n1
    thc_today = np.where(same, th - 1.0e-6 * np.abs(c)[None], -1.0)
    wmax_today = np.where(same, np.abs(rel - n0 * L) + hw, 0.5000001 * L)
    # the wave-uniform image, and the per-lane fallback where one image would leave the error bound's cover
    nu = np.rint(rel / L)
    wmax_u = np.abs(rel - nu * L) + hw
    fb = ~same & ~(wmax_u + he[None] < cap) & (0.5000001 * L + he[None] < cap)
    thc = np.where(fb, -1.0, th - 1.0e-6 * np.abs(c)[None])
    wmax = np.where(fb, 0.5000001 * L, wmax_u)
    base = (np.abs(rel) + hw + he[None] < 1.49 * L) & (he[None] < 0.9 * L)
    covered_today = (base & (wmax_today + he[None] < cap)).all(axis=2)  # [W, T]
    covered = (base & (wmax + he[None] < cap)).all(axis=2)
    # group test: the nearest image of the centres' difference minus the half extents
    d = wc[:, None, :] - gc[None, :, :]  # [W, G, 3]
    s = wh[:, None, :] + gh[None, :, :]
    gap = np.maximum(np.abs(d - np.rint(d / L) * L) - s, 0.0)
    reach = (r_cut + 1e-3) * 1.00001
    keep = (gap * gap).sum(axis=2) < reach * reach
    D_today = (wc[:, None, :] - n0 * L)[:, tile_of, :] - gc[None]
    today = ~(np.abs(D_today) + s <= thc_today[:, tile_of, :])
    D = (wc[:, None, :] - nu * L)[:, tile_of, :] - gc[None]
    thc_g = thc[:, tile_of, :]
    plain = np.abs(D) + s <= thc_g
    shift = ~plain & (thc_g >= 0) & (np.abs(D) - s >= L - thc_g)
    state = np.where(plain, PLAIN, np.where(shift, SHIFT, WRAP))
    return dict(keep=keep & covered[:, tile_of], keep_today=keep & covered_today[:, tile_of], today=today, state=state,
                n=nu, fallback=fb, shift_sign=-np.sign(D), tile_of=tile_of)


def paths(state):
    """Per (wave, group): the axis that runs the shift variant (-1: none) and the axes that take the per-pair wrap —
    a shift axis next to any other axis that is not plain takes the per-pair wrap with it."""
    nonplain = state != PLAIN
    single = (nonplain.sum(axis=-1) == 1) & (state == SHIFT).any(axis=-1)
    shift_axis = np.where(single, np.argmax(state == SHIFT, axis=-1), -1)
    return shift_axis, nonplain & ~single[..., None]


def summarize(g, chunk=32):
    nW = g["wc"].shape[1]
    acc = dict(pairs=0, swept=0, today_axes=0.0, uni_axes=0.0, wrap_axes=0.0, all_plain=0, single=0, mixed=0, wrap_only=0,
               fallback=0, triples=0, lost=0)
    for w0 in range(0, nW, chunk):
        k = classify(g, np.arange(w0, min(nW, w0 + chunk)))
        keep = k["keep"]
        shift_axis, wrapped = paths(k["state"])
        nonplain = k["state"] != PLAIN
        acc["pairs"] += keep.size
        acc["swept"] += int(keep.sum())
        acc["today_axes"] += int(k["today"][k["keep_today"]].sum())
        acc["uni_axes"] += int(nonplain[keep].sum())
        acc["wrap_axes"] += int(wrapped[keep].sum())
        anyshift = (k["state"] == SHIFT).any(axis=-1)
        acc["all_plain"] += int((~nonplain.any(axis=-1))[keep].sum())
        acc["single"] += int((shift_axis >= 0)[keep].sum())
        acc["mixed"] += int((anyshift & (shift_axis < 0))[keep].sum())
        acc["wrap_only"] += int((nonplain.any(axis=-1) & ~anyshift)[keep].sum())
        acc["fallback"] += int(k["fallback"].sum())
        acc["triples"] += k["fallback"].size
        acc["lost"] += int((k["keep_today"] & ~keep).sum())
    return acc


def report(name):
    from mdproptools_amd import synth

    cfg = synth.rdf_config(name)
    x = synth.rdf_frames(cfg["n_atoms"], [0], cfg["box_len"], cfg["seed_offset"])[0]
    a = summarize(geometry(x, cfg["box_len"], cfg["r_cut"]))
    sw = float(a["swept"])
    print("%s frame 0: %d atoms, L = %.3f, r_cut = %.1f" % (name, cfg["n_atoms"], cfg["box_len"], cfg["r_cut"]))
    print("groups swept                         %.1f %% of the (wave, group) pairs" % (100.0 * sw / a["pairs"]))
    print("wrapped axes per swept group   per-lane image %.3f   wave-uniform image %.3f   with a single-axis shift %.3f"
          % (a["today_axes"] / sw, a["uni_axes"] / sw, a["wrap_axes"] / sw))
    print("swept groups by state                all plain %.1f %%   shift on one axis, two plain %.1f %%   "
          "shift with another axis not plain %.1f %%   wrap only %.1f %%"
          % tuple(100.0 * a[k] / sw for k in ("all_plain", "single", "mixed", "wrap_only")))
    # per group (two packed slots): 6 packed instructions per wrapped axis, 2 per shifted one
    print("wrap instructions per swept group    per-lane image %.2f   wave-uniform image %.2f   with a single-axis shift %.2f"
          % (6 * a["today_axes"] / sw, 6 * a["uni_axes"] / sw, (6 * a["wrap_axes"] + 2 * a["single"]) / sw))
    print("per-lane fallback                    %d of %d (wave, tile, axis); groups leaving the packed path: %d"
          % (a["fallback"], a["triples"], a["lost"]))


if __name__ == "__main__":
    for nm in sys.argv[1:] or ["C2"]:
        report(nm)
