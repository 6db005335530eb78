#!/usr/bin/env python3
"""
tools/slot_share.py [C1|C2|C3 ...] — where the pair slots of the packed sweep go (numpy only, no GPU).

A slot is the 64 i atoms of one wave against one j atom. On frame 0 of a bench.py shape, with the geometry of
tools/wrap_share.py (Hilbert order, wave boxes of 64, group boxes of 4, padded as cull_boxes_kernel pads them), the share
of all (wave, j atom) slots that is
    swept today            the 4-atom group box comes within reach of the wave box (sj_item_pk's group test),
    swept per half, box    the same test on the box of each 2-atom half of a group (`half_reach`, the rule modelled for
                           a sweep that can leave one half of a group out),
    swept per half, atoms  a half is swept when one of its two atoms comes within reach of the wave box,
    live                   at least one of the 64 lanes is inside the cutoff (exact),
and the share of lanes inside the cutoff in a live slot. All pairs of the frame, not the triangular half; the tile-pair
lists and the cover test of the error bound are not modelled (a group that passes the group test lies in a listed tile).

The half-group rule is a MODEL: no kernel implements it. It was built once (2-atom boxes from cull_boxes_kernel, half masks in
sj_item_pk, one-half instances of the group sweep), measured slower than the sweep without it and taken out again:
DESIGN.md 9.001, profiles/halves_ab.txt. tests/test_slot_share_cpu.py shows the rule conservative.

Under the half-box rule, the swept groups split into "both halves in reach", "first half only" and "second half only",
for plain groups (no axis takes the per-pair wrap) and for wrapping ones: only plain groups outside the diagonal tile
could run a one-half instance of the group sweep.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wrap_share as W  # noqa: E402

HALF = 2


def reach_of(r_cut):
    """PairArgs::reach: the cutoff rounded up, plus slack for the f32 box test."""
    return (r_cut + 1e-3) * 1.00001


def box_gap2(wc, wh, bc, bh, L):
    """The kernel's box test: squared gap between wave boxes [W, 3] and boxes [B, 3] (centre, half extents), per axis
    the distance of the centres at the nearest image minus the half extents — a lower bound of the reference's
    per-axis distance min(|d|, ||d| - L|) of every pair of the two boxes, whatever image the atoms are given at."""
    d = wc[:, None, :] - bc[None, :, :]
    s = wh[:, None, :] + bh[None, :, :]
    gap = np.maximum(np.abs(d - np.rint(d / L) * L) - s, 0.0)
    return (gap * gap).sum(axis=2)


def half_boxes(g):
    """(centre, half extents) [3, 2 * n_groups] of every 2 consecutive sorted atoms, padded as the group boxes are;
    a half without atoms (ragged last group) gets half extents of -1e18, as an empty box does in cull_boxes_kernel."""
    hc, hh = W._boxes(g["xs"], HALF, g["L"])
    n_half = 2 * g["gc"].shape[1]
    if hc.shape[1] < n_half:
        extra = n_half - hc.shape[1]
        hc = np.concatenate([hc, np.zeros((3, extra))], axis=1)
        hh = np.concatenate([hh, np.full((3, extra), -1.0e18)], axis=1)
    return hc, hh


def half_reach(g, waves):
    """The rule of part 2: keep [W, G, 2] — half s of group G is swept by wave W iff the box of its two atoms comes
    within reach of the wave's box."""
    hc, hh = half_boxes(g)
    r = reach_of(g["r_cut"])
    keep = box_gap2(g["wc"][:, waves].T, g["wh"][:, waves].T, hc.T, hh.T, g["L"]) < r * r
    return keep.reshape(len(waves), -1, 2)


def ref_rsq(xi, xj, L):
    """The reference's squared distance (per axis min(|d|, ||d| - L|): its single wrap) of xi [3, A] x xj [3, B]."""
    a = np.abs(xi[:, :, None] - xj[:, None, :])
    a = np.minimum(a, np.abs(a - L[:, None, None]))
    return (a * a).sum(axis=0)


def summarize(g, chunk=8, wave_step=1):
    """Counts over every `wave_step`-th chunk of waves (the Hilbert order visits the whole cell, so a stride over the
    waves samples it evenly)."""
    xs, L, r_cut = g["xs"], g["L"], g["r_cut"]
    n, nW, nG = xs.shape[1], g["wc"].shape[1], g["gc"].shape[1]
    r = reach_of(r_cut)
    group_of = np.arange(n) // W.GROUP
    half_of = np.arange(n) // HALF
    acc = dict(slots=0, group=0, half_box=0, half_atom=0, live=0, lanes_in=0, lanes_live=0)
    split = {k: np.zeros(3, dtype=np.int64) for k in ("plain", "wrapping")}
    for w0 in range(0, nW, chunk * wave_step):
        waves = np.arange(w0, min(nW, w0 + chunk))
        wc, wh = g["wc"][:, waves].T, g["wh"][:, waves].T
        kg = box_gap2(wc, wh, g["gc"].T, g["gh"].T, L) < r * r  # [W, G]
        kh = half_reach(g, waves)  # [W, G, 2]
        # each atom against the wave box: a point is a box without extent
        ka = box_gap2(wc, wh, xs.T, np.zeros((n, 3)), L) < r * r  # [W, n]
        ka_half = np.zeros((len(waves), 2 * nG), dtype=bool)
        np.logical_or.at(ka_half, (slice(None), half_of), ka)
        acc["slots"] += len(waves) * n
        acc["group"] += int(kg[:, group_of].sum())
        acc["half_box"] += int(kh.reshape(len(waves), -1)[:, half_of].sum())
        acc["half_atom"] += int(ka_half[:, half_of].sum())
        for k, w in enumerate(waves):
            xi = xs[:, w * W.WAVE:(w + 1) * W.WAVE]
            inside = ref_rsq(xi, xs, L) < r_cut * r_cut  # [lanes, n]
            live = inside.any(axis=0)
            acc["live"] += int(live.sum())
            acc["lanes_in"] += int(inside[:, live].sum())
            acc["lanes_live"] += int(live.sum()) * xi.shape[1]
        state = W.classify(g, waves)["state"]
        plain = (state == W.PLAIN).all(axis=2)
        either = kh.any(axis=2)
        for name, sel in (("plain", plain), ("wrapping", ~plain)):
            m = either & sel
            split[name] += np.array([(m & kh[..., 0] & kh[..., 1]).sum(), (m & kh[..., 0] & ~kh[..., 1]).sum(),
                                     (m & ~kh[..., 0] & kh[..., 1]).sum()])
    return acc, split


def report(name, out=sys.stdout):
    from mdproptools_amd import synth

    cfg = synth.rdf_config(name)
    x = synth.rdf_frames(cfg["n_atoms"], [0], cfg["box_len"], cfg["seed_offset"])[0]
    step = 1 if cfg["n_atoms"] <= 20_000 else 16  # C3: 1563 waves, one chunk of 8 in every 16
    acc, split = summarize(W.geometry(x, cfg["box_len"], cfg["r_cut"]), wave_step=step)
    s = float(acc["slots"])
    p = lambda k: 100.0 * acc[k] / s  # noqa: E731
    out.write("%s frame 0: %d atoms, L = %.3f, r_cut = %.1f; share of all (wave, j atom) slots, %%%s\n"
              % (name, cfg["n_atoms"], cfg["box_len"], cfg["r_cut"], "" if step == 1 else " (every %dth chunk of 8 waves)" % step))
    out.write("  swept today (4-atom group box against wave box)                  %5.1f\n" % p("group"))
    out.write("  swept if tested per 2-atom half group (box against wave box)     %5.1f\n" % p("half_box"))
    out.write("  swept if tested per 2-atom half group (each atom against box)    %5.1f\n" % p("half_atom"))
    out.write("  at least one lane inside the cutoff (exact)                      %5.1f\n" % p("live"))
    out.write("  lanes inside the cutoff in a slot that is not skipped            %5.1f\n"
              % (100.0 * acc["lanes_in"] / acc["lanes_live"]))
    tot = float(split["plain"].sum() + split["wrapping"].sum())
    for k in ("plain", "wrapping"):
        v = 100.0 * split[k] / tot
        out.write("  swept groups, %-8s  both halves in reach %5.1f   first half only %4.1f   second half only %4.1f   "
                  "(%% of the groups swept under the half-box rule)\n" % (k, v[0], v[1], v[2]))


if __name__ == "__main__":
    for nm in sys.argv[1:] or ["C1", "C2", "C3"]:
        report(nm)
