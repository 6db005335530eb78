"""tools/slot_share.py, the CPU model of where the packed sweep's pair slots go: the half-group rule it models (the box
of every 2 consecutive sorted atoms against the wave's box) is conservative — on random small frames no half that holds a
pair inside r_cut by the reference's own distance is ever dropped — with cells that do not start at the origin, stray
atoms outside the cell and cutoffs close to L/2; and the rule never keeps a half whose group the sweep drops today."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import slot_share as S  # noqa: E402
import wrap_share as W  # noqa: E402

N = 2048 + 37  # a ragged last tile, wave, group and half


def frame(rng, L, lo, strays):
    Lv = np.broadcast_to(np.asarray(L, dtype=float), (3,))
    x = np.asarray(lo, dtype=float)[:, None] + rng.uniform(0, 1, (3, N)) * Lv[:, None]
    if strays:  # atoms up to most of a box length outside the cell, on a random axis and side
        who = rng.choice(N, strays, replace=False)
        ax = rng.integers(0, 3, strays)
        x[ax, who] += rng.choice([-1.0, 1.0], strays) * rng.uniform(0.05, 0.9, strays) * Lv[ax]
    return x, Lv


@pytest.mark.parametrize("L,r_cut,lo,strays", [
    (25.0, 10.0, (0.0, 0.0, 0.0), 0),
    (25.0, 12.45, (0.0, 0.0, 0.0), 0),          # r_cut just under L/2
    (25.0, 12.45, (-7.5, 113.0, 2.0e3), 0),     # the cell does not start at the origin
    (25.0, 10.0, (-7.5, 113.0, 2.0e3), 40),     # and some atoms lie outside it
    ((25.0, 31.0, 40.0), 12.45, (3.0, -40.0, 0.0), 40),
    (25.0, 12.45, (0.0, 0.0, 0.0), 200),
])
def test_half_rule_never_drops_a_pair_inside_the_cutoff(L, r_cut, lo, strays):
    rng = np.random.default_rng([78, strays, int(100 * r_cut)])
    x, Lv = frame(rng, L, lo, strays)
    g = W.geometry(x, Lv, r_cut)
    xs = g["xs"]
    nW, nG = g["wc"].shape[1], g["gc"].shape[1]
    waves = np.arange(nW)
    keep = S.half_reach(g, waves)  # [W, G, 2]
    assert keep.shape == (nW, nG, 2)
    half_of = np.arange(N) // S.HALF
    r = S.reach_of(r_cut)
    group_keep = S.box_gap2(g["wc"].T, g["wh"].T, g["gc"].T, g["gh"].T, Lv) < r * r
    # a half box lies inside its group's box: the rule keeps nothing that the group test drops
    assert not (keep.any(axis=2) & ~group_keep).any()
    flat = keep.reshape(nW, -1)
    inside_pairs = dropped_halves = 0
    for w in waves:
        xi = xs[:, w * W.WAVE:(w + 1) * W.WAVE]
        inside = (S.ref_rsq(xi, xs, Lv) < r_cut * r_cut).any(axis=0)  # per j atom: some lane of the wave inside r_cut
        need = np.zeros(2 * nG, dtype=bool)
        need[half_of[inside]] = True
        assert not (need & ~flat[w]).any(), (w, np.flatnonzero(need & ~flat[w])[:4])
        inside_pairs += int(inside.sum())
        dropped_halves += int((~flat[w]).sum())
    # the case is not vacuous: pairs inside the cutoff exist, and so do dropped halves and one-half groups (few of
    # them at r_cut = 12.45 in a 25 A cell, where the cutoff sphere reaches most of the cell from anywhere)
    assert inside_pairs > 1000 and dropped_halves > 0
    assert (keep[..., 0] != keep[..., 1]).any()


def test_model_table_on_a_small_frame():
    """summarize(): the shares are ordered as the rules imply — exact <= per atom <= per half box <= per group."""
    rng = np.random.default_rng(79)
    x, Lv = frame(rng, 25.0, (0.0, 0.0, 0.0), 0)
    acc, split = S.summarize(W.geometry(x, Lv, 10.0))
    assert 0 < acc["live"] <= acc["half_atom"] <= acc["half_box"] <= acc["group"] <= acc["slots"]
    assert acc["lanes_in"] <= acc["lanes_live"]
    assert split["plain"].sum() + split["wrapping"].sum() > 0
