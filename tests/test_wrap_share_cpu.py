"""tools/wrap_share.py, the CPU model of the packed sweep's image rules, on 2048 random atoms: the wave-uniform image
never flags an axis that the per-lane rule leaves plain, and every pair that the plain or the shift path handles meets
the condition that makes those paths valid — the difference used is the reference's single-wrap distance on that axis, or
both lie beyond the cutoff on that axis alone."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import wrap_share as W  # noqa: E402


@pytest.mark.parametrize("L,r_cut", [(25.0, 10.0), (25.0, 12.45), ((25.0, 31.0, 40.0), 10.0)])
def test_image_rules_on_2048_atoms(L, r_cut):
    rng = np.random.default_rng(77)
    Lv = np.broadcast_to(np.asarray(L, dtype=float), (3,))
    x = rng.uniform(0, 1, (3, 2048)) * Lv[:, None]
    g = W.geometry(x, Lv, r_cut)
    k = W.classify(g, np.arange(g["wc"].shape[1]))
    keep, state, today = k["keep"], k["state"], k["today"]
    assert keep.any() and np.array_equal(keep, k["keep_today"])  # no group leaves the packed path
    # never an axis flagged that the per-lane rule leaves plain
    assert not ((state != W.PLAIN) & ~today)[keep].any()
    assert (state == W.SHIFT)[keep].any() and (state == W.WRAP)[keep].any()
    shift_axis, wrapped = W.paths(state)
    xs, tc = g["xs"], g["tc"].astype(np.float32).astype(np.float64)
    th = Lv - r_cut - (1.0e-3 * Lv + 1.0e-3)
    checked = 0
    for w in range(keep.shape[0]):
        xi = xs[:, w * W.WAVE:(w + 1) * W.WAVE]  # [3, 64]
        for gi in np.flatnonzero(keep[w]):
            t = k["tile_of"][gi]
            xj = xs[:, gi * W.GROUP:(gi + 1) * W.GROUP]  # [3, 4]
            for ax in range(3):
                if wrapped[w, gi, ax]:
                    continue
                # d' = xr_i - xr_j with xr_i = (x_i - c) - n L, xr_j = x_j - c
                dp = ((xi[ax] - tc[ax, t]) - k["n"][w, t, ax] * Lv[ax])[:, None] - (xj[ax] - tc[ax, t])[None, :]
                d = xi[ax][:, None] - xj[ax][None, :]
                ref = np.abs(d - Lv[ax] * np.rint(d / Lv[ax]))  # the reference's single wrap (atoms inside the cell)
                if shift_axis[w, gi] == ax:
                    assert (np.abs(dp) >= Lv[ax] - th[ax]).all() and (np.sign(dp) == -k["shift_sign"][w, gi, ax]).all()
                    dp = dp + k["shift_sign"][w, gi, ax] * Lv[ax]
                else:
                    assert state[w, gi, ax] == W.PLAIN and (np.abs(dp) <= th[ax]).all()
                used = np.abs(dp)
                assert (np.isclose(used, ref, rtol=0, atol=1e-9) | ((used > r_cut) & (ref > r_cut))).all(), (w, gi, ax)
                checked += dp.size
    assert checked > 1_000_000


def test_long_box_reaches_the_per_lane_fallback():
    """The shape tests/test_gpu_pair_image.py uses for the fallback: swept groups on a fallback axis exist, on each long
    axis, and no group leaves the packed path."""
    rng = np.random.default_rng(4108)
    box = np.array([25.0, 25.0, 100.0])
    x = rng.uniform(0, 1, (3, 2048)) * box[:, None]
    for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        g = W.geometry(x[perm], box[perm], 10.0)
        k = W.classify(g, np.arange(g["wc"].shape[1]))
        on_fb = k["fallback"][:, k["tile_of"], :]  # [W, G, 3]
        assert np.array_equal(k["keep"], k["keep_today"])
        assert (k["keep"] & on_fb.any(axis=2)).sum() > 500
        assert on_fb[k["keep"]].any(axis=0).tolist() == [a == perm.index(2) for a in range(3)]
        # a fallback axis has no box bound: every group on it wraps
        assert (k["state"][on_fb] == W.WRAP).all()
