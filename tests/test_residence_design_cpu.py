"""
The closed-form residence counts of tests/residence_design.py against the brute-force oracle
(oracle.cpu_ref.shell_indicator + residence_counts) on the same coordinates: the reference the long and large GPU
tests of tests/test_gpu_residence.py compare with is proven here first. No GPU.
"""
import numpy as np
import pytest

import residence_design as RD


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("same", [False, True])
def test_design_closed_form_equals_oracle(F, same):
    pats = RD.patterns(F, seed=F)
    groups = [(pats["always"], 2, 3), (pats["run"], 1, 2), (pats["periodic"], 3, 1), (pats["random"], 2, 2),
              (pats["ends"], 1, 3), (pats["never"], 2, 1)]
    d = RD.designed(groups, seed=F, same=same)
    want, n_want = RD.oracle_counts(d, same=same)
    np.testing.assert_array_equal(d.counts, want)
    assert d.n_records == n_want
    assert d.counts[0] > 0


def test_design_large_box_and_unwrapped_coordinates():
    """A box far larger than the lattice (the re-sweep cluster's setting); the central atoms' whole-box jumps are real."""
    F = 40
    pats = RD.patterns(F, seed=3)
    d = RD.designed([(pats["always"], 4, 4), (pats["periodic"], 2, 3)], seed=3, box=(1000.0, 1000.0, 1000.0))
    assert np.abs(d.xi).max() > 900.0  # some central atoms sit a box length away from their cluster
    want, n_want = RD.oracle_counts(d)
    np.testing.assert_array_equal(d.counts, want)
    assert d.n_records == n_want == 16 * F + 6 * int(pats["periodic"].sum())


def test_acorr_fft_path_is_exact():
    """Above 2048 frames acorr() takes an FFT and rounds: it must equal the direct integer sum."""
    for F in (2049, 5000):
        for name, p in RD.patterns(F, seed=F).items():
            q = np.asarray(p, dtype=np.int64)
            np.testing.assert_array_equal(RD.acorr(p), np.correlate(q, q, "full")[F - 1:], err_msg=name)


def test_acorr_closed_forms():
    F = 1000
    pats = RD.patterns(F)
    np.testing.assert_array_equal(RD.acorr(pats["always"]), F - np.arange(F))
    ends = RD.acorr(pats["ends"])
    assert ends[0] == 2 and ends[F - 1] == 1 and ends[1:F - 1].sum() == 0
    assert not RD.acorr(pats["never"]).any()
