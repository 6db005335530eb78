"""
The full-lag MSD plan is what the device runs: every case of tests/lag_plan_cases.py goes through backend.lag_msd with
the case's options, and the call leaves the kernel name and launch count that mdhip_lag_plan — given the context's own
options and device limits — predicted, takes no slow-path repeat, and writes a finite status word. No numeric check is
repeated here: tests/test_gpu_lag_exact.py and test_gpu_parity.py compare every path against exact sums and the oracle.
"""
import numpy as np
import pytest

import lag_plan_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from mdproptools_amd import backend

    return backend


@pytest.fixture(scope="module")
def ctx(B):
    return B.default_context()


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_plan_is_what_the_device_ran(B, ctx, name):
    case = P.CASES[name]
    want = P.plan(dict(case, opts={"lag_variant": 2, **case["opts"]}), cu_count=0, lds_bytes=0, ctx=ctx)
    assert want["status"] == 0, want
    got = P.run(case, B, ctx)
    print(name, got["kernel"], got["launches"], "bound %.3e status %.3e" % (got["bound"], got["status"]))
    assert (got["kernel"], got["launches"]) == (want["kernel"], want["launches"]), (got["kernel"], want)
    assert got["fallbacks"] == 0
    assert np.isfinite(got["status"]) and got["status"] >= 0.0
    assert got["out"].shape == (case["max_lag"] + 1, len(case["go"]) - 1, 4)
