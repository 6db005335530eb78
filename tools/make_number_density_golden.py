#!/usr/bin/env python
"""
tools/make_number_density_golden.py — tests/golden/number_density.npz from the REAL reference's calc_number_density.

Build container only (the reference is not on the GPU box; what travels is this script's output, as data):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_number_density_golden.py

The reference package is imported read-only with the stand-ins of oracle/shims (oracle/shims/README.md). Its function
names np.int and np.product, which numpy no longer has: both are aliased here (np.int = int, np.product = np.prod)
before the import, nothing else is touched.

Stored: the seeded frame sets (tests/number_density_ref.py frame_sets), per case of number_density_ref.CASES the
returned array, its column names and the CSV bytes — or the name of the exception's type — and the signature of the
reference's function (parameter names and the repr of their defaults).
"""

import contextlib
import inspect
import io
import os
import sys
import tempfile

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("MDPROPTOOLS_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(REPO, "oracle", "shims"), REPO, os.path.join(REPO, "tests"), REF]

import numpy as np  # noqa: E402

if not hasattr(np, "int"):
    np.int = int
if not hasattr(np, "product"):
    np.product = np.prod

from mdproptools.structural import number_density as ref  # noqa: E402  (the reference module)
import number_density_ref as R  # noqa: E402

OUT = os.environ.get("MDHIP_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden", "number_density.npz")


def run_ref(frames, **kw):
    with tempfile.TemporaryDirectory() as wd:
        pattern = R.write_dumps(frames, wd)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                df = ref.calc_number_density(pattern, working_dir=wd, **kw)
        except Exception as e:  # noqa: BLE001  (recorded: the drop-in must raise the same type)
            assert not os.path.exists(os.path.join(wd, "number_density.csv"))
            return None, None, type(e).__name__
        with open(os.path.join(wd, "number_density.csv"), "rb") as fh:
            return df, fh.read(), ""


def main():
    store = {}
    for key, frames in R.frame_sets().items():
        store[key + "_xyz"] = np.stack([f["xyz"] for f in frames])
        store[key + "_type"] = np.stack([f["types"] for f in frames]).astype(np.int8)
        store[key + "_bounds"] = np.stack([f["bounds"] for f in frames])
        store[key + "_timestep"] = np.array([f["timestep"] for f in frames], dtype=np.int64)
    sig = inspect.signature(ref.calc_number_density)
    store["sig_names"] = np.array(list(sig.parameters))
    store["sig_defaults"] = np.array(["<required>" if p.default is inspect.Parameter.empty else repr(p.default)
                                      for p in sig.parameters.values()])
    for key in R.CASES:
        frames, kw = R.case_args(store, key)
        df, csv, err = run_ref(frames, **kw)
        store[key + "_error"] = np.array(err)
        if err:
            print(key, "raises", err)
            continue
        store[key + "_csv"] = np.frombuffer(csv, dtype=np.uint8)
        store[key + "_values"] = df.to_numpy()
        store[key + "_columns"] = np.array([str(c) for c in df.columns])
        print(key, df.shape, "column sums", df.iloc[:, 1:].to_numpy().sum(axis=0))
    for key in R.CASES:
        assert str(store[key + "_error"]) == R.RAISES.get(key, ""), (key, store[key + "_error"])
    assert store["no_surface_values"][:, 1:].sum() == 0.0
    assert store["wrap_values"][-6:, 1:].sum() > 0.0  # the wrapped atoms sit in the top bins
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
