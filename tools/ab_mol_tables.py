#!/usr/bin/env python
"""tools/ab_mol_tables.py OLD.so NEW.so [--out FILE] — mdhip_axis_vectors, mdhip_mol_moments, mdhip_dihedral_angles,
mdhip_mol_shape and mdhip_free_volume through two BUILDS of libmdhip.so in one process: the small calls of
tests/test_gpu_mol_tables.py (RUNS) and the refusing calls of the five families' invalid-argument tests. Every call of
the five entry points is recorded — its return code, the error text when it refuses, last_kernel and last_launches —
and every output array of the small calls is taken byte for byte. Any difference between the builds is printed and
makes the exit status 1."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401

from mdproptools_amd import _lib  # noqa: E402
from mdproptools_amd import backend as B  # noqa: E402

ENTRY_POINTS = ("mdhip_axis_vectors", "mdhip_mol_moments", "mdhip_dihedral_angles", "mdhip_mol_shape", "mdhip_free_volume")
REFUSING = (("test_gpu_reorientation", "test_axis_vectors_invalid_arguments"), ("test_gpu_dipole", "test_moments_invalid_arguments"),
            ("test_gpu_dihedrals", "test_invalid_arguments_leave_the_outputs_untouched"),
            ("test_gpu_shape", "test_invalid_arguments_leave_the_outputs_untouched"),
            ("test_gpu_free_volume", "test_arguments_are_refused_before_anything_is_written"))


def digest(value):
    if value is None:
        return "None"
    a = np.ascontiguousarray(value.cpu().numpy() if hasattr(value, "cpu") else value)
    return "%s%s:%s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()[:16])


def record(path):
    """Every call of the five entry points while RUNS and the refusing tests go through the build at `path`."""
    _lib._lib, _lib._default, _lib.STRICT, _lib.LIB_PATH = None, {}, False, os.path.abspath(path)
    os.environ.pop("MDHIP_LIB", None)
    lib = _lib.load(build_if_missing=False)
    log = []

    def wrap(name):
        call = getattr(lib, name)

        def recorded(h, *args):
            rc = call(h, *args)
            n = C.c_int(0)
            lib.mdhip_last_kernel_ms(h, C.byref(n))
            text = (lib.mdhip_last_error(h) or b"").decode() if rc else ""
            log.append("%s rc %d kernel %s launches %d %s" % (name, rc, (lib.mdhip_last_kernel_name(h) or b"").decode(), n.value, text))
            return rc

        setattr(lib, name, recorded)

    for name in ENTRY_POINTS:
        wrap(name)
    import test_gpu_mol_tables as T

    for label, run in T.RUNS:
        got = run(B)
        log.append("%s: %s" % (label, " ".join("%s=%s" % (k, digest(got[k])) for k in sorted(got))))
    for module, test in REFUSING:
        log.append("-- %s::%s" % (module, test))
        getattr(__import__(module), test)(B)
    return log


def main():
    libs = [a for a in sys.argv[1:] if a.endswith(".so")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if len(libs) != 2:
        raise SystemExit(__doc__)
    old, new = record(libs[0]), record(libs[1])
    lines = ["%s against %s: %d records (calls of the five entry points, output digests of the small calls)" % (libs[1], libs[0], len(new))]
    different = [(a, b) for a, b in zip(old, new) if a != b]
    if len(old) != len(new):
        different.append(("%d records" % len(old), "%d records" % len(new)))
    for a, b in different:
        lines += ["DIFFERENT", "  old: " + a, "  new: " + b]
    calls = [r for r in new if r.startswith("mdhip_")]
    lines.append("%d calls, %d of them refused; %d records differ" % (len(calls), sum(" rc 0 " not in r for r in calls), len(different)))
    lines += ["", "the records of %s:" % libs[1]] + new
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if different else 0)


if __name__ == "__main__":
    main()
