#!/usr/bin/env python
"""tools/dropin_host_path.py [--tree DIR] [n_atoms] [n_files] — wall time of the HOST path of calc_atomic_rdf (frame
stream on and off) and calc_atomic_cn alone: text dumps of tests/bench/bench_e2e.py's default shape (200 files x 10 000
atoms), the backend's pair loops replaced by stand-ins that return zeros. Needs no GPU. What is left is parsing,
batching, labels and densities, normalisation, the frame-ordered sum and the CSV. `--tree DIR` times the package of
another checkout (an A/B of two commits: run parent, branch, parent). One JSON line; every figure the best of 3."""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]
    tree = HERE
    if argv[:1] == ["--tree"]:
        tree, argv = os.path.abspath(argv[1]), argv[2:]
    sys.path.insert(0, tree)
    n = int(argv[0]) if argv else 10_000
    F = int(argv[1]) if len(argv) > 1 else 200
    from mdproptools_amd import backend, synth
    from mdproptools_amd.structural import rdf_cn

    def rdf_loop(xyz, types, box, rel, r_cut, ddr, nbins, per_frame=True, **kw):
        return (np.zeros((len(xyz), nbins), np.uint64), np.zeros((len(xyz), len(rel), nbins), np.uint64), 0)

    def cn_loop(xyz, types, box, rel, cuts, per_frame=True, **kw):
        return np.zeros((len(xyz), len(rel)), np.uint64)

    backend.rdf_loop, backend.cn_loop = rdf_loop, cn_loop
    L = 50.0 * (n / 10_000) ** (1 / 3)
    rel = [[a for a, b in synth.ALL_PAIRS_4], [b for a, b in synth.ALL_PAIRS_4]]
    mass = [1.0, 2.0, 3.0, 4.0]
    ty, ids = synth.rdf_types(n), np.arange(1, n + 1)
    with tempfile.TemporaryDirectory() as tmp:
        for f in range(F):
            x = synth.rdf_frames(n, [f], L, 2)[0]
            with open(os.path.join(tmp, "dump.nvt.%d.dump" % (f * 1000)), "wt") as fh:
                fh.write("ITEM: TIMESTEP\n%d\nITEM: NUMBER OF ATOMS\n%d\nITEM: BOX BOUNDS pp pp pp\n" % (f * 1000, n))
                fh.write(("0.0 %r\n" % L) * 3)
                fh.write("ITEM: ATOMS id type x y z\n")
                np.savetxt(fh, np.column_stack([ids, ty, x.T]), fmt="%d %d %.6f %.6f %.6f")
        pattern = os.path.join(tmp, "dump.nvt.*.dump")

        def best(call):
            times = []
            for _ in range(4):  # the first pass pays the page-table population of the fresh files: not counted
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            return round(min(times[1:]), 4)

        out = {"tree": tree, "n_atoms": n, "n_files": F}
        for on in (True, False):
            rdf_cn.STREAM = on
            out["calc_atomic_rdf_stream_%s_s" % ("on" if on else "off")] = best(
                lambda: rdf_cn.calc_atomic_rdf(20.0, 0.05, 4, mass, rel, pattern, path_or_buff=os.path.join(tmp, "rdf.csv")))
        rdf_cn.STREAM = True
        out["calc_atomic_cn_s"] = best(
            lambda: rdf_cn.calc_atomic_cn([2.325 + 0.5 * k for k in range(10)], 0.05, 4, mass, rel, pattern,
                                          path_or_buff=os.path.join(tmp, "cn.csv")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
