#!/usr/bin/env python
"""tools/sweep_gaps.py DIR — from a rocprofv3 --kernel-trace CSV output of a pipelined bench run: how the sweeps of
consecutive pair calls follow each other on the device. For the launches of the most frequent pair_hist_sj kernel that
follow the launch before them within a millisecond (the pipelined steps; the profiler's own overhead is in the numbers):

  period     start of sweep k -> start of sweep k + 1
  gap        end of sweep k -> start of sweep k + 1 (negative: the two sweeps overlap)
  pre-pass   summed duration of the kernels that start between the two sweep starts, sweep and its merge excluded
  hidden     how much of that pre-pass lies before the end of sweep k, i.e. under it
"""
import collections
import csv
import glob
import re
import sys

import numpy as np

d = sys.argv[1]
rows = []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
names = collections.Counter(n for _s, _e, n in rows if "pair_hist_sj_kernel" in n)
sweep_name = names.most_common(1)[0][0]
sweeps = [(s, e) for s, e, n in rows if n == sweep_name]
med = np.median([e - s for s, e in sweeps])
period, gap, pre, hidden, dur = [], [], [], [], []
for (s0, e0), (s1, e1) in zip(sweeps[:-1], sweeps[1:]):
    if abs((e0 - s0) - med) > 0.2 * med or abs((e1 - s1) - med) > 0.2 * med or s1 - e0 > 1_000_000:
        continue
    period.append(s1 - s0)
    gap.append(s1 - e0)
    dur.append(e0 - s0)
    between = [(s, e) for s, e, n in rows if s0 < s < s1 and "pair_hist_sj_kernel" not in n and "merge_slices" not in n]
    pre.append(sum(e - s for s, e in between))
    hidden.append(sum(max(0, min(e, e0) - s) for s, e in between))
us = lambda v: np.median(v) / 1e3
print("%s: %d launches, %d pipelined pairs of them" % (re.search(r"pair_hist_sj_kernel<[^>]*>", sweep_name).group(0), len(sweeps), len(period)))
print("median per pipelined step: sweep %.1f us   period %.1f us   gap end -> next start %.1f us   "
      "pre-pass kernels %.1f us, of which under the sweep before %.1f us" % (us(dur), us(period), us(gap), us(pre), us(hidden)))
print("gap quartiles: %.1f / %.1f / %.1f us" % tuple(np.percentile(gap, [25, 50, 75]) / 1e3))
