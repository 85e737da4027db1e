#!/usr/bin/env python3
"""Per kernel of a traced bench run: launches, launches per step, average duration, sum per step.
tools/kernel_per_step.py <rocprofv3 kernel_trace.csv>   (a step = one k_piece_compat launch)"""
import collections
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
steps = sum(1 for r in rows if "k_piece_compat" in r["Kernel_Name"])
acc = collections.defaultdict(lambda: [0, 0])
for r in rows:
    n = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", ""))
    a = acc[n]
    a[0] += 1
    a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
print("# steps (k_piece_compat launches): %d" % steps)
print("# %-44s %8s %9s %9s %12s" % ("kernel", "launches", "per_step", "avg_us", "sum_per_step"))
for n, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
    print("  %-44s %8d %9.2f %9.2f %12.2f" % (n[:44], c, c / max(steps, 1), t / c / 1e3, t / max(steps, 1) / 1e3))
