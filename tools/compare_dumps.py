#!/usr/bin/env python3
"""`bench.py --dump-outputs DIR` of two builds: is every array equal (==, not close)?  tools/compare_dumps.py <dir a> <dir b>"""
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
ok = True
for n in sorted(set(os.listdir(a)) | set(os.listdir(b))):
    pa, pb = os.path.join(a, n), os.path.join(b, n)
    if not (os.path.exists(pa) and os.path.exists(pb)):
        print("%-24s only in one directory" % n)
        ok = False
        continue
    x, y = np.load(pa), np.load(pb)
    same = x.shape == y.shape and np.array_equal(x, y)
    print("%-24s %-12s %s" % (n, x.shape, "equal" if same else "DIFFERENT"))
    ok = ok and same
print("ALL EQUAL" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
