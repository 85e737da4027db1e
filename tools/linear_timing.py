"""Device-route timing of linear-index typing (csrc/hgx_linear.hip): 1 M groups x up to 10 records of a CODIS-like locus, SAM
text in host memory -> Gene_counts + Gene_cmpt.  Prints ms per call (median of 5 after one warm-up) and bytes sent per record."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import importlib  # noqa: E402
import random  # noqa: E402

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import capi, engine, synth  # noqa: E402
from hisatgenotype_amd.locus import PackedLocus  # noqa: E402
from test_gpu_linear import random_sam  # noqa: E402

ht = importlib.import_module("hisatgenotype_amd.typing")


def main():
    capi.set_device(0)
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    sam = random_sam(loc, random.Random(5), 1000000, 10).encode()
    n_rec = sam.count(b"\n")
    ts = []
    with engine.test_switches(front="device"):
        for k in range(6):
            t0 = time.perf_counter()
            ht.linear_counts(pl, sam, "bowtie2")
            ts.append((time.perf_counter() - t0) * 1e3)
        route = engine.front_last()
        nbytes = engine.front_last_bytes()
    with engine.test_switches(front="host"):
        t0 = time.perf_counter()
        ht.linear_counts(pl, sam, "bowtie2")
        t_host = (time.perf_counter() - t0) * 1e3
    print("records %d, text %.1f MB, route %s | device route %.1f ms (median of 5) | host route %.1f ms | %.1f bytes sent per record"
          % (n_rec, len(sam) / 1e6, route, statistics.median(ts[1:]), t_host, nbytes / n_rec))
    pl.close()


if __name__ == "__main__":
    main()
