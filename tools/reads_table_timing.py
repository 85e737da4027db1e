"""Timing of the aligner's read table (csrc/hgx_reads.hip against load_reads of csrc/hgx_align_host.cpp): the same inflated paired
FASTQ texts, 2 x 100 bp, through engine.Reads.from_text with front=device (upload included: the texts start in host memory) and
with front=host, at 1 K / 4 K / 16 K / 64 K / 1 M reads (and 64 .. 512 and 2 K reads beside them, around the break-even); median of 5
after one warm-up.  Prints one row per size -- bytes of text,
ms either way, the ratio -- and the break-even: the smallest measured text from which the device table is the faster one (the
gate HGX_RD_GATE is that, rounded up to a power of two).

    python tools/reads_table_timing.py [--max-reads N]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import align, capi, engine  # noqa: E402

SIZES = [1 << 6, 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12, 1 << 14, 1 << 16, 1 << 20]


def texts(n_reads, seed=1):
    """Two FASTQ texts of n_reads / 2 records each, 100 bases a read."""
    rng = np.random.default_rng(seed)
    n = n_reads // 2
    out = []
    for mate in range(2):
        seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, 100))]
        quals = (rng.integers(0, 40, size=(n, 100)) + 35).astype(np.uint8)
        out.append(b"".join(b"@read%09d/%d\n%s\n+\n%s\n" % (k, mate + 1, seqs[k].tobytes(), quals[k].tobytes()) for k in range(n)))
    return out


def run(t, switch, reps=6):
    ts, made = [], None
    with engine.test_switches(front=switch):
        for _ in range(reps):
            t0 = time.perf_counter()
            r = engine.Reads.from_text(t)
            ts.append((time.perf_counter() - t0) * 1e3)
            made = (r.route, r.decline, r.n_reads)
            r.close()
    return statistics.median(ts[1:]), made


def main():
    capi.set_device(0)
    top = int(sys.argv[sys.argv.index("--max-reads") + 1]) if "--max-reads" in sys.argv else SIZES[-1]
    print("reads | text bytes | device table ms (upload included) | host loader ms | host / device")
    even = None
    for n in [s for s in SIZES if s <= top]:
        t = texts(n)
        nb = sum(map(len, t))
        dev, made = run(t, "device")
        assert made == (2, 0, n), made
        host, made_h = run(t, "host")
        assert made_h == (0, align.READS_DECLINE_SWITCH, n), made_h
        print("%7d | %10d | %8.3f | %8.3f | x%.2f" % (n, nb, dev, host, host / dev), flush=True)
        if even is None and dev < host:
            even = nb
    if even is None:
        print("the device table was never the faster one")
    else:
        gate = 1
        while gate < even:
            gate <<= 1
        print("break-even at or below %d bytes of text -> gate %d (HGX_RD_GATE is %d)" % (even, gate, align.READS_GATE))


if __name__ == "__main__":
    main()
