"""Timing of read extraction from a BAM (csrc/hgx_extract.hip: hgx_extract_feed_bam): the synthetic stream of tools/extract_timing.py,
cut down so that its records stay under 1 GB, written as a BAM; one feed of the file's deflated bytes, upload and copy back included,
median of 5 after a warm-up, for the device route and for front=host; then hgx_extract_file on the same BAM (on a checkout without
hgx_extract_feed_bam that is the one-piece path: host inflate + text + feed), and the device / host break-even over small chunks.

The figure of the commit before hgx_extract_feed_bam is taken ON a checkout of that commit, with a copy of this file and
`--file-only`: only hgx_extract_file is timed there (it has no feed_bam), never on the code under test.

    python tools/extract_bam_timing.py [n_pairs] [--file-only]"""
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import bamio, capi, engine, extract  # noqa: E402
from extract_timing import FAMILIES, REGIONS  # noqa: E402

REFS = [(str(c), 250_000_000) for c in range(1, 23)] + [("X", 250_000_000)]


def run(call, switch, reps):
    ts, st, n_out = [], None, 0
    with engine.test_switches(front=switch):
        for _ in range(reps):
            ex = extract.Extractor(REGIONS, FAMILIES, "hisat2", True, False, True)
            t0 = time.perf_counter()
            call(ex)
            ts.append((time.perf_counter() - t0) * 1e3)
            st = ex.stats()
            n_out = sum(len(ex.take(f, m)) for f in range(len(FAMILIES)) for m in range(2))
            ex.close()
    return ts, st, n_out


def as_bam(sam, tmp, name):
    path = os.path.join(tmp, name)
    bamio.write_bam_native(path, sam, REFS)
    with open(path, "rb") as f:
        return path, f.read()


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1_500_000      # ~3.1 M records, ~1.0e9 B of text
    capi.set_device(0)
    sam = extract.synth_stream(n_pairs, REGIONS, seed=3, hit_fraction=0.015, read_len=100)
    n_rec = sam.count(b"\n")
    with tempfile.TemporaryDirectory() as tmp:
        path, data = as_bam(sam, tmp, "stream.bam")
        inflated = sum(len(b) for b in bamio._bgzf_blocks(data))
        print("%d records, text %.1f MB, BAM %.1f MB deflated / %.1f MB inflated" % (n_rec, len(sam) / 1e6, len(data) / 1e6, inflated / 1e6), flush=True)
        fs, stf, n_out_f = run(lambda ex: ex.feed_file(path), "device", 6)
        print("hgx_extract_file %.1f ms (all %s) = %.2f M records/s, chunks %d device / %d host"
              % (statistics.median(fs[1:]), ["%.0f" % t for t in fs], n_rec / statistics.median(fs[1:]) / 1e3, stf["chunks_device"], stf["chunks_host"]))
        if "--file-only" in sys.argv or not hasattr(extract.Extractor, "feed_bam"):
            return
        ts, st, n_out = run(lambda ex: ex.feed_bam(data, last=True), "device", 6)
        assert st["route"] == 2 and n_out == n_out_f, st
        hs, sth, n_out_h = run(lambda ex: ex.feed_bam(data, last=True), "host", 3)
        assert n_out_h == n_out and sth["written"] == st["written"]
        dev_ms, host_ms = statistics.median(ts[1:]), statistics.median(hs[1:])
        print("feed_bam device route %.1f ms (all %s) = %.2f M records/s in %d chunks | front=host %.1f ms = %.2f M records/s | x%.1f"
              % (dev_ms, ["%.0f" % t for t in ts], n_rec / dev_ms / 1e3, st["chunks_device"], host_ms, n_rec / host_ms / 1e3, host_ms / dev_ms))
        lines = sam.split(b"\n")
        for n in (1000, 2000, 5000):
            _, part = as_bam(b"\n".join(lines[:n]) + b"\n", tmp, "part%d.bam" % n)
            d, _, _ = run(lambda ex: ex.feed_bam(part, last=True), "device", 8)
            h, _, _ = run(lambda ex: ex.feed_bam(part, last=True), "host", 8)
            print("  %6d records: device %.3f ms, host %.3f ms" % (n, statistics.median(d[2:]), statistics.median(h[2:])))


if __name__ == "__main__":
    main()
