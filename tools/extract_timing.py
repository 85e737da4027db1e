"""Timing of read extraction (csrc/hgx_extract.hip): a seeded HISAT2-like SAM stream already in host memory, >= 5 M records, most
of them outside every region and 1-2 % of the pairs hits -> the FASTQ text per family.  Prints, for the device route and the host
route (one hgx_extract_feed of the whole text, upload included; median of 5 after one warm-up): ms, records/s, bytes sent per
record, the record pass's byte model against HBM peak, and the device / host break-even over small chunks (the gate).

    python tools/extract_timing.py [n_pairs] [--reference-loop]     (--reference-loop: the spec's Python loop on 1/50 of the text)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import capi, engine, extract  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X
FAMILIES = ["hla", "codis", "cyp"]
REGIONS = [("hla", "6", 29_900_000 + 40_000 * k, 29_900_000 + 40_000 * k + 6_000) for k in range(20)] + \
          [("codis", str(c), 5_000_000 * c, 5_000_000 * c + 600) for c in range(1, 21)] + \
          [("cyp", "22", 42_100_000 + 30_000 * k, 42_100_000 + 30_000 * k + 5_000) for k in range(8)]


def run(data, switch, reps):
    ts, st = [], None
    with engine.test_switches(front=switch):
        for _ in range(reps):
            ex = extract.Extractor(REGIONS, FAMILIES, "hisat2", True, False, True)
            t0 = time.perf_counter()
            ex.feed(data, last=True)               # ends in a stream synchronise and the copy of the text back
            ts.append((time.perf_counter() - t0) * 1e3)
            st = ex.stats()
            n_out = sum(len(ex.take(f, m)) for f in range(len(FAMILIES)) for m in range(2))
            ex.close()
    return ts, st, n_out


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 2_600_000
    capi.set_device(0)
    t0 = time.perf_counter()
    data = extract.synth_stream(n_pairs, REGIONS, seed=3, hit_fraction=0.015, read_len=100)
    n_rec = data.count(b"\n")
    print("generated %d records, %.1f MB in %.0f s" % (n_rec, len(data) / 1e6, time.perf_counter() - t0), flush=True)
    ts, st, n_out = run(data, "device", 6)
    assert st["route"] == 2, st
    dev_ms = statistics.median(ts[1:])
    hs, sth, n_out_h = run(data, "host", 3)
    assert n_out_h == n_out and sth["written"] == st["written"]
    host_ms = statistics.median(hs[1:])
    sent = len(data) + 8 * n_rec
    model = len(data) + (8 + 64) * n_rec                    # the record pass: the text once, 8 B line table in, 64 B fields out
    print("records %d, groups %d, written %s, output %.1f MB" % (n_rec, st["groups"], st["written"], n_out / 1e6))
    print("device route %.1f ms (median of 5; all %s) = %.2f M records/s | host route %.1f ms = %.2f M records/s | x%.1f"
          % (dev_ms, ["%.0f" % t for t in ts], n_rec / dev_ms / 1e3, host_ms, n_rec / host_ms / 1e3, host_ms / dev_ms))
    print("bytes sent per record %.1f | record-pass byte model %.1f B per record: %.3f ms at HBM peak = %.2f %% of the device route's time"
          % (sent / n_rec, model / n_rec, model / HBM_PEAK * 1e3, 100 * model / HBM_PEAK * 1e3 / dev_ms))
    # the gate: device against host on chunks of a few hundred to a few thousand records
    lines = data.split(b"\n")
    for n in (250, 500, 1000, 2000, 4000, 8000, 16000):
        part = b"\n".join(lines[:n]) + b"\n"
        d, _, _ = run(part, "device", 8)
        h, _, _ = run(part, "host", 8)
        print("  %6d records: device %.3f ms, host %.3f ms" % (n, statistics.median(d[2:]), statistics.median(h[2:])))
    if "--reference-loop" in sys.argv:
        import extract_ref
        part = b"\n".join(lines[:n_rec // 50]) + b"\n"
        t0 = time.perf_counter()
        extract_ref.extract(part.decode(), REGIONS, FAMILIES, "hisat2", True, False, True)
        dt = time.perf_counter() - t0
        print("the spec's Python loop: %d records in %.2f s = %.3f M records/s" % (n_rec // 50, dt, n_rec / 50 / dt / 1e6))


if __name__ == "__main__":
    main()
