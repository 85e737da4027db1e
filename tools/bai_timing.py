"""A locus region out of a genome-sized BAM: hgx_type_file with and without the file's index.

Makes ONE coordinate-sorted BAM under 4 GB of inflated stream -- the reads of a synthetic HLA-like locus on chromosome "6" (default
1 M reads) plus decoy records on other chromosomes up to --stream-gb (default 3) -- indexes it, and times hgx_type_file with the locus
region, median of five after a warm-up:
    (b) this tree with the test switch bai=off   (the path every call took before the index)
    (c) this tree with the index
and, with --sweep, the same for smaller files of the same make-up (decoys only up to each size) to find where (c) stops beating (b):
the break-even HGX_BAI_MIN_BYTES should sit at.
    (a) is this tool run with --no-index on a checkout of the parent commit: only calls the parent has (no switch, no report, the BAM
        made the same way and left without an index).  (a) against (b) shows that the old path did not move.
Prints one JSON line per file: sizes, the times with their spread (min / median / max of the five), bytes read and sent.

Usage: tools/bai_timing.py [--no-index] [--stream-gb 3] [--locus-pairs 500000] [--sweep 8,32,128,512] [--dir DIR] [--keep]"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hisatgenotype_amd as hgx  # noqa: E402
from hisatgenotype_amd import bamio, capi, engine, locus as hl, synth  # noqa: E402

DECOY_REFS = [("1", 240000000), ("2", 240000000), ("3", 190000000)]
REFS = DECOY_REFS[:2] + [("6", 170000000)] + DECOY_REFS[2:]
LEFT = 29900000                                  # where the locus lies on chromosome 6 (0-based)


def decoy_text(n, seed):
    """n decoy records spread over the decoy chromosomes, 150 random bases each, as SAM text (any order: the writer sorts)."""
    rng = random.Random(seed)
    seqs = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(997)]
    quals = ["".join(chr(33 + rng.randrange(40)) for _ in range(150)) for _ in range(991)]
    out = []
    for k in range(n):
        name, ln = DECOY_REFS[k % len(DECOY_REFS)]
        out.append("d%09d\t0\t%s\t%d\t60\t150M\t*\t0\t0\t%s\t%s\tNM:i:0\n" % (k, name, 1 + rng.randrange(ln - 200), seqs[k % 997], quals[k % 991]))
    return "".join(out)


def make_bam(path, locus_rows, stream_bytes, seed):
    """The locus reads + decoys up to about `stream_bytes` of inflated BAM stream (a decoy record takes ~ 290 bytes of it)."""
    locus_bytes = sum(len(r) for r in locus_rows)
    n_decoys = max(0, int((stream_bytes - locus_bytes) / 290))
    text = "".join(locus_rows) + decoy_text(n_decoys, seed)
    bamio.write_bam_native(path, text.encode(), REFS, sort_by_coordinate=True)
    return n_decoys


def timed(fn, reps=5):
    fn()                                         # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 2), "median_ms": round(statistics.median(ts), 2), "max_ms": round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-index", action="store_true", help="only calls the parent commit has: no index is written, no switch set, no report read")
    ap.add_argument("--stream-gb", type=float, default=3.0)
    ap.add_argument("--locus-pairs", type=int, default=500000)
    ap.add_argument("--sweep", default="", help="comma-separated sizes of inflated stream in MB for the break-even")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true")
    a = ap.parse_args()
    capi.set_device(0)
    loc = synth.make_hla_like_locus(gene="A", n_alleles=600, length=3569, n_vars=1300, seed=300)
    pl = hl.PackedLocus.from_synth(loc)
    sam = synth.simulate_sam_fast(loc, synth.pick_sample(loc, 40), a.locus_pairs, err_rate=0.003, seed=50)
    rows = []
    for l in sam.split("\n"):
        if l:
            f = l.split("\t")
            f[2], f[3], f[7] = "6", str(int(f[3]) + LEFT), str(int(f[7]) + LEFT)
            rows.append("\t".join(f) + "\n")
    regions = ["6:%d-%d" % (LEFT + 1, LEFT + len(loc.backbone)), loc.ref_allele]
    sizes = [int(a.stream_gb * (1 << 30))] + [int(float(x) * (1 << 20)) for x in a.sweep.split(",") if x]
    tmp = a.dir or tempfile.mkdtemp(prefix="bai_timing_")
    for k, size in enumerate(sizes):
        path = os.path.join(tmp, "genome_%d.bam" % k)
        n_rows = rows if k == 0 else rows[:max(2000, int(len(rows) * min(1.0, size / sizes[0])))]      # (smaller files: the same make-up)
        n_decoys = make_bam(path, n_rows, size, 7 + k)
        out = {"stream_target_bytes": size, "file_bytes": os.path.getsize(path), "locus_records": len(n_rows), "decoys": n_decoys}

        def call():
            return hgx.type_file(pl, path, regions, base_locus=LEFT)

        if a.no_index:
            out["a_no_index"] = timed(call)
            out["bytes_to_device"] = engine.front_last_bytes()
        else:
            t0 = time.perf_counter()
            bamio.index_bam(path)
            out["index_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out["index_bytes"] = os.path.getsize(path + ".bai")
            with engine.test_switches(bai="off"):
                want = call()
                out["b_index_off"] = timed(call)
                out["b_bytes_to_device"] = engine.front_last_bytes()
            with engine.test_switches(bai="force"):
                got = call()
                out["c_index"] = timed(call)
                out["c_bytes_to_device"] = engine.front_last_bytes()
                out["c_report"] = engine.bam_index_last()
            assert got.gene_prob == want.gene_prob and got.em == want.em and got.num_reads == want.num_reads
            out["c_beats_b"] = out["c_index"]["median_ms"] < out["b_index_off"]["median_ms"]
        print(json.dumps(out), flush=True)
        if not a.keep:
            for p in (path, path + ".bai"):
                if os.path.exists(p):
                    os.remove(p)


if __name__ == "__main__":
    main()
