#!/usr/bin/env python3
"""Files -> results for a panel of 64 samples x 6 HLA loci at the panel64 workload's sizes (bench.py PANEL, --panel-pairs), three ways:

  (a) six ManyBatch.from_files over the 64 MULTI-locus files (one BAM per sample, every locus' records in it) -- what
      run_panel(many=True) did with such input before engine.AlignmentSet: every file read, sent, inflated and walked once per locus;
  (b) six ManyBatch.from_files over 384 SINGLE-locus files -- the input the panel64 end-to-end figure is measured on;
  (c) one engine.AlignmentSet over the 64 multi-locus files, one route, six ManyBatch.from_set side by side.

All three end in the same typing.type_many_loci call (light results), so the difference is the front end.  The three ways alternate
in one process: one warm-up round, then the median of --reps rounds each; bytes sent to the device are reported per way.
HGX_PARSE_PROFILE=1 prints the per-phase laps of every call on stderr.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import bamio, capi, engine, locus as hl, synth  # noqa: E402

htyping = sys.modules["hisatgenotype_amd.typing"]
PANEL = [("A", 7000, 3569, 2500), ("B", 8000, 4081, 2800), ("C", 7000, 4305, 2600), ("DRB1", 3000, 3800, 1800),
         ("DQA1", 500, 3300, 600), ("DQB1", 2000, 3600, 1400)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5000, help="read pairs per (sample, locus)")
    ap.add_argument("--err", type=float, default=0.002)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loci", type=int, default=len(PANEL))
    args = ap.parse_args()
    capi.set_device(0)
    loci = [synth.make_hla_like_locus(gene=g, n_alleles=a, length=ln, n_vars=v, seed=500 + i, var_id_base=10000 * i)
            for i, (g, a, ln, v) in enumerate(PANEL[:args.loci])]
    pls = [hl.PackedLocus.from_synth(loc) for loc in loci]
    for pl in pls:
        pl.index()
    refs = [(loc.ref_allele, len(loc.backbone)) for loc in loci]
    regions = [loc.ref_allele for loc in loci]
    d = tempfile.mkdtemp(prefix="hgx_panel_set_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        multi, single, truth = [], [[] for _ in loci], {}
        for s in range(args.samples):
            sams = []
            for k, loc in enumerate(loci):
                sample = synth.pick_sample(loc, 1000 * s + k)
                truth[(s, k)] = sorted(sample)
                sam = synth.simulate_sam_fast(loc, sample, args.pairs, err_rate=args.err, seed=100 * s + k)
                sams.append(sam)
                single[k].append(os.path.join(d, "s%02d_%s.bam" % (s, loc.gene)))
                bamio.write_bam_native(single[k][-1], sam.encode(), [refs[k]], sort_by_coordinate=True)
            multi.append(os.path.join(d, "s%02d.bam" % s))
            bamio.write_bam_native(multi[-1], "".join(sams).encode(), refs, sort_by_coordinate=True)
        sent = {}

        def finish(manies):
            try:
                return htyping.type_many_loci(pls, manies, light=True)
            finally:
                for m in manies:
                    m.close()

        def per_locus(name, paths_of):
            t0 = time.perf_counter()
            manies, n = [], 0
            for k, pl in enumerate(pls):
                manies.append(engine.ManyBatch.from_files(pl, paths_of(k), regions=[regions[k]] * args.samples))
                assert engine.front_last() == (2, 0), engine.front_last()
                n += engine.front_last_bytes()
            t1 = time.perf_counter()
            sent[name] = n
            return finish(manies), t1 - t0, time.perf_counter() - t0

        def way_a():
            return per_locus("a", lambda k: multi)

        def way_b():
            return per_locus("b", lambda k: single[k])

        def way_c():
            t0 = time.perf_counter()
            with engine.AlignmentSet(multi) as aset:
                assert aset.resident
                aset.route(regions)
                manies = htyping._many_from_set_side_by_side(pls, aset, list(range(len(pls))))
                t1 = time.perf_counter()
                sent["c"] = aset.bytes_to_device
                rows = finish(manies)
            return rows, t1 - t0, time.perf_counter() - t0

        ways = (("a", way_a), ("b", way_b), ("c", way_c))
        rows = {name: fn()[0] for name, fn in ways}                                  # warm-up round (and the results to compare)
        assert rows["a"] == rows["b"] == rows["c"], "the three ways disagree"
        correct = sum(sorted(r[1]) == truth[(s, k)] for k, row in enumerate(rows["c"]) for s, r in enumerate(row))
        front, total = {n: [] for n, _ in ways}, {n: [] for n, _ in ways}
        for _ in range(args.reps):
            for name, fn in ways:
                _, tf, tt = fn()
                front[name].append(tf * 1e3)
                total[name].append(tt * 1e3)
        out = {"samples": args.samples, "loci": len(loci), "pairs_per_task": args.pairs, "reps": args.reps,
               "tasks_correct": "%d/%d" % (correct, args.samples * len(loci)),
               "multi_locus_file_MB": round(sum(os.path.getsize(p) for p in multi) / 1e6, 1),
               "single_locus_file_MB": round(sum(os.path.getsize(p) for ps in single for p in ps) / 1e6, 1)}
        for name, label in (("a", "a_from_files_multi_locus"), ("b", "b_from_files_single_locus"), ("c", "c_alignment_set")):
            out[label] = {"files_to_results_ms_median": round(statistics.median(total[name]), 2),
                          "files_to_batches_ms_median": round(statistics.median(front[name]), 2),
                          "files_to_results_ms_all": [round(x, 2) for x in total[name]],
                          "MB_to_device": round(sent[name] / 1e6, 1)}
        print(json.dumps(out))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
