"""Genome-wide alignment in, report out: the chain with files in between against the resident chain.

The stream is the one of tools/extract_timing.py (seeded, HISAT2-like, most pairs outside every region) with the reads of the golden
self-test call "pairs_two_genes" written into the hla family's regions, so that the typing stage has loci to type; as SAM text and
as BAM.  Per form, after one warm-up run, the median of `--reps` runs of
  files     extract_reads -> <sample>-hla-extracted-{1,2}.fq.gz -> typing() with typing_options.align_resident
  resident  extract_reads_resident -> typing_options.reads -> typing()
with wall time and CPU-seconds (time.process_time: every thread of the process) per sample, and the split of the resident chain:
emit -> take_reads (extract_reads_resident: stream in, the family's Reads out, the table included), the table alone (the same text
through Reads.from_text, upload included: an upper bound), align (AlignIndex.align_resident over the Reads) and type (typing(), which
aligns again: its wall time holds the align stage).  There is no target ratio: the tool reports what comes out.

    python tools/stream_to_report_timing.py [--pairs N] [--reps K] [--bam]      (default 2 600 000 pairs = 5.4 M records)"""
import contextlib
import importlib
import io
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hisatgenotype_amd  # noqa: E402,F401
from hisatgenotype_amd import align, bamio, capi, engine, extract  # noqa: E402

CHROMS = [str(i + 1) for i in range(22)] + ["X"]


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def make_stream(call, n_pairs, seed=3):
    """SAM text: n_pairs synthetic pairs outside every region (none on chromosomes 6 and 7), then the call's read pairs inside the
    two hla regions there."""
    outside = extract.synth_stream(n_pairs, [], seed=seed, hit_fraction=0.0, read_len=100, chroms=[c for c in CHROMS if c not in "67"])
    m1, m2 = call["reads"]
    inside = []
    for k in range(len(m1)):
        chrom, pos = ("6", 1000100 + 3 * k) if k % 2 == 0 else ("7", 5000100 + 3 * k)
        for (_, s, _), flag, p in ((m1[k], 0x43, pos), (m2[k], 0x83, pos + 300)):
            inside.append("zfrag%06d\t%d\t%s\t%d\t60\t%dM\t=\t%d\t300\t%s\t%s\tNH:i:1\n" % (k, flag, chrom, p, len(s), pos, s, "F" * len(s)))
    return outside + "".join(inside).encode(), len(m1)


def timed(fn):
    w0, c0 = time.perf_counter(), time.process_time()
    out = fn()
    return out, time.perf_counter() - w0, time.process_time() - c0


def main():
    import align_cases
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")
    capi.set_device(0)
    n_pairs, reps = arg("--pairs", 2_600_000), arg("--reps", 3)
    work = tempfile.mkdtemp()
    try:
        call = align_cases.selftest_calls("pairs_two_genes", os.path.join(work, "loop"))[-1]
        ix_dir = os.path.join(work, "genome")
        os.makedirs(ix_dir)
        with open(os.path.join(ix_dir, "genotype_genome.locus"), "w") as f:
            f.write("HLA\tA*BACKBONE\t6\t1000000\t2000000\t3000\t+\nHLA\tB*BACKBONE\t7\t5000000\t6000000\t3000\t+\n")
        t0 = time.perf_counter()
        sam, n_in = make_stream(call, n_pairs)
        stream = os.path.join(work, "genome.sam")
        with open(stream, "wb") as f:
            f.write(sam)
        if "--bam" in sys.argv:
            stream = os.path.join(work, "genome.bam")
            bamio.write_bam_native(stream, sam.decode(), [(c, 200000000) for c in CHROMS])
        print("stream: %d records, %.1f MB as %s, %d pairs inside the family (made in %.0f s)"
              % (sam.count(b"\n"), os.path.getsize(stream) / 1e6, "BAM" if stream.endswith(".bam") else "SAM", n_in, time.perf_counter() - t0), flush=True)
        del sam
        typing_mod.typing_options.align_resident = True

        def args_for(out_dir):
            a = list(call["args"])
            a[0], a[2], a[14], a[19], a[24], a[26], a[27], a[34] = False, ["A", "B"], [["hgx", "graph"]], False, True, "", [], out_dir
            a[25] = [os.path.join(out_dir, "sample-hla-extracted-%d.fq.gz" % m) for m in (1, 2)]
            return a

        def files(k):
            out = os.path.join(work, "files%d" % k)
            os.makedirs(out)
            _, w1, c1 = timed(lambda: extract.extract_reads("genotype_genome", ix_dir, ["hla"], "", out, "fq.gz", ["sample", "sample"], True, True,
                                                            False, 8, 1, 1, [0, 1], "hisat2", 0, False, alignment_fname=stream))
            _, w2, c2 = timed(lambda: typing_mod.typing(*args_for(out)))
            return dict(wall=w1 + w2, cpu=c1 + c2, extract=w1, type=w2)

        def resident(k):
            out = os.path.join(work, "resident%d" % k)
            os.makedirs(out)
            reads, w1, c1 = timed(lambda: extract.extract_reads_resident("genotype_genome", ix_dir, ["hla"], stream, True, True, False, "hisat2"))
            typing_mod.typing_options.reads = reads["hla"]
            try:
                _, w2, c2 = timed(lambda: typing_mod.typing(*args_for(out)))
                # the stages of their own, outside the chain's time
                texts = [reads["hla"].input_text(i) for i in range(2)]
                r2, wt, _ = timed(lambda: engine.Reads.from_text(texts))
                r2.close()
                ix = align.cached_index(call["Genes"], call["Vars"], call["Var_list"], call["refGenes"])
                al, wa, _ = timed(lambda: ix.align_resident(reads["hla"], max_edits=call["num_editdist"]))
                al.close()
            finally:
                typing_mod.typing_options.reads = None
                reads["hla"].close()
            return dict(wall=w1 + w2, cpu=c1 + c2, extract=w1, type=w2, table=wt, align=wa)

        with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
            for name, fn in (("files", files), ("resident", resident)):
                runs = [fn(k) for k in range(reps + 1)][1:]
                med = {key: statistics.median(r[key] for r in runs) for key in runs[0]}
                print("%-8s wall %.3f s  cpu %.3f s per sample | " % (name, med["wall"], med["cpu"]) +
                      "  ".join("%s %.1f ms" % (key, med[key] * 1e3) for key in med if key not in ("wall", "cpu")), flush=True)
    finally:
        typing_mod.typing_options.align_resident = False
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
