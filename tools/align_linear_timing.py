"""Time the "hgx" aligner on a linear index: its device route against its host route, in reads/s and candidates/s
of LinearAlignIndex.align, upload and copy back included.

    python tools/align_linear_timing.py [--alleles 100,1000,7000] [--length 3500] [--sizes 8192,64000] [--k 10] [--max-edits 2]
                                        [--err 0.5] [--reps 5] [--host-reads 4096] [--no-host]

A family is one random sequence of --length bases and --alleles copies of it with ten substitutions each (near-identical windows in
every seed bucket, as at an HLA locus).  Reads are 2 x 100: pairs cut 250 bases apart from random alleles, --err percent errors per
base, mate 2 reverse-complemented.  Prints one line per family, size and route: the median and range of --reps calls after one
warm-up call -- on BOTH routes -- reads/s, candidates/s (seed-table entries looked at per second), the route taken and its decline
code.  The host route is single-threaded and pays for every candidate: where the input is larger it is timed on the first
--host-reads reads only (the line says over how many), and reads/s are what compare.  A tool, not a test.
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hisatgenotype_amd import align, capi          # noqa: E402

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def family(n, length, seed=1):
    rng = random.Random(seed)
    base = [rng.choice("ACGT") for _ in range(length)]
    Genes = {"F": {"F*BACKBONE": "".join(base)}}
    for a in range(n):
        s = list(base)
        for p in rng.sample(range(length), 10):
            s[p] = rng.choice([b for b in "ACGT" if b != s[p]])
        Genes["F"]["F*%05d" % a] = "".join(s)
    return Genes, {"F": "F*BACKBONE"}


def reads_of(Genes, n_reads, err_percent, seed=2):
    rng = random.Random(seed)
    seqs = [s for n, s in Genes["F"].items() if "BACKBONE" not in n]
    m1, m2 = [], []

    def noisy(s):
        return "".join(rng.choice([b for b in "ACGT" if b != c]) if rng.random() * 100 < err_percent else c for c in s)
    for k in range(n_reads // 2):
        s = seqs[rng.randrange(len(seqs))]
        p = rng.randrange(0, len(s) - 250)
        m1.append(">r%d\n%s\n" % (k, noisy(s[p:p + 100])))
        m2.append(">r%d\n%s\n" % (k, noisy("".join(_COMP[c] for c in reversed(s[p + 150:p + 250])))))
    return ["".join(m1).encode(), "".join(m2).encode()]


def head_of(texts, n_reads):
    return [b"\n".join(t.split(b"\n")[:n_reads]) + b"\n" for t in texts]       # n_reads / 2 records of two lines per input


def timed(ix, texts, route, reps, warm, **kw):
    times = []
    for r in range(reps + (1 if warm else 0)):
        t0 = time.perf_counter()
        out = ix.align(texts, route=route, **kw)
        dt = time.perf_counter() - t0
        if r or not warm:
            times.append(dt)
    return times, out, align.align_linear_last()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", default="100,1000,7000")
    ap.add_argument("--length", type=int, default=3500)
    ap.add_argument("--sizes", default="8192,64000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-edits", type=int, default=2)
    ap.add_argument("--err", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    capi.set_device(0)
    kw = dict(max_edits=a.max_edits, k=a.k)
    for n_alleles in [int(x) for x in a.alleles.split(",")]:
        t0 = time.perf_counter()
        Genes, refGenes = family(n_alleles, a.length)
        ix = align.LinearAlignIndex(Genes, refGenes)
        print("family of %d alleles x %d bases: index built in %.2f s" % (n_alleles, a.length, time.perf_counter() - t0), flush=True)
        for n_reads in [int(x) for x in a.sizes.split(",")]:
            texts = reads_of(Genes, n_reads, a.err)
            dev, out_d, last = timed(ix, texts, "device", a.reps, True, **kw)
            med = statistics.median(dev)
            print("  %6d reads  device  median %8.2f ms (%.2f .. %.2f)  %10.0f reads/s  %.3g candidates/s  route %d decline %d  %d records"
                  % (n_reads, med * 1e3, min(dev) * 1e3, max(dev) * 1e3, n_reads / med, last["candidates"] / med, last["route"], last["decline"],
                     last["records"]), flush=True)
            if a.no_host:
                continue
            n_host = min(n_reads, a.host_reads)
            part = texts if n_host == n_reads else head_of(texts, n_host)
            host, out_h, last = timed(ix, part, "host", a.reps, True, **kw)
            med = statistics.median(host)
            same = out_h == out_d if n_host == n_reads else out_d.startswith(out_h[:len(out_h) // 2])
            print("  %6d reads  host    median %8.2f ms (%.2f .. %.2f)  %10.0f reads/s  %.3g candidates/s  over %d reads, %d calls  bytes %s"
                  % (n_reads, med * 1e3, min(host) * 1e3, max(host) * 1e3, n_host / med, last["candidates"] / med, n_host, len(host),
                     "equal" if same else "DIFFER"), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
