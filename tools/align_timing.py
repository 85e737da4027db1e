"""Time the "hgx" aligner's device route against its host route: reads/s of AlignIndex.align on simulated
100-base pairs of a synth HLA-like locus, upload and copy back included, at a few read counts round the route gate.

    python tools/align_timing.py [--err 0.5] [--reps 5] [--sizes 250,500,1000,2000,4000,16000,64000]

Prints one line per size (best of --reps after one warm-up call) and the break-even size if the sweep brackets it.  A tool,
not a test.
"""
import argparse
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hisatgenotype_amd import align, capi, simulate, synth          # noqa: E402


def reads_of(err_percent, n_pairs):
    loc = synth.make_hla_like_locus(n_alleles=200, n_vars=1500, seed=5)
    d = loc.reference_dicts()
    alleles = loc.allele_names[1:7]
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        random.seed(1)
        simulate.simulate_reads(d["Genes"], "t", [alleles], d["Vars"], d["Links"], simulate_interval=7,
                                perbase_errorrate=err_percent, out_dir=tmp)
        mates = [simulate._read_fasta(os.path.join(tmp, "t_input_%d.fa" % m)) for m in (1, 2)]
    finally:
        os.chdir(cwd)
    texts = []
    for recs in mates:
        recs = [("r%d" % k, recs[k % len(recs)][1]) for k in range(n_pairs)]
        texts.append("".join(">%s\n%s\n" % r for r in recs).encode())
    return d, texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--err", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="250,500,1000,2000,4000,16000,64000")
    args = ap.parse_args()
    capi.set_device(0)
    rows = []
    for n in [int(x) for x in args.sizes.split(",")]:
        d, texts = reads_of(args.err, n // 2)
        ix = align.AlignIndex(d["Genes"], d["Vars"], d["Var_list"], d["refGenes"])
        out, best = {}, {}
        for route in ("device", "host"):
            out[route] = ix.align(texts, route=route)
            last = align.align_last()
            assert last["route"] == (2 if route == "device" else 0), last
            ts = []
            for _ in range(args.reps):
                t = time.perf_counter()
                ix.align(texts, route=route)
                ts.append(time.perf_counter() - t)
            best[route] = min(ts)
        assert out["device"] == out["host"]
        rows.append((n, best["device"], best["host"]))
        print("%7d reads  device %9.3f ms %10.0f reads/s   host %9.3f ms %10.0f reads/s   aligned %d" % (
            n, best["device"] * 1e3, n / best["device"], best["host"] * 1e3, n / best["host"], last["aligned"]), flush=True)
        ix.close()
    for (n0, d0, h0), (n1, d1, h1) in zip(rows, rows[1:]):
        if d0 > h0 and d1 <= h1:
            print("break-even between %d and %d reads" % (n0, n1))
    if rows and rows[0][1] <= rows[0][2]:
        print("the device route is already ahead at %d reads" % rows[0][0])


if __name__ == "__main__":
    main()
