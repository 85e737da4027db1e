"""Time reads -> per-locus DeviceBatches, and reads -> typed loci, through the alignment FILE (the default: AlignIndex.align, the
Python split and the coordinate-sorted BAM of simulate._store_as_the_reference_does, engine.Alignment(path), parse_dev per locus)
and through the RESIDENT hand-off (AlignIndex.align_resident, parse_dev per locus; DESIGN.md 5.13 "Resident hand-off").

    python tools/align_resident_timing.py [--sizes 4000,16000,64000] [--loci 1,6] [--reps 5] [--err 0.5]

Reads: 100-base pairs of synth.simulate_pairs over 1 or 6 synth HLA-like loci (200 alleles, 1 500 variants each), 2 000 pairs per
locus cycled to the read count, FASTA texts in memory.  Per size and locus count, after one warm-up of each route, the two routes
ALTERNATE --reps times in this process (run the tool a second time for the second process); printed per leg: median and range.
  file route      align (text copied back) | Python decode + split + BAM write | open (read, upload, inflate) | parse_dev, all loci
  resident route  align_resident (text stays in HBM) | parse_dev, all loci
  typed           the same with typing.type_locus(alignment=...) per locus instead of parse_dev alone
What the resident route adds on the device (record keys, radix sort, scan, gather) is printed as the difference of two medians:
align(order="coordinate") - align() (both copy the text back) and align_resident - align().  The loci are parsed one after the
other on one stream in both routes.  A tool, not a test."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import importlib                                                      # noqa: E402

from hisatgenotype_amd import align, capi, engine, simulate, synth     # noqa: E402
from hisatgenotype_amd.locus import PackedLocus                        # noqa: E402

typing_mod = importlib.import_module("hisatgenotype_amd.typing")
GENES = ["A", "B", "C", "DRB1", "DQA1", "DQB1"]


def panel(n_loci, n_reads, err_percent):
    """(dicts of all loci, [PackedLocus], [mate-1 FASTA, mate-2 FASTA])"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = lambda s: "".join(comp.get(b, b) for b in reversed(s))           # noqa: E731
    d = dict(Genes={}, Vars={}, Var_list={}, refGenes={})
    pls, pools = [], []
    for k in range(n_loci):
        loc = synth.make_hla_like_locus(gene=GENES[k], n_alleles=200, n_vars=1500, seed=5 + k)
        rd = loc.reference_dicts()
        for key in d:
            d[key].update(rd[key])
        pls.append(PackedLocus.from_synth(loc))
        als = synth.simulate_pairs(loc, loc.allele_names[1:3], 2000, read_len=100, frag_len=(300, 400), err_rate=err_percent / 100.0, seed=13 + k)
        mates = [[], []]
        for a in als:
            mates[0 if a.flag & 0x40 else 1].append((rc(a.seq) if a.flag & 0x10 else a.seq).upper())
        pools.append(mates)
    n_pairs = n_reads // 2
    texts = []
    for m in (0, 1):
        texts.append("".join(">r%d\n%s\n" % (k, pools[k % n_loci][m][(k // n_loci) % len(pools[k % n_loci][m])]) for k in range(n_pairs)).encode())
    return d, pls, texts


def lap(legs, name, t0):
    t1 = time.perf_counter()
    legs.setdefault(name, []).append((t1 - t0) * 1e3)
    return t1


def file_route(ix, d, pls, texts, path, legs, typed):
    t_all = t = time.perf_counter()
    text = ix.align(texts, route="device")
    t = lap(legs, "file: align, text back", t)
    simulate._store_as_the_reference_does(path, text.decode())
    t = lap(legs, "file: split + BAM write", t)
    al = engine.Alignment(path)
    t = lap(legs, "file: open", t)
    out = per_locus(al, d, pls, typed)
    t = lap(legs, "file: loci", t)
    al.close()
    os.remove(path)
    lap(legs, "file: TOTAL", t_all)
    return out


def resident_route(ix, d, pls, texts, legs, typed):
    t_all = t = time.perf_counter()
    al = ix.align_resident(texts, route="device")
    t = lap(legs, "resident: align_resident", t)
    out = per_locus(al, d, pls, typed)
    t = lap(legs, "resident: loci", t)
    al.close()
    lap(legs, "resident: TOTAL", t_all)
    return out


def per_locus(al, d, pls, typed):
    out = []
    for pl in pls:
        region = [d["refGenes"][pl.gene]]
        if typed:
            res = typing_mod.type_locus(pl, None, regions=region, alignment=al)
            out.append((res.num_reads, res.num_pairs, [(n, float(p)) for n, p in res.gene_prob]))
        else:
            db = al.parse_dev(pl, region)
            out.append((db.n_reads, db.n_pairs, db.n_pieces, db.n_refs))
            db.close()
    capi.sync(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000,16000,64000")
    ap.add_argument("--loci", default="1,6")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--err", type=float, default=0.5)
    args = ap.parse_args()
    capi.set_device(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "timing.bam")
    for n_loci in [int(x) for x in args.loci.split(",")]:
        for n in [int(x) for x in args.sizes.split(",")]:
            d, pls, texts = panel(n_loci, n, args.err)
            ix = align.AlignIndex(d["Genes"], d["Vars"], d["Var_list"], d["refGenes"])
            for typed in (False, True):
                legs = {}
                a = file_route(ix, d, pls, texts, path, {}, typed)                 # warm-up of each route
                b = resident_route(ix, d, pls, texts, {}, typed)
                assert a == b, "the two routes disagree"
                for _ in range(args.reps):
                    assert file_route(ix, d, pls, texts, path, legs, typed) == a
                    assert resident_route(ix, d, pls, texts, legs, typed) == a
                for _ in range(args.reps):                                        # the device's share: the same call in its three forms
                    for name, fn in (("align()", lambda: ix.align(texts, route="device")),
                                     ("align(order=coordinate)", lambda: ix.align(texts, route="device", order="coordinate")),
                                     ("align_resident()", lambda: ix.align_resident(texts, route="device").close())):
                        t = time.perf_counter()
                        fn()
                        lap(legs, name, t)
                last = align.align_last()
                print("---- %d loci, %d reads (aligned %d, route %d), %s: per-locus reads %s" % (
                    n_loci, n, last["aligned"], last["route"], "typed (type_locus)" if typed else "DeviceBatches (parse_dev)", [r[0] for r in a]))
                for name, ts in legs.items():
                    print("    %-34s median %9.3f ms   range %9.3f .. %9.3f ms" % (name, statistics.median(ts), min(ts), max(ts)))
                med = {k: statistics.median(v) for k, v in legs.items()}
                print("    resident adds on the device: sorted text copied back %+.3f ms, kept in HBM %+.3f ms against align()" % (
                    med["align(order=coordinate)"] - med["align()"], med["align_resident()"] - med["align()"]))
                print("    file route spends on the host and the file: split + BAM write %.3f ms, open %.3f ms" % (
                    med["file: split + BAM write"], med["file: open"]))
                print("    TOTAL file %.3f ms, resident %.3f ms: resident / file = %.3f" % (
                    med["file: TOTAL"], med["resident: TOTAL"], med["resident: TOTAL"] / med["file: TOTAL"]), flush=True)
            ix.close()
            for pl in pls:
                pl.close()
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
