"""Time the "hgx" aligner's device route against its host route: reads/s of AlignIndex.align, upload and copy
back included, at a few read counts.

    python tools/align_timing.py [--workload synth|tandem|paralog|overhang|novel|mixed] [--search ways|states|states_all] [--pair]
                                 [--clip N] [--gap N] [--rescue G,C]
                                 [--err 0.5] [--reps 5] [--sizes 250,500,1000,2000,4000,16000,64000] [--tandem-indels 12] [--no-host]

--workload synth   simulated 100-base pairs of a synth HLA-like locus, at read counts round the route gate
--workload tandem  150-base single reads across a GATA x 40 repeat with --tandem-indels known unit deletions and as many known
                   unit insertions (two alleles: the backbone's, and one with three units fewer).  Reads inside the plain repeat
                   pass the kernels' anchor slots: with --search ways the call goes to the host route (default --sizes 64).
--workload paralog 100-base pairs of two loci that share a 300-base stretch (one base of the copy differs): mate 1 inside the
                   stretch, cut from either locus, mate 2 unique and 300 to 500 bases on at home (default --sizes 16000,64000)
--workload overhang 100-base single reads tiled every 7 bases from 50 bases in front of a synth locus' backbone to 50 bases behind it
                   (random bases outside), every fifth with a ten-base random tail, --err errors, cycled to the read count
                   (default --sizes 16000,64000): the reads the clip tier exists for
--workload novel   100-base pairs of synth.simulate_pairs over the synth locus, a tenth of the reads with a novel one-base deletion
                   (novel_del_frac) and a tenth with a novel one- or two-base insertion (novel_ins_frac), --err errors, cycled to
                   the read count (default --sizes 16000,64000): the reads the gap tier exists for
--workload mixed   single reads over the synth locus: half of them the overhang workload's tiled reads, half the novel workload's
                   pairs (both mates), --err errors (default --sizes 16000,64000): the reads both tiers in one call exist for
--rescue G,C       time both routes with gap=G alone, with clip=C alone and with rescue=(G, C) (hgx_align_more.rescue_clip) beside
                   the default, and print, per route: reads aligned under each of the three, both counter triples of the rescue
                   call, the reads the cost rule kept out of its gap pass (clip searched - gap searched), the cost per 8 192-read
                   chunk of each against the default, and the ratio of the rescue call's cost to the sum of the two tiers' costs
--gap N            time both routes with gap=N (hgx_align_more.gap) beside gap=0 and print the counters of hgx_align_last_gap and the
                   cost per 8 192-read chunk; the two gap texts are compared with each other, not with the gap=0 texts
--clip N           time both routes with clip=N (hgx_align_opts.clip) beside clip=0 and print the counters of hgx_align_last_clip and
                   the cost per 8 192-read chunk; the two clip texts are compared with each other, not with the clip=0 texts
--pair             time the device route with pair="aware" beside pair="independent" (hgx_align_opts.pair) and print the pair
                   counters; the texts differ by design, so they are not compared with each other
--search           the search form of the device-route call (hgx_align_opts.search).  The host route is timed with "ways" and,
                   when --search is not "ways", with "states" as well.

Prints one line per size and configuration: the median and the range of --reps calls after one warm-up call, the route the call
took and its decline code, what the states form took.  With --workload synth it also prints the break-even size of device
against host "ways" if the sweep brackets it.  A tool, not a test.
"""
import argparse
import os
import random
import statistics
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


def tandem_reads(n_indels, n_reads, units=40, flank=300, read_len=150, stride=11):
    """(reference dicts, [one FASTA text]): a locus flank + GATA x units + flank with n_indels known 4-base deletions and n_indels
    known GATA insertions inside the repeat, 8 bases apart; reads cut every `stride` bases from the backbone and from an allele
    with three units fewer, one substitution in every third read, cycled to n_reads."""
    rng = random.Random(7)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))          # noqa: E731
    bb = seq(flank) + "GATA" * units + seq(flank)
    Vars, Var_list = {}, []
    for j in range(min(n_indels, units // 2)):
        for t, p, data in (("deletion", flank + 4 + 8 * j, "4"), ("insertion", flank + 8 + 8 * j, "GATA")):
            vid = "hv%d" % len(Var_list)
            Vars[vid] = [t, p, data]
            Var_list.append([p, vid])
    short = bb[:flank + 4] + bb[flank + 16:]
    pool = []
    for allele in (bb, short):
        for k, start in enumerate(range(0, len(allele) - read_len + 1, stride)):
            r = list(allele[start:start + read_len])
            if k % 3 == 0:
                r[20] = "ACGT"[("ACGT".index(r[20]) + 1) % 4]
            pool.append("".join(r))
    rng.shuffle(pool)
    text = "".join(">t%d\n%s\n" % (k, pool[k % len(pool)]) for k in range(n_reads)).encode()
    return dict(Genes={"T": {"T*BACKBONE": bb}}, Vars={"T": Vars}, Var_list={"T": Var_list}, refGenes={"T": "T*BACKBONE"}), [text]


def paralog_reads(n_pairs):
    """(reference dicts, [mate-1 FASTA, mate-2 FASTA]): P (2 500 bases) and Q (900 bases), Q[300:600] = P[1000:1300] but for one base."""
    rng = random.Random(9)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))          # noqa: E731
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = lambda s: "".join(comp[b] for b in reversed(s))                   # noqa: E731
    p = seq(2500)
    q = list(seq(300) + p[1000:1300] + seq(300))
    q[450] = "ACGT"[("ACGT".index(q[450]) + 1) % 4]
    q = "".join(q)
    m1, m2 = [], []
    for k in range(n_pairs):
        a = 1000 + (k * 7) % 200                                           # mate 1 at P[a : a + 100], inside the stretch
        home = (k // 3) % 2                                                # 0: the fragment is P's, 1: Q's
        if home == 0:
            b = a + 300 + (k * 13) % 200
            m1.append((p if k % 3 else q)[a if k % 3 else a - 700:][:100])   # every third: mate 1 reads as Q's copy does
            m2.append(rc(p[b:b + 100]))
        else:
            m1.append(q[a - 700:a - 600])
            m2.append(rc(q[700 + (k * 13) % 100:][:100]))
    texts = ["".join(">r%d\n%s\n" % (k, s) for k, s in enumerate(m)).encode() for m in (m1, m2)]
    return dict(Genes={"P": {"P*BACKBONE": p}, "Q": {"Q*BACKBONE": q}}, Vars={}, Var_list={},
                refGenes={"P": "P*BACKBONE", "Q": "Q*BACKBONE"}), texts


def overhang_reads(err_percent, n_reads, read_len=100, step=7, tail_every=5):
    """(reference dicts, [one FASTA text])"""
    loc = synth.make_hla_like_locus(n_alleles=200, n_vars=1500, seed=5)
    d = loc.reference_dicts()
    rng = random.Random(11)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))          # noqa: E731
    ext = seq(read_len) + loc.backbone.upper() + seq(read_len)
    pool = []
    for k, start in enumerate(range(read_len // 2, len(ext) - read_len - read_len // 2 + 1, step)):
        r = list(ext[start:start + read_len])
        if k % tail_every == 0:
            r[-10:] = seq(10)
        for i in range(read_len):
            if rng.random() * 100.0 < err_percent:
                r[i] = "ACGT"[("ACGT".index(r[i]) + rng.randrange(1, 4)) % 4]
        pool.append("".join(r))
    rng.shuffle(pool)
    text = "".join(">o%d\n%s\n" % (k, pool[k % len(pool)]) for k in range(n_reads)).encode()
    return d, [text]


def novel_reads(err_percent, n_pairs, pool_pairs=2000, read_len=100):
    """(reference dicts, [mate-1 FASTA, mate-2 FASTA])"""
    loc = synth.make_hla_like_locus(n_alleles=200, n_vars=1500, seed=5)
    d = loc.reference_dicts()
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = lambda s: "".join(comp.get(b, b) for b in reversed(s))           # noqa: E731
    als = synth.simulate_pairs(loc, loc.allele_names[1:7], pool_pairs, read_len=read_len, frag_len=(300, 400), err_rate=err_percent / 100.0,
                               seed=13, novel_del_frac=0.1, novel_ins_frac=0.1)
    mates = [[], []]
    for a in als:
        mates[0 if a.flag & 0x40 else 1].append((rc(a.seq) if a.flag & 0x10 else a.seq).upper())
    texts = ["".join(">r%d\n%s\n" % (k, m[k % len(m)]) for k in range(n_pairs)).encode() for m in mates]
    return d, texts


def mixed_reads(err_percent, n_reads):
    """(reference dicts, [one FASTA text]): overhang_reads and novel_reads (both build the same locus), half and half, shuffled."""
    d, (over,) = overhang_reads(err_percent, n_reads // 2)
    _, novel = novel_reads(err_percent, (n_reads - n_reads // 2 + 1) // 2)
    seqs = [t.decode().split("\n")[1::2] for t in (over, novel[0], novel[1])]
    pool = (seqs[0] + seqs[1] + seqs[2])[:n_reads]
    random.Random(17).shuffle(pool)
    return d, ["".join(">m%d\n%s\n" % (k, s) for k, s in enumerate(pool)).encode()]


def timed(ix, texts, reps, **kw):
    out = ix.align(texts, **kw)                                       # warm-up
    last = align.align_last()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        ix.align(texts, **kw)
        ts.append(time.perf_counter() - t)
    return out, last, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("synth", "tandem", "paralog", "overhang", "novel", "mixed"), default="synth")
    ap.add_argument("--pair", action="store_true", help="also time the device route with pair=\"aware\"")
    ap.add_argument("--clip", type=int, default=0, help="also time both routes with clip=N")
    ap.add_argument("--gap", type=int, default=0, help="also time both routes with gap=N")
    ap.add_argument("--rescue", default=None, help="G,C: also time both routes with gap=G, with clip=C and with rescue=(G, C)")
    ap.add_argument("--search", choices=sorted(align.SEARCHES), default="ways")
    ap.add_argument("--err", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--tandem-indels", type=int, default=12)
    ap.add_argument("--no-host", action="store_true", help="time the device-route call only")
    args = ap.parse_args()
    sizes = args.sizes or {"synth": "250,500,1000,2000,4000,16000,64000", "tandem": "64", "paralog": "16000,64000",
                           "overhang": "16000,64000", "novel": "16000,64000", "mixed": "16000,64000"}[args.workload]
    capi.set_device(0)
    search = {} if args.search == "ways" else {"search": args.search}
    configs = [("device " + args.search, dict(route="device", **search))]
    if not args.no_host:
        configs.append(("host ways", dict(route="host")))
        if search:
            configs.append(("host states", dict(route="host", search="states")))
    if args.pair:
        assert not search, "pair=\"aware\" needs --search ways"
        configs.insert(1, ("device ways pairs", dict(route="device", pair="aware")))
    if args.clip:
        assert not search and not args.pair, "clip needs --search ways and no --pair"
        configs.append(("device ways clip", dict(route="device", clip=args.clip)))
        if not args.no_host:
            configs.append(("host ways clip", dict(route="host", clip=args.clip)))
    if args.gap:
        assert not search and not args.pair and not args.clip, "gap needs --search ways, no --pair and no --clip"
        configs.append(("device ways gap", dict(route="device", gap=args.gap)))
        if not args.no_host:
            configs.append(("host ways gap", dict(route="host", gap=args.gap)))
    rescue = None
    if args.rescue:
        assert not search and not args.pair and not args.clip and not args.gap, "rescue needs --search ways and none of --pair, --clip, --gap"
        rescue = tuple(int(x) for x in args.rescue.split(","))
        for route in ["device"] + ([] if args.no_host else ["host"]):
            configs.append(("%s ways gap" % route, dict(route=route, gap=rescue[0])))
            configs.append(("%s ways clip" % route, dict(route=route, clip=rescue[1])))
            configs.append(("%s ways rescue" % route, dict(route=route, rescue=rescue)))
    rows = []
    for n in [int(x) for x in sizes.split(",")]:
        d, texts = (reads_of(args.err, n // 2) if args.workload == "synth" else paralog_reads(n // 2) if args.workload == "paralog"
                    else overhang_reads(args.err, n) if args.workload == "overhang" else novel_reads(args.err, n // 2)
                    if args.workload == "novel" else mixed_reads(args.err, n) if args.workload == "mixed"
                    else tandem_reads(args.tandem_indels, n))
        ix = align.AlignIndex(d["Genes"], d["Vars"], d["Var_list"], d["refGenes"])
        outs, clip_outs, med, rescue_outs = [], [], {}, {}
        for name, kw in configs:
            out, last, ts = timed(ix, texts, args.reps, **kw)
            if rescue:
                base, tier = name.rsplit(" ", 1) if name.split()[-1] in ("gap", "clip", "rescue") else (name, None)
                chunks = -(-n // 8192)
                if tier is None:
                    outs.append(out)
                else:
                    rescue_outs.setdefault(tier, []).append(out)
                    cost = (statistics.median(ts) - med[base]) * 1e3 / chunks
                    med[name + " cost"] = cost
                    print("%7d reads  %-18s aligned %d; clip: searched %d clipped %d bases %d; gap: searched %d gapped %d bases %d; %+.3f ms per "
                          "8 192-read chunk against %s" % (n, name, last["aligned"], last["clip_searched"], last["clip_clipped"],
                                                          last["clip_bases"], last["gap_searched"], last["gap_gapped"], last["gap_bases"], cost,
                                                          base), flush=True)
                    if tier == "rescue":
                        both = med[base + " gap cost"] + med[base + " clip cost"]
                        print("%7d reads  %-18s kept out of the gap pass by the cost rule: %d of %d; cost / (gap cost + clip cost) = %.3f" % (
                            n, name, last["clip_searched"] - last["gap_searched"], last["clip_searched"], cost / both if both else float("nan")),
                            flush=True)
            elif kw.get("clip"):
                base = name[:-5]
                chunks = -(-n // 8192)
                clip_outs.append(out)
                print("%7d reads  %-18s clip %d: searched %d clipped %d bases %d; %+.3f ms per 8 192-read chunk against %s" % (
                    n, name, kw["clip"], last["clip_searched"], last["clip_clipped"], last["clip_bases"],
                    (statistics.median(ts) - med[base]) * 1e3 / chunks, base), flush=True)
            elif kw.get("gap"):
                base = name[:-4]
                chunks = -(-n // 8192)
                clip_outs.append(out)
                print("%7d reads  %-18s gap %d: searched %d gapped %d bases %d; %+.3f ms per 8 192-read chunk against %s" % (
                    n, name, kw["gap"], last["gap_searched"], last["gap_gapped"], last["gap_bases"],
                    (statistics.median(ts) - med[base]) * 1e3 / chunks, base), flush=True)
            elif kw.get("pair") == "aware":
                chunks = -(-n // 8192)
                print("%7d reads  %-18s pairs searched %d placed %d changed %d; %+.3f ms per 8 192-read chunk against %s" % (
                    n, name, last["pairs_searched"], last["pairs_placed"], last["pairs_changed"],
                    (statistics.median(ts) - med[configs[0][0]]) * 1e3 / chunks, configs[0][0]), flush=True)
            else:
                outs.append(out)
            med[name] = statistics.median(ts)
            print("%7d reads  %-18s median %10.3f ms  range %10.3f .. %10.3f ms  %10.0f reads/s   route %d decline %d aligned %d  "
                  "states: reads %d anchors %d cells %d" % (
                      n, name, med[name] * 1e3, min(ts) * 1e3, max(ts) * 1e3, n / med[name], last["route"], last["decline"],
                      last["aligned"], last["states_reads"], last["states_anchors"], last["states_cells"]),
                  flush=True)
        assert all(o == outs[0] for o in outs) and all(o == clip_outs[0] for o in clip_outs)
        assert all(o == v[0] for v in rescue_outs.values() for o in v)
        rows.append((n, med[configs[0][0]], med.get("host ways")))
        ix.close()
    if args.workload == "synth" and not args.no_host:
        for (n0, d0, h0), (n1, d1, h1) in zip(rows, rows[1:]):
            if d0 > h0 and d1 <= h1:
                print("break-even between %d and %d reads" % (n0, n1))
        if rows and rows[0][1] <= rows[0][2]:
            print("the device route is already ahead at %d reads" % rows[0][0])


if __name__ == "__main__":
    main()
