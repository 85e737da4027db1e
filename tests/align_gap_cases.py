"""Inputs the gap tier's three statements (tests/align_gap_ref.py, the host route, the kernels) are judged on: hand-made loci with
their records written by hand, synth reads with novel 1- and 2-base indels, formats and lengths, seeded random loci, and the inputs
of tests/align_cases.py under gap = 16."""
import gzip
import random

import align_cases
import align_gap_ref
import align_ref
from align_cases import _bb, _other, fasta, fastq

GAP = 16
L = align_ref.Locus
rc = align_ref.revcomp


def _not(*bases):
    return [b for b in "ACGT" if b not in bases][0]


def _plant(bb, at, motif):
    """bb with `motif` written over its bases from `at` on."""
    return bb[:at] + motif + bb[at + len(motif):]


def hand_cases():
    """[(title, [Locus], reads [(name, seq)], max_edits, gap, expected)], expected as align_cases.hand_cases(): one entry per read,
    None (unaligned) or (flag, rname, pos1, mapq, cigar, tags without YT).  Every site is planted so that the neighbouring bases
    differ from the gap's: the expected gap position is the only one (except in the tie-break cases, which say so)."""
    cases = []

    # 0 -- lengths: a deletion of 1, of N = 3 and of N + 1 (unaligned: the budget of 5 would pay for it), the same for insertions ---
    bb = _plant(_bb(301, 400), 147, "CAGTCTGA")                    # 147 .. 154; the gaps sit in front of 150 = 'T'
    loc = L("H1*BACKBONE", bb, [])
    a = bb[100:150]
    reads = [("d1", a + bb[151:201]), ("d3", a + bb[153:203]), ("d4", a + bb[154:204]),
             ("i1", a + "A" + bb[150:199]), ("i3", a + "AGA" + bb[150:197]), ("i4", a + "AGAG" + bb[150:196])]
    cases.append(("lengths", [loc], reads, 5, 3, [
        (0, "H1*BACKBONE", 101, 60, "50M1D50M", "NM:i:1\tMD:Z:50^T50\tNH:i:1"),
        (0, "H1*BACKBONE", 101, 60, "50M3D50M", "NM:i:3\tMD:Z:50^TCT50\tNH:i:1"),
        None,
        (0, "H1*BACKBONE", 101, 60, "50M1I49M", "NM:i:1\tMD:Z:99\tNH:i:1"),
        (0, "H1*BACKBONE", 101, 60, "50M3I47M", "NM:i:3\tMD:Z:97\tNH:i:1"),
        None]))

    # 1, 2 -- a gap of 2 and a mismatch: unaligned with max_edits 2, NM 3 with 3 ------------------------------------------------
    rd = list(a + bb[152:202])
    rd[80] = _other(rd[80])
    rd = "".join(rd)
    cases.append(("gap 2 + 1 mismatch, budget 2", [loc], [("g2m", rd)], 2, GAP, [None]))
    cases.append(("gap 2 + 1 mismatch, budget 3", [loc], [("g2m", rd)], 3, GAP, [
        (0, "H1*BACKBONE", 101, 60, "50M2D50M", "NM:i:3\tMD:Z:50^TC30%s19\tNH:i:1" % bb[182])]))

    # 3 -- the gap touching the anchor: a 32-base read has the seeds 0, 4, 8, 12, 16; with the deletion at r = 16 only the seeds 0
    #      (gap at o + 16) and 16 (gap at o) are whole, and a mismatch spoils one of the two.  A 30-base read with the gap at r = 15
    #      has no whole seed (0 .. 15 and 14 .. 29 both span it): unaligned.  A gap one base from a read end: the read aligns end to
    #      end with one mismatch and is written as align_ref writes it. ------------------------------------------------------------------
    r32 = bb[134:150] + bb[151:167]
    right, left = list(r32), list(r32)
    right[20] = _other(right[20])                                  # spoils seed 16: the gap is at r = o + 16 of seed 0
    left[10] = _other(left[10])                                    # spoils seed 0: the gap is at r = o of seed 16
    r30 = bb[135:150] + bb[151:166]
    end1 = bb[149] + bb[151:250]                                   # "deletion" behind the first base
    cases.append(("the gap and the anchor", [loc], [("o16", "".join(right)), ("o0", "".join(left)), ("r15", r30), ("end1", end1)], 2, GAP, [
        (0, "H1*BACKBONE", 135, 60, "16M1D16M", "NM:i:2\tMD:Z:16^T4%s11\tNH:i:1" % bb[155]),
        (0, "H1*BACKBONE", 135, 60, "16M1D16M", "NM:i:2\tMD:Z:10%s5^T16\tNH:i:1" % bb[144]),
        None,
        (0, "H1*BACKBONE", 151, 60, "100M", "NM:i:1\tMD:Z:0%s99\tNH:i:1" % bb[150])]))

    # 4 -- tie-breaks: a homopolymer and a dinucleotide repeat give the leftmost gap; deletion before insertion at one offset; the
    #      shorter gap at one offset and kind -------------------------------------------------------------------------------------
    hb = _plant(_bb(302, 400), 149, "CAAAAAAG")                    # A x 6 at 150 .. 155
    hb = _plant(hb, 249, "GCACACACAT")                             # CA x 4 at 250 .. 257
    #   kind: ..A GTG.. with the read ending in TG (max_edits 1): deleting the first G (T on T, G on G) and inserting the T (G on
    #   the first G) both cost 1 at r = L - 2; end to end costs 2
    hb = _plant(hb, 348, "CAGTGC")                                 # G T G at 350 .. 352
    hloc = L("H2*BACKBONE", hb, [])
    homo = hb[100:150] + "AAAAA" + hb[156:201]
    homo_i = hb[100:150] + "AAAAAAA" + hb[156:199]
    dinuc = hb[200:250] + "CACACA" + hb[258:302]
    kind = hb[252:350] + "TG"
    cases.append(("leftmost", [hloc], [("homo", homo), ("homoi", homo_i), ("dinuc", dinuc)], 2, GAP, [
        (0, "H2*BACKBONE", 101, 60, "50M1D50M", "NM:i:1\tMD:Z:50^A50\tNH:i:1"),
        (0, "H2*BACKBONE", 101, 60, "50M1I49M", "NM:i:1\tMD:Z:99\tNH:i:1"),
        (0, "H2*BACKBONE", 201, 60, "50M2D50M", "NM:i:2\tMD:Z:50^CA50\tNH:i:1")]))
    cases.append(("deletion before insertion", [hloc], [("kind", kind)], 1, GAP, [
        (0, "H2*BACKBONE", 253, 60, "98M1D2M", "NM:i:1\tMD:Z:98^G2\tNH:i:1")]))
    #   length: ..T GAAACC.. with the read ending in AACC (max_edits 2): at r = L - 4 deleting G costs 1 + the mismatch C on A,
    #   deleting GA costs 2; end to end costs 3
    lb = _plant(_bb(303, 400), 349, "TGAAACCT")                    # G at 350
    lloc = L("H3*BACKBONE", lb, [])
    cases.append(("the shorter gap", [lloc], [("len", lb[254:350] + "AACC")], 2, GAP, [
        (0, "H3*BACKBONE", 255, 60, "96M1D4M", "NM:i:2\tMD:Z:96^G2A1\tNH:i:1")]))

    # 6 -- known variants around the gap: a novel deletion of 149 leads to the state (49, 150), whose known insertion and known
    #      deletion follow at once; a known deletion elsewhere in the read; a novel deletion that equals a known one IS the known one
    #      (end to end, free, no gap) ------------------------------------------------------------------------------------------------
    kb = _plant(_bb(304, 400), 146, "GTCAGTCA")                    # 149 = 'A', 150 = 'G'
    kloc = L("H4*BACKBONE", kb, [("deletion", 120, "3", "hv0"), ("insertion", 150, "CCTCCTC", "hv1"), ("deletion", 150, "2", "hv2"),
                                 ("deletion", 300, "2", "hv3")])
    both = kb[100:120] + kb[120:149] + "CCTCCTC" + kb[152:196]
    far = kb[100:120] + kb[123:200] + "T" + kb[200:202]            # hv0 taken, a novel T inserted in front of 200
    assert kb[199] != "T" and kb[200] != "T"
    same = kb[250:300] + kb[302:352]
    cases.append(("known indels around the gap", [kloc], [("both", both), ("far", far), ("same", same)], 2, GAP, [
        (0, "H4*BACKBONE", 101, 60, "49M1D7I2D44M", "NM:i:1\tMD:Z:49^A0^%s44\tZs:Z:49|I|hv1,7|D|hv2\tNH:i:1" % kb[150:152]),
        (0, "H4*BACKBONE", 101, 60, "20M3D77M1I2M", "NM:i:1\tMD:Z:20^%s79\tZs:Z:20|D|hv0\tNH:i:1" % kb[120:123]),
        (0, "H4*BACKBONE", 251, 60, "50M2D50M", "NM:i:0\tMD:Z:50^%s50\tZs:Z:50|D|hv3\tNH:i:1" % kb[300:302])]))

    # 7 -- rendering: a gap followed at once by a mismatch; an insertion in front of a known single (its bases count into the gap of
    #      the single's Zs item) -----------------------------------------------------------------------------------------------------
    rb = _plant(_bb(305, 400), 147, "CAGATCGA")                    # 150 = 'A', 151 = 'T'
    rloc = L("H5*BACKBONE", rb, [("single", 160, _other(rb[160]), "hv0")])
    mm = rb[100:150] + "C" + rb[152:201]                         # 150 deleted, C on the T of 151
    sg = rb[100:150] + "TT" + rb[150:160] + _other(rb[160]) + rb[161:198]
    cases.append(("rendering", [rloc], [("mm", mm), ("sg", sg)], 2, GAP, [
        (0, "H5*BACKBONE", 101, 60, "50M1D50M", "NM:i:2\tMD:Z:50^A0T49\tNH:i:1"),
        (0, "H5*BACKBONE", 101, 60, "50M2I48M", "NM:i:2\tMD:Z:60%s37\tZs:Z:62|S|hv0\tNH:i:1" % rb[160])]))

    # 8 -- both strands, and NH 2 for a gapped read on two loci -----------------------------------------------------------------------
    shared = _plant(_bb(306, 100), 47, "CAGTCTGA")
    la = L("H6*BACKBONE", _bb(307, 100) + shared + _bb(308, 100), [])
    lb2 = L("H7*BACKBONE", _bb(309, 50) + shared + _bb(310, 70), [])
    two = shared[10:50] + shared[51:91]
    cases.append(("strands and loci", [loc, la, lb2], [("fw", reads[0][1]), ("rv", rc(reads[0][1])), ("two", two), ("twor", rc(two))], 2, GAP, [
        (0, "H1*BACKBONE", 101, 60, "50M1D50M", "NM:i:1\tMD:Z:50^T50\tNH:i:1"),
        (16, "H1*BACKBONE", 101, 60, "50M1D50M", "NM:i:1\tMD:Z:50^T50\tNH:i:1"),
        (0, "H6*BACKBONE", 111, 1, "40M1D40M", "NM:i:1\tMD:Z:40^T40\tNH:i:2"),
        (16, "H6*BACKBONE", 111, 1, "40M1D40M", "NM:i:1\tMD:Z:40^T40\tNH:i:2")]))
    return cases


N_HAND = 10


def pair_case():
    """(loci, mate-1 records, mate-2 records): mate 2 of `up` carries a novel deletion, so the default writes mate 1 as UP and
    gap = 16 writes a CP pair; `cp` is concordant either way."""
    bb = _plant(_bb(311, 600), 447, "CAGTCTGA")
    loc = L("H8*BACKBONE", bb, [])
    m1 = [("up", bb[250:350]), ("cp", bb[100:200])]
    m2 = [("up", rc(bb[400:450] + bb[451:501])), ("cp", rc(bb[300:400]))]
    return [loc], m1, m2


def synth_novel(err_percent, seed=11, n_pairs=60, read_len=100):
    """(dicts, mate-1 records, mate-2 records): pairs of synth.simulate_pairs over a synth locus in which a fifth of the reads
    carry a novel 1-base deletion and a fifth a novel 1- or 2-base insertion, `err_percent` per-base errors."""
    from hisatgenotype_amd import synth
    loc = synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=seed)
    d = loc.reference_dicts()
    als = synth.simulate_pairs(loc, synth.pick_sample(loc, seed), n_pairs, read_len=read_len, frag_len=(300, 300),
                               err_rate=err_percent / 100.0, seed=seed, novel_del_frac=0.2, novel_ins_frac=0.2)
    m1, m2 = [], []
    for a in als:
        s = rc(a.seq) if a.flag & 0x10 else a.seq
        (m1 if a.flag & 0x40 else m2).append((a.qname, s.upper()))
    assert len(m1) == len(m2) == n_pairs
    return (d["Genes"], d["Vars"], d["Var_list"], d["refGenes"]), m1, m2


def random_case(seed):
    """(loci, reads, max_edits, gap): a short backbone over a small alphabet (ties, several diagonals, repeats) with up to 13
    known variants, and reads cut from it with a novel deletion or insertion of 1 .. 3 bases, random substitutions and sometimes
    a known variant applied."""
    rng = random.Random(seed)
    n = rng.choice([60, 120, 200])
    alpha = rng.choice(["ACGT", "AC", "ACG"])
    bb = "".join(rng.choice(alpha) for _ in range(n))
    vs = []
    for k in range(rng.randrange(0, 14)):
        t, p = rng.choice(["single", "deletion", "insertion"]), rng.randrange(1, n - 1)
        d = (rng.choice([b for b in "ACGT" if b != bb[p]]) if t == "single" else str(rng.randrange(1, 5)) if t == "deletion"
             else "".join(rng.choice(alpha) for _ in range(rng.randrange(1, 5))))
        vs.append((t, p, d, "hv%d" % k))
    vs.sort(key=lambda v: v[1])
    loci = [L("F1*BACKBONE", bb, vs)]
    if rng.random() < 0.3:
        loci.append(L("F2*BACKBONE", bb[10:50] + align_cases.rand_seq(rng, 30), []))
    reads = []
    for r in range(10):
        n_r = rng.choice([24, 33, 50])
        a = rng.randrange(0, n - n_r - 4)
        s = bb[a:a + n_r + 4]
        if vs and rng.random() < 0.5:
            t, p, d, _ = rng.choice(vs)
            q = p - a
            if 2 < q < n_r - 2:
                s = s[:q] + d + s[q:] if t == "insertion" else s[:q] + s[q + int(d):] if t == "deletion" else s[:q] + d + s[q + 1:]
        if rng.random() < 0.8:                                     # the novel gap
            q, g = rng.randrange(1, n_r - 1), rng.randrange(1, 4)
            s = s[:q] + s[q + g:] if rng.random() < 0.5 else s[:q] + align_cases.rand_seq(rng, g) + s[q:]
        s = list(s[:n_r])
        for _ in range(rng.randrange(0, 3)):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        s = "".join(s)
        if len(s) >= 16:
            reads.append(("r%d" % r, rc(s) if rng.random() < 0.3 else s))
    return loci, reads, rng.randrange(1, 5), rng.choice([1, 2, 3, 16])


# seeds of random_case on which the statement writes at least one gapped record (chosen by running it over 0 .. 199; the test
# asserts the property again)
RANDOM_SEEDS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26, 28, 29, 30, 31, 33, 34, 35, 36, 37, 38, 39,
                41, 42, 43, 44, 45, 47, 48, 49, 50, 51, 52, 53, 55, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 69, 70, 71]

_RANDOM = []


def random_cases():
    """[(seed, loci, reads, max_edits, gap, the statement's text, its counters)], computed once per process."""
    if not _RANDOM:
        for seed in RANDOM_SEEDS:
            loci, reads, me, gap = random_case(seed)
            st = {}
            text = align_gap_ref.align_text(loci, [[(q, s, None) for q, s in reads]], me, gap=gap, stats=st).encode()
            _RANDOM.append((seed, loci, reads, me, gap, text, st))
    return _RANDOM


_INPUTS = {}


def inputs():
    """{id: (dicts, [input texts (bytes)], max_edits, gap)}: the hand cases, the pair in FASTA / FASTQ / gzip, single and paired,
    synth reads with novel indels at 0 and 1 % errors, and reads of 17, 33, 100 and 1 024 bases."""
    if _INPUTS:
        return _INPUTS
    for k, (title, loci, reads, me, gap, _) in enumerate(hand_cases()):
        _INPUTS["ghand%d" % k] = (align_cases.dicts_of(loci), [fasta(reads)], me, gap)
    loci, m1, m2 = pair_case()
    pd = align_cases.dicts_of(loci)
    q1 = [(n, s, align_cases._quals(s, k)) for k, (n, s) in enumerate(m1)]
    q2 = [(n, s, align_cases._quals(s, k + 3)) for k, (n, s) in enumerate(m2)]
    _INPUTS["gpair-fasta"] = (pd, [fasta(m1), fasta(m2)], 2, GAP)
    _INPUTS["gpair-fastq-gz"] = (pd, [gzip.compress(fastq(q1)), gzip.compress(fastq(q2))], 2, GAP)
    _INPUTS["gsingle-fastq"] = (pd, [fastq(q1 + q2)], 2, GAP)
    for err in (0, 1):
        d, s1, s2 = synth_novel(float(err))
        _INPUTS["novel-err%d" % err] = (d, [fasta(s1), fasta(s2)], 2, GAP)
    _INPUTS["novel-single"] = (d, [fasta(s1 + s2)], 2, GAP)
    # lengths: a deletion in reads of 17 (unaligned: no whole seed), 33, 100 and 1 024 bases
    bb = _plant(_bb(312, 1400), 297, "CAGTCTGA")
    loc = L("H9*BACKBONE", bb, [])
    reads = [("len17", bb[292:300] + bb[301:310]), ("len33", bb[283:300] + bb[301:317]), ("len100", bb[250:300] + bb[301:351]),
             ("len1024", bb[200:300] + bb[301:1225])]
    _INPUTS["glengths"] = (align_cases.dicts_of([loc]), [fasta(reads)], 2, GAP)
    return _INPUTS


INPUT_IDS = (["ghand%d" % k for k in range(N_HAND)] + ["gpair-fasta", "gpair-fastq-gz", "gsingle-fastq", "novel-err0", "novel-err1",
                                                       "novel-single", "glengths"])

_REF = {}


def ref_text(key, gap=None, stats=None, max_edits=None):
    """The gap statement's SAM text for inputs()[key] (bytes), and its counters into `stats`."""
    d, texts, me, g = inputs()[key] if key in inputs() else align_cases.inputs()[key] + (GAP,)
    g = g if gap is None else gap
    me = me if max_edits is None else max_edits
    if (key, g, me) not in _REF:
        loci = align_ref.loci_from_dicts(d[0], d[1], d[2], d[3])
        st = {}
        text = align_gap_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me, gap=g, stats=st).encode()
        _REF[(key, g, me)] = (text, st)
    if stats is not None:
        stats.update(_REF[(key, g, me)][1])
    return _REF[(key, g, me)][0]


def records(text):
    return [l for l in text.decode().split("\n") if l and not l.startswith("@")]


def is_gapped(line):
    """A record with a novel gap: an I or D of the CIGAR that no Zs item stands for."""
    f = line.split("\t")
    n_ops = sum(f[5].count(op) for op in "ID")
    zs = [t for t in f[11:] if t.startswith("Zs:Z:")]
    n_known = sum(1 for it in zs[0][5:].split(",") if it.split("|")[1] in "ID") if zs else 0
    return n_ops > n_known
