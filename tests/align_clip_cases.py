"""Inputs the clip tier's three statements (tests/align_clip_ref.py, the host route, the kernels) are judged on: hand-made loci with
their records written by hand, overhang tilings of a synth locus, and the inputs of tests/align_cases.py under clip = 32."""
import gzip
import random

import align_cases
import align_clip_ref
import align_ref
from align_cases import _bb, _other, _plain_md, fasta, fastq

CLIP = 32
L = align_ref.Locus
rc = align_ref.revcomp


def _junk(seed, n):
    return _bb(900 + seed, n)


def _not(*bases):
    return [b for b in "ACGT" if b not in bases][0]


def hand_cases():
    """[(title, [Locus], reads [(name, seq)], max_edits, clip, expected)], expected as align_cases.hand_cases()."""
    cases = []

    # -- overhangs of 1 and of `clip` bases at either end, and of clip + 1 (unaligned) -----------------------------------------
    bb = _bb(101, 300)
    loc = L("C1*BACKBONE", bb, [])
    j = _junk(1, 40)
    reads = [("l1", j[:1] + bb[:99]), ("l32", j[:32] + bb[:68]), ("l33", j[:33] + bb[:67]),
             ("r1", bb[201:] + j[:1]), ("r32", bb[232:] + j[:32]), ("r33", bb[233:] + j[:33])]
    cases.append(("overhangs", [loc], reads, 2, CLIP, [
        (0, "C1*BACKBONE", 1, 60, "1S99M", "NM:i:0\tMD:Z:99\tNH:i:1"),
        (0, "C1*BACKBONE", 1, 60, "32S68M", "NM:i:0\tMD:Z:68\tNH:i:1"),
        None,
        (0, "C1*BACKBONE", 202, 60, "99M1S", "NM:i:0\tMD:Z:99\tNH:i:1"),
        (0, "C1*BACKBONE", 233, 60, "68M32S", "NM:i:0\tMD:Z:68\tNH:i:1"),
        None]))

    # -- an overhang at both ends of a short locus ------------------------------------------------------------------------------
    bb = _bb(102, 60)
    loc = L("C2*BACKBONE", bb, [])
    cases.append(("both ends", [loc], [("b", j[:10] + bb + j[10:22])], 2, CLIP, [
        (0, "C2*BACKBONE", 1, 60, "10S60M12S", "NM:i:0\tMD:Z:60\tNH:i:1")]))

    # -- a tail with max_edits + 1 mismatches: clipped up to the outermost of them, the other two stay edits ------------------------
    bb = _bb(103, 400)
    loc = L("C3*BACKBONE", bb, [])
    t = list(bb[100:200])
    for k in (80, 88, 95):
        t[k] = _other(t[k])
    cases.append(("tail with three mismatches", [loc], [("t3", "".join(t))], 2, CLIP, [
        (0, "C3*BACKBONE", 101, 60, "95M5S", "NM:i:2\tMD:Z:80%s7%s6\tNH:i:1" % (bb[180], bb[188]))]))

    # -- (clip 10, NM 2) beats (clip 11, NM 1) and (clip 12, NM 0): mismatches at 88, 89, 90 of a 100-base read, budget 2 -----------
    t = list(bb[200:300])
    for k in (88, 89, 90):
        t[k] = _other(t[k])
    t2 = list(rc(bb[200:300]))                                     # the same on the - strand: the tail is the record's LEFT end
    for k in (88, 89, 90):
        t2[k] = _other(t2[k])
    cases.append(("fewest clipped bases first", [loc], [("c10", "".join(t)), ("c10rc", "".join(t2))], 2, CLIP, [
        (0, "C3*BACKBONE", 201, 60, "90M10S", "NM:i:2\tMD:Z:88%s0%s0\tNH:i:1" % (bb[288], bb[289])),
        (16, "C3*BACKBONE", 211, 60, "10S90M", "NM:i:2\tMD:Z:0%s0%s88\tNH:i:1" % (bb[210], bb[211]))]))

    # -- a known deletion and a known insertion inside the aligned part of a clipped read; Zs gaps from the first aligned base --------
    bb = _bb(104, 400)
    loc = L("C4*BACKBONE", bb, [("deletion", 150, "3", "hv0"), ("insertion", 180, "GATTACA", "hv1")])
    rd = j[:4] + _not(bb[119]) + bb[120:150] + bb[153:180] + "GATTACA" + bb[180:200] + _not(bb[200]) + j[5:13]
    cases.append(("known indels inside a clipped read", [loc], [("di", rd), ("dirc", rc(rd))], 0, CLIP, [
        (0, "C4*BACKBONE", 121, 60, "5S30M3D27M7I20M9S", "NM:i:0\tMD:Z:30^%s47\tZs:Z:30|D|hv0,27|I|hv1\tNH:i:1" % bb[150:153]),
        (16, "C4*BACKBONE", 121, 60, "5S30M3D27M7I20M9S", "NM:i:0\tMD:Z:30^%s47\tZs:Z:30|D|hv0,27|I|hv1\tNH:i:1" % bb[150:153])]))

    # -- a known indel right at the clip boundary is not taken: the read ends with the inserted bases + junk (right), or starts with
    #    junk + the bases behind a deletion (left) -------------------------------------------------------------------------------------
    bb = _bb(105, 400)
    loc = L("C5*BACKBONE", bb, [("insertion", 200, "GATTACAGG", "hv0"), ("deletion", 100, "4", "hv1")])
    at_r = bb[140:200] + "GATTACAGG" + _not(bb[200]) + _junk(2, 5)      # taking hv0 would save 9 clipped bases; a way never ends in an indel
    at_l = _junk(3, 5) + _not(bb[99], bb[103]) + bb[104:170]            # the deletion in front of the first aligned base is not taken
    e_r = _clip_right_expect(bb, 140, at_r, 200)
    cases.append(("indel at the clip boundary", [loc], [("ir", at_r), ("dl", at_l)], 0, CLIP, [
        (0, "C5*BACKBONE", 141, 60) + e_r,
        (0, "C5*BACKBONE", 105, 60, "6S66M", "NM:i:0\tMD:Z:66\tNH:i:1")]))

    # -- NH 2 for a clipped read on two loci ----------------------------------------------------------------------------------------
    shared = _bb(106, 80)
    la = L("C6*BACKBONE", _bb(107, 100) + shared + _bb(108, 100), [])
    lb = L("C7*BACKBONE", _bb(109, 50) + shared + _bb(110, 70), [])
    cases.append(("clipped on two loci", [la, lb], [("two", shared[10:80] + _not(la.bb[180], lb.bb[130]) + _junk(4, 19))], 0, CLIP, [
        (0, "C6*BACKBONE", 111, 1, "70M20S", "NM:i:0\tMD:Z:70\tNH:i:2")]))
    return cases


def _clip_right_expect(bb, pos0, read, stop):
    """(cigar, tags) of a read aligned from pos0 whose bases from backbone position `stop` on are clipped, NM 0."""
    n = stop - pos0
    assert read[:n] == bb[pos0:stop]
    return ("%dM%dS" % (n, len(read) - n), "NM:i:0\tMD:Z:%d\tNH:i:1" % n)


def pair_case():
    """(loci, mate-1 records, mate-2 records): mate 2 of `up` hangs over the locus' right end, so the default writes mate 1 as UP and
    clip = 32 writes a CP pair; `cp` is concordant either way."""
    bb = _bb(111, 500)
    loc = L("C8*BACKBONE", bb, [])
    m1 = [("up", bb[250:350]), ("cp", bb[100:200])]
    m2 = [("up", rc(bb[420:500] + _junk(5, 20))), ("cp", rc(bb[300:400]))]
    return [loc], m1, m2


def overhang_pairs(err_percent, seed=7, read_len=100, step=7, tail_every=5, gap=50):
    """(synth locus, dicts, mate-1 records, mate-2 records): fragments tiled over a synth locus' backbone so that reads start from
    -L/2 and end up to len(bb) + L/2 (the parts outside are random bases); mate 1 is the fragment's first `read_len` bases, mate 2
    the reverse complement of its last; every `tail_every`-th mate 1 ends in a ten-base random tail; `err_percent` per-base
    errors."""
    from hisatgenotype_amd import synth
    loc = synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=seed)
    d = loc.reference_dicts()
    bb = loc.backbone.upper()
    rng = random.Random(seed)
    ext = align_cases.rand_seq(rng, read_len) + bb + align_cases.rand_seq(rng, read_len)
    frag = 2 * read_len + gap

    def errors(s):
        s = list(s)
        for i in range(len(s)):
            if rng.random() * 100.0 < err_percent:
                s[i] = _other(s[i], rng.randrange(1, 4))
        return "".join(s)

    m1, m2 = [], []
    for k, start in enumerate(range(read_len // 2, len(ext) - frag - read_len // 2 + 1, step)):
        a, b = ext[start:start + read_len], ext[start + frag - read_len:start + frag]
        if k % tail_every == 0:
            a = a[:-10] + align_cases.rand_seq(rng, 10)
        m1.append(("ov%d" % k, errors(a)))
        m2.append(("ov%d" % k, rc(errors(b))))
    return loc, (d["Genes"], d["Vars"], d["Var_list"], d["refGenes"]), m1, m2


def random_case(rng):
    """(loci, reads, max_edits, clip): a short backbone over a small alphabet (ties, several diagonals) with up to 13 known variants,
    and reads cut across it and over its ends, with random substitutions, random tails and sometimes a known variant applied."""
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
    for r in range(12):
        n_r = rng.choice([20, 33, 50])
        a = rng.randrange(-10, n - n_r + 10)
        s = [bb[i] if 0 <= i < n else rng.choice("ACGT") for i in range(a, a + n_r)]
        for _ in range(rng.randrange(0, 4)):
            s[rng.randrange(n_r)] = rng.choice("ACGT")
        if rng.random() < 0.4:
            k = rng.randrange(1, 9)
            s[-k:] = [rng.choice("ACGT") for _ in range(k)]
        s = "".join(s)
        if vs and rng.random() < 0.5:
            t, p, d, _ = rng.choice(vs)
            q = p - a
            if 2 < q < n_r - 2:
                s = (s[:q] + d + s[q:])[:n_r] if t == "insertion" else s[:q] + s[q + int(d):] if t == "deletion" else s[:q] + d + s[q + 1:]
        if len(s) >= 16:
            reads.append(("r%d" % r, rc(s) if rng.random() < 0.3 else s))
    return loci, reads, rng.randrange(0, 4), rng.choice([1, 3, 8, 32])


_RANDOM = []


def random_cases(n=60, seed=5):
    """[(loci, reads, max_edits, clip, the statement's text, its counters)], computed once per process."""
    if not _RANDOM:
        rng = random.Random(seed)
        for _ in range(n):
            loci, reads, me, clip = random_case(rng)
            st = {}
            text = align_clip_ref.align_text(loci, [[(q, s, None) for q, s in reads]], me, clip=clip, stats=st).encode()
            _RANDOM.append((loci, reads, me, clip, text, st))
    return _RANDOM


_INPUTS = {}


def inputs():
    """{id: (dicts, [input texts (bytes)], max_edits, clip)}: the hand cases, the pair, overhang tilings at 0 and 1 % errors, formats
    (FASTA, FASTQ, gzip; single and paired) and read lengths 16, 17, 100 and 1 024."""
    if _INPUTS:
        return _INPUTS
    for k, (title, loci, reads, me, clip, _) in enumerate(hand_cases()):
        _INPUTS["chand%d" % k] = (align_cases.dicts_of(loci), [fasta(reads)], me, clip)
    loci, m1, m2 = pair_case()
    pd = align_cases.dicts_of(loci)
    q1 = [(n, s, align_cases._quals(s, k)) for k, (n, s) in enumerate(m1)]
    q2 = [(n, s, align_cases._quals(s, k + 3)) for k, (n, s) in enumerate(m2)]
    _INPUTS["cpair-fasta"] = (pd, [fasta(m1), fasta(m2)], 2, CLIP)
    _INPUTS["cpair-fastq-gz"] = (pd, [gzip.compress(fastq(q1)), gzip.compress(fastq(q2))], 2, CLIP)
    _INPUTS["csingle-fastq"] = (pd, [fastq(q1 + q2)], 2, CLIP)
    for err in (0, 1):
        _, d, o1, o2 = overhang_pairs(float(err))
        _INPUTS["overhang-err%d" % err] = (d, [fasta(o1), fasta(o2)], 2, CLIP)
    _INPUTS["overhang-single"] = (d, [fasta(o1 + o2)], 2, CLIP)
    # lengths: reads of 16, 17, 100 and 1 024 bases hanging 3 bases over the right end of a locus (a 16-base read has one seed,
    # which must lie inside: it hangs over by 0 and is written end to end or not at all)
    bb = _bb(112, 1400)
    loc = L("C9*BACKBONE", bb, [])
    tail = _junk(6, 3)
    reads = [("len16", bb[-16:]), ("len17", bb[-16:] + tail[:1]), ("len100", bb[-97:] + tail), ("len1024", bb[-1021:] + tail)]
    _INPUTS["clengths"] = (align_cases.dicts_of([loc]), [fasta(reads)], 2, CLIP)
    return _INPUTS


INPUT_IDS = (["chand%d" % k for k in range(7)] + ["cpair-fasta", "cpair-fastq-gz", "csingle-fastq", "overhang-err0", "overhang-err1", "overhang-single",
                                                  "clengths"])

_REF = {}


def ref_text(key, clip=None, stats=None):
    """The clip statement's SAM text for inputs()[key] (bytes), and its counters into `stats`."""
    d, texts, me, c = inputs()[key] if key in inputs() else align_cases.inputs()[key] + (CLIP,)
    c = c if clip is None else clip
    if (key, c) not in _REF:
        loci = align_ref.loci_from_dicts(d[0], d[1], d[2], d[3])
        st = {}
        text = align_clip_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me, clip=c, stats=st).encode()
        _REF[(key, c)] = (text, st)
    if stats is not None:
        stats.update(_REF[(key, c)][1])
    return _REF[(key, c)][0]


def records(text):
    return [l for l in text.decode().split("\n") if l and not l.startswith("@")]


def is_clipped(line):
    return "S" in line.split("\t")[5]
