"""Inputs the three statements of "both tiers in one call" (tests/align_rescue_ref.py, the host route, the kernels with
hgx_align_more.rescue_clip > 0) are judged on: hand-made reads on the gap cases' first locus with their records written by hand,
a pair with one mate clipped and the other gapped, seeded random loci (align_gap_cases.random_case with overhanging reads added),
the formats and lengths of the gap cases, the synth inputs of both tiers and their mix over one locus."""
import gzip
import random

import align_cases
import align_clip_cases as cc
import align_clip_ref
import align_gap_cases as gc
import align_gap_ref
import align_ref
import align_rescue_ref as rr
from align_cases import _bb, fasta, fastq
from align_gap_cases import _not, _plant

GAP, CLIP = 16, 32
L = align_ref.Locus
rc = align_ref.revcomp


def locus():
    """The locus of the issue's table: the gap cases' first one (150 = 'T', its neighbours differ)."""
    return L("R1*BACKBONE", _plant(_bb(301, 400), 147, "CAGTCTGA"), [])


def hand_cases():
    """[(title, [Locus], reads [(name, seq)], max_edits, gap, clip, expected, (clip searched, gap searched))], expected as
    align_cases.hand_cases(): one entry per read, None (unaligned) or (flag, rname, pos1, mapq, cigar, tags without YT)."""
    cases = []
    loc = locus()
    bb = loc.bb
    j = cc._junk(1, 40)
    x = _not(bb[399])

    # 0 -- overhangs of one base: cost(C) = 1, the gap search is skipped and the record is the clip, not the insertion the gap tier
    #      alone would write (98M1I1M, NM 1, at the right end: the overhanging base equals the backbone's last)
    reads = [("r1", bb[301:400] + bb[399]), ("l1", _not(bb[0]) + bb[0:99])]
    cases.append(("one-base overhangs", [loc], reads, 2, GAP, CLIP, [
        (0, "R1*BACKBONE", 302, 60, "99M1S", "NM:i:0\tMD:Z:99\tNH:i:1"),
        (0, "R1*BACKBONE", 1, 60, "1S99M", "NM:i:0\tMD:Z:99\tNH:i:1")], (2, 0)))

    # 1 -- cost 2: `tie2` hangs over by two bases of which the last equals the backbone's last (97M2I1M costs 2 as well: the tie
    #      goes to the clip); `r2` hangs over by two bases that no gap explains (the gap search runs and finds nothing).  A five-base
    #      overhang: only the clip exists
    reads = [("tie2", bb[302:400] + x + bb[399]), ("r2", bb[302:400] + x + x), ("r5", bb[305:400] + j[:5])]
    cases.append(("overhangs of two and five", [loc], reads, 2, GAP, CLIP, [
        (0, "R1*BACKBONE", 303, 60, "98M2S", "NM:i:0\tMD:Z:98\tNH:i:1"),
        (0, "R1*BACKBONE", 303, 60, "98M2S", "NM:i:0\tMD:Z:98\tNH:i:1"),
        (0, "R1*BACKBONE", 306, 60, "95M5S", "NM:i:0\tMD:Z:95\tNH:i:1")], (3, 3)))

    # 2 -- a novel one-base deletion 3 and 20 bases from the read's right end (the clip statement: clip 1 and 16 plus NM 2), and 40
    #      bases from both ends of an 80-base read (past the clip budget: only the gap exists)
    reads = [("d3", bb[53:150] + bb[151:154]), ("d20", bb[70:150] + bb[151:171]), ("d40", bb[110:150] + bb[151:191])]
    cases.append(("novel deletions", [loc], reads, 2, GAP, CLIP, [
        (0, "R1*BACKBONE", 54, 60, "97M1D3M", "NM:i:1\tMD:Z:97^T3\tNH:i:1"),
        (0, "R1*BACKBONE", 71, 60, "80M1D20M", "NM:i:1\tMD:Z:80^T20\tNH:i:1"),
        (0, "R1*BACKBONE", 111, 60, "40M1D40M", "NM:i:1\tMD:Z:40^T40\tNH:i:1")], (3, 3)))

    # 3 -- a read neither tier aligns (50 backbone bases, 40 foreign ones, 10 from elsewhere), one that aligns end to end, and both
    #      strands of a clipped and of a gapped read
    reads = [("none", bb[100:150] + j[:40] + bb[20:30]), ("e2e", bb[200:300]), ("r1rc", rc(bb[301:400] + bb[399])),
             ("d20rc", rc(bb[70:150] + bb[151:171]))]
    cases.append(("neither, end to end, the other strand", [loc], reads, 2, GAP, CLIP, [
        None,
        (0, "R1*BACKBONE", 201, 60, "100M", "NM:i:0\tMD:Z:100\tNH:i:1"),
        (16, "R1*BACKBONE", 302, 60, "99M1S", "NM:i:0\tMD:Z:99\tNH:i:1"),
        (16, "R1*BACKBONE", 71, 60, "80M1D20M", "NM:i:1\tMD:Z:80^T20\tNH:i:1")], (3, 2)))

    # 4 -- NH 2 on two loci: a part both loci share, with a one-base deletion in the read (gapped) and with a five-base tail that is
    #      foreign to both (clipped: the fewest clipped bases come first in the clip tier's order, so two of the five stay edits)
    shared = _plant(_bb(306, 100), 47, "CAGTCTGA")
    la = L("R6*BACKBONE", _bb(307, 100) + shared + _bb(308, 100), [])
    lb = L("R7*BACKBONE", _bb(309, 50) + shared + _bb(310, 70), [])
    tail = "".join(_not(a, b, c) for a, b, c in zip(la.bb[200:205], lb.bb[150:155], "ACGTA"))
    reads = [("two-g", shared[10:50] + shared[51:91]), ("two-c", shared[20:100] + tail)]
    cases.append(("two loci", [la, lb], reads, 2, GAP, CLIP, [
        (0, "R6*BACKBONE", 111, 1, "40M1D40M", "NM:i:1\tMD:Z:40^T40\tNH:i:2"),
        (0, "R6*BACKBONE", 121, 1, "82M3S", "NM:i:2\tMD:Z:80%s0%s0\tNH:i:2" % (la.bb[200], la.bb[201]))], (2, 2)))
    return cases


N_HAND = 5


def pair_case():
    """(loci, mate-1 records, mate-2 records): mate 1 of `up` hangs three bases over the locus' left end (clipped), its mate 2 carries
    a novel deletion (gapped): the default writes neither, each tier alone writes one of them as UP, both tiers write a CP pair;
    `cp` is concordant either way."""
    bb = _plant(_bb(311, 600), 447, "CAGTCTGA")
    loc = L("R8*BACKBONE", bb, [])
    m1 = [("up", cc._junk(2, 3) + bb[0:97]), ("cp", bb[100:200])]
    m2 = [("up", rc(bb[400:450] + bb[451:501])), ("cp", rc(bb[300:400]))]
    return [loc], m1, m2


def random_case(seed):
    """(loci, reads, max_edits, gap, clip): align_gap_cases.random_case(seed) with six reads added that hang 1 .. 6 bases over an
    end of the first locus (some with a substitution), and a clip budget."""
    loci, reads, me, gap = gc.random_case(seed)
    rng = random.Random(10000 + seed)
    bb = loci[0].bb
    for r in range(6):
        n_r, over = rng.choice([24, 33, 50]), rng.randrange(1, 7)
        junk = align_cases.rand_seq(rng, over)
        s = list(junk + bb[:n_r - over] if rng.random() < 0.5 else bb[len(bb) - (n_r - over):] + junk)
        if rng.random() < 0.4:
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        s = "".join(s)
        reads.append(("o%d" % r, rc(s) if rng.random() < 0.3 else s))
    return loci, reads, me, gap, rng.choice([3, 8, 32])


def choices(loci, reads, me, gap, clip):
    """Per read without an end-to-end alignment: (the rule's choice, "gap first"'s, "clip first"'s), each "clip", "gap" or None --
    from the two tiers' own statements."""
    out = []
    for _, s in reads:
        if align_ref.align_read(loci, s, me) is not None:
            continue
        c, g = align_clip_ref.align_read(loci, s, me, clip), align_gap_ref.align_read(loci, s, me, gap)
        rule = "gap" if rr.gap_wins(c, g) else "clip" if c is not None else None
        out.append((rule, "gap" if g is not None else "clip" if c is not None else None,
                    "clip" if c is not None else "gap" if g is not None else None))
    return out


# seeds of random_case on which the statement writes at least one clipped and one gapped record; on the seeds of NOT_GAP_FIRST a
# record differs from chaining the tiers gap first, on those of NOT_CLIP_FIRST from chaining them clip first (chosen by running the
# statements over 0 .. 47; the test asserts the properties again)
RANDOM_SEEDS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26, 28, 29, 30, 31, 33, 34, 35, 36, 37, 38, 39, 41, 42, 43, 44, 45, 47]
NOT_GAP_FIRST = [0, 1, 4, 5, 6, 8, 10, 13, 15, 16, 17, 20, 21, 23, 24, 25, 26, 28, 29, 30, 31, 33, 34, 35, 36, 37, 41, 42, 45, 47]
NOT_CLIP_FIRST = [0, 1, 3, 4, 6, 7, 10, 11, 13, 15, 16, 17, 19, 20, 21, 22, 23, 24, 26, 28, 29, 30, 31, 33, 34, 35, 36, 37, 38, 39, 41, 42, 44, 45, 47]

_RANDOM = []


def random_cases():
    """[(seed, loci, reads, max_edits, gap, clip, the statement's text, its counters)], computed once per process."""
    if not _RANDOM:
        for seed in RANDOM_SEEDS:
            loci, reads, me, gap, clip = random_case(seed)
            st = {}
            text = rr.align_text(loci, [[(q, s, None) for q, s in reads]], me, gap=gap, clip=clip, stats=st).encode()
            _RANDOM.append((seed, loci, reads, me, gap, clip, text, st))
    return _RANDOM


_INPUTS = {}


def inputs():
    """{id: (dicts, [input texts (bytes)], max_edits, gap, clip)}: the hand cases; the pair in FASTA / FASTQ / gzip, single and
    paired; the gap cases' lengths (17, 33, 100 and 1 024 bases) and the clip cases'; the synth reads with novel indels, the overhang
    tiling, and `mixed`: both over one synth locus."""
    if _INPUTS:
        return _INPUTS
    for k, (title, loci, reads, me, gap, clip, _, _) in enumerate(hand_cases()):
        _INPUTS["rhand%d" % k] = (align_cases.dicts_of(loci), [fasta(reads)], me, gap, clip)
    loci, m1, m2 = pair_case()
    pd = align_cases.dicts_of(loci)
    q1 = [(n, s, align_cases._quals(s, k)) for k, (n, s) in enumerate(m1)]
    q2 = [(n, s, align_cases._quals(s, k + 3)) for k, (n, s) in enumerate(m2)]
    _INPUTS["rpair-fasta"] = (pd, [fasta(m1), fasta(m2)], 2, GAP, CLIP)
    _INPUTS["rpair-fastq-gz"] = (pd, [gzip.compress(fastq(q1)), gzip.compress(fastq(q2))], 2, GAP, CLIP)
    _INPUTS["rsingle-fastq"] = (pd, [fastq(q1 + q2)], 2, GAP, CLIP)
    for key in ("gpair-fasta", "gpair-fastq-gz", "gsingle-fastq", "glengths", "novel-err1"):
        d, texts, me, gap = gc.inputs()[key]
        _INPUTS[key] = (d, texts, me, gap, CLIP)
    for key in ("cpair-fastq-gz", "clengths"):
        d, texts, me, clip = cc.inputs()[key]
        _INPUTS[key] = (d, texts, me, GAP, clip)
    d, texts = mixed(1.0)
    _INPUTS["mixed-err1"] = (d, texts, 2, GAP, CLIP)
    _INPUTS["mixed-single"] = (d, [texts[0] + texts[1]], 2, GAP, CLIP)
    return _INPUTS


def mixed(err_percent, seed=11, step=29):
    """(dicts, [mate-1 text, mate-2 text]): the overhang tiling of align_clip_cases and the novel-indel pairs of align_gap_cases
    over ONE synth locus (both build it from the same seed)."""
    _, d, o1, o2 = cc.overhang_pairs(err_percent, seed=seed, step=step)
    d2, n1, n2 = gc.synth_novel(err_percent, seed=seed, n_pairs=40)
    assert d2[0] == d[0] and d2[1] == d[1]
    return d, [fasta(o1 + n1), fasta(o2 + n2)]


INPUT_IDS = (["rhand%d" % k for k in range(N_HAND)] + ["rpair-fasta", "rpair-fastq-gz", "rsingle-fastq", "gpair-fasta", "gpair-fastq-gz",
                                                       "gsingle-fastq", "glengths", "novel-err1", "cpair-fastq-gz", "clengths", "mixed-err1",
                                                       "mixed-single"])

_REF = {}


def _input(key):
    return inputs()[key] if key in inputs() else align_cases.inputs()[key] + (GAP, CLIP)


def ref_text(key, gap=None, clip=None, stats=None, max_edits=None):
    """The statement's SAM text for inputs()[key] or align_cases.inputs()[key] (bytes), and its counters into `stats`."""
    d, texts, me, g, c = _input(key)
    g, c, me = g if gap is None else gap, c if clip is None else clip, me if max_edits is None else max_edits
    if (key, g, c, me) not in _REF:
        loci = align_ref.loci_from_dicts(d[0], d[1], d[2], d[3])
        st = {}
        text = rr.align_text(loci, [align_ref.read_records(t) for t in texts], me, gap=g, clip=c, stats=st).encode()
        _REF[(key, g, c, me)] = (text, st)
    if stats is not None:
        stats.update(_REF[(key, g, c, me)][1])
    return _REF[(key, g, c, me)][0]


records = gc.records
is_gapped = gc.is_gapped
is_clipped = cc.is_clipped
