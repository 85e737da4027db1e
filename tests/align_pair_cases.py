"""Inputs of the pair-aware placement (tests/align_pair_ref.py): hand-made two-locus families with the records written down from
their construction, and the many-placements construction over align_cases.limit_case("anchors", n)."""
import gzip

import align_cases
import align_pair_ref
import align_ref
from align_cases import _bb, _other

rc = align_ref.revcomp
PERIOD = 39                          # of limit_case("anchors", n): 23 random bases, then the 16-base word


def family(changed=()):
    """P (2 500 bases) and Q (900 bases) with Q[300:600] = P[1000:1300], except at the Q positions in `changed`."""
    p = _bb(61, 2500)
    q = list(_bb(62, 300) + p[1000:1300] + _bb(63, 300))
    for x in changed:
        q[x] = _other(q[x])
    return [align_ref.Locus("P*BACKBONE", p, []), align_ref.Locus("Q*BACKBONE", "".join(q), [])]


def many(n, k=None, both=False):
    """(loci, mate 1, mate 2) on limit_case("anchors", n): mate 1 is the 16-base word that stands n times (copy j at PERIOD * j +
    23); mate 2 is the reverse complement of the 23 unique bases behind copy k - 1 (k = n: the locus' last bases), or with `both`
    of the word itself."""
    loci, reads = align_cases.limit_case("anchors", n)
    k = n if k is None else k
    w, bb = reads[0][1], loci[0].bb
    assert bb[PERIOD * (k - 1) + 23:PERIOD * k] == w
    return loci, w, rc(w if both else bb[PERIOD * k:PERIOD * k + 23])


def hand_cases():
    """[(id, loci, mate-1 reads, mate-2 reads, max_fragment, expected)]: reads [(name, seq)]; expected = one (FLAG, RNAME, POS, NM,
    NH, YT) per written record, in the order of the text."""
    cases = []
    P, Q = "P*BACKBONE", "Q*BACKBONE"
    fam = family()
    p = fam[0].bb
    # mate 1 lies in the stretch both loci hold, its partner 300 bases on is unique: one concordant combination
    cases.append(("ambiguous", fam, [("amb", p[1100:1200])], [("amb", rc(p[1500:1600]))], 1000,
                  [(99, P, 1101, 0, 1, "CP"), (147, P, 1501, 0, 1, "CP")]))
    # one base of Q's copy differs and mate 1 is cut from Q: NM 0 on Q, NM 1 at home, where the pair is concordant
    fam = family(changed=(450,))
    q = fam[1].bb
    cases.append(("rescue", fam, [("res", q[400:500])], [("res", rc(p[1500:1600]))], 1000,
                  [(99, P, 1101, 1, 1, "CP"), (147, P, 1501, 0, 1, "CP")]))
    # the rescuing combination spans [1100, 1600): rescued at max_fragment 500, at 499 the records are the independent ones
    cases.append(("edge-at", fam, [("edge", q[400:500])], [("edge", rc(p[1500:1600]))], 500,
                  [(99, P, 1101, 1, 1, "CP"), (147, P, 1501, 0, 1, "CP")]))
    cases.append(("edge-below", fam, [("edge", q[400:500])], [("edge", rc(p[1500:1600]))], 499,
                  [(97, Q, 401, 0, 1, "DP"), (145, P, 1501, 0, 1, "DP")]))
    # both mates inside the shared stretch: (P, P) and (Q, Q), equal sums: the smaller locus; two (placement, placement) pairs
    fam = family()
    cases.append(("both-ambiguous", fam, [("both", p[1010:1110])], [("both", rc(p[1180:1280]))], 1000,
                  [(99, P, 1011, 0, 2, "CP"), (147, P, 1181, 0, 2, "CP")]))
    # Q differs from P once under each mate; mate 1 is Q's, mate 2 is P's: (P, P) costs 1 + 0, (Q, Q) costs 0 + 1 -- mate 1's key
    # decides, NM 0 first
    fam = family(changed=(350, 550))
    q = fam[1].bb
    cases.append(("1+0-against-0+1", fam, [("tie", q[310:410])], [("tie", rc(p[1190:1290]))], 1000,
                  [(99, Q, 311, 0, 2, "CP"), (147, Q, 491, 1, 2, "CP")]))
    # 30 copies of mate 1's word, mate 2 behind copy 27 (pos0 28 * 39): concordant with copy j iff 39 * (28 - j) <= max_fragment
    loci, w, m2 = many(30, 28)
    R = "R1*BACKBONE"
    cases.append(("many-wide", loci, [("many", w)], [("many", m2)], 1000,
                  [(99, R, PERIOD * 3 + 24, 0, 25, "CP"), (147, R, PERIOD * 28 + 1, 0, 25, "CP")]))
    cases.append(("many-tight", loci, [("many", w)], [("many", m2)], PERIOD,
                  [(99, R, PERIOD * 27 + 24, 0, 1, "CP"), (147, R, PERIOD * 28 + 1, 0, 1, "CP")]))
    return cases


HAND_IDS = ["ambiguous", "rescue", "edge-at", "edge-below", "both-ambiguous", "1+0-against-0+1", "many-wide", "many-tight"]
# hgx_align_last_pairs (searched, placed, changed) of each hand case, counted by hand
HAND_COUNTERS = {"ambiguous": (1, 1, 1), "rescue": (1, 1, 1), "edge-at": (1, 1, 1), "edge-below": (1, 0, 0),
                 "both-ambiguous": (1, 1, 0), "1+0-against-0+1": (1, 1, 1), "many-wide": (1, 1, 1), "many-tight": (1, 1, 1)}


def fields(text):
    """(FLAG, RNAME, POS, NM, NH, YT) of every record of a SAM text."""
    out = []
    for line in (text.decode() if isinstance(text, bytes) else text).split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        tags = dict((t[:2], t[5:]) for t in f[11:])
        out.append((int(f[1]), f[2], int(f[3]), int(tags["NM"]), int(tags["NH"]), tags["YT"]))
    return out


_INPUTS, _REF = {}, {}


def inputs():
    """{id: (dicts, [mate-1 text, mate-2 text] or [one text], max_edits, max_fragment)}: the hand cases in FASTA, the first two also
    in FASTQ and gzip, all of them in one call, a pair with one unaligned mate beside a rescued pair, the word pair whose
    (placement, placement) set is a triangle, and single-end input."""
    if _INPUTS:
        return _INPUTS
    for key, loci, m1, m2, frag, _ in hand_cases():
        _INPUTS[key] = (align_cases.dicts_of(loci), [align_cases.fasta(m1), align_cases.fasta(m2)], 2, frag)
    for key in ("ambiguous", "rescue"):
        d, texts, me, frag = _INPUTS[key]
        recs = [align_ref.read_records(t) for t in texts]
        fq = [align_cases.fastq([(n, s, align_cases._quals(s, 3 + m)) for n, s, _ in r]) for m, r in enumerate(recs)]
        _INPUTS[key + "-fastq"] = (d, fq, me, frag)
        _INPUTS[key + "-fastq-gz"] = (d, [gzip.compress(t) for t in fq], me, frag)
        _INPUTS[key + "-fasta-gz"] = (d, [gzip.compress(t) for t in texts], me, frag)
    # one family, several pairs: rescued, one mate without candidates (either one), ambiguous in Q's changed copy, none aligned
    fam = family(changed=(450,))
    p, q = fam[0].bb, fam[1].bb
    junk = _bb(64, 100)
    m1 = [("r0", q[400:500]), ("h1", junk), ("r1", q[400:500]), ("h2", p[1100:1200]), ("amb", p[1150:1250]), ("no", junk)]
    m2 = [("r0", rc(p[1500:1600])), ("h1", rc(p[1500:1600])), ("r1", rc(p[1700:1800])), ("h2", junk), ("amb", rc(p[1500:1600])),
          ("no", rc(junk))]
    _INPUTS["mixed"] = (align_cases.dicts_of(fam), [align_cases.fasta(m1), align_cases.fasta(m2)], 2, 1000)
    _INPUTS["mixed-single"] = (align_cases.dicts_of(fam), [align_cases.fasta(m1 + [(n + "b", s) for n, s in m2])], 2, 1000)
    loci, w, m2w = many(40, both=True)
    _INPUTS["triangle"] = (align_cases.dicts_of(loci), [align_cases.fasta([("tri", w)]), align_cases.fasta([("tri", m2w)])], 2, 400)
    return _INPUTS


INPUT_IDS = (HAND_IDS + [k + s for k in ("ambiguous", "rescue") for s in ("-fastq", "-fastq-gz", "-fasta-gz")] +
             ["mixed", "mixed-single", "triangle"])


def _parsed(key):
    d, texts, me, frag = inputs()[key]
    return align_ref.loci_from_dicts(*d), [align_ref.read_records(t) for t in texts], me, frag


def ref_text(key):
    """The statement's SAM text with the pair rule for inputs()[key] (bytes), computed once."""
    if key not in _REF:
        loci, reads, me, frag = _parsed(key)
        _REF[key] = align_pair_ref.align_text(loci, reads, me, frag).encode()
    return _REF[key]


PAIRED = (["pairs_two_genes-%d" % n for n in range(3)] + ["single_test_id_and_list-%d" % n for n in range(2)] +
          ["basic_with_errors-%d" % n for n in range(4)] +
          ["synth-err0", "synth-err1", "pairs-fasta", "pairs-fastq", "pairs-fasta-gz", "pairs-fastq-gz", "empty-pair"])
_REF_PAIRED = {}


def ref_text_paired(key):
    """The statement's text with the pair rule for the paired input align_cases.inputs()[key] (max_fragment 1 000), computed once."""
    if key not in _REF_PAIRED:
        d, texts, me = align_cases.inputs()[key]
        loci = align_ref.loci_from_dicts(*d)
        _REF_PAIRED[key] = align_pair_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me).encode()
    return _REF_PAIRED[key]


def ref_counters(key):
    loci, reads, me, frag = _parsed(key)
    return align_pair_ref.counters(loci, reads, me, frag)


def survivors(text):
    """Pairs of a SAM text that pass the typing front end's filter: both records written, NH == 1 and FLAG & 2 on each."""
    by_name = {}
    for line in (text.decode() if isinstance(text, bytes) else text).split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        nh = int([t for t in f[11:] if t.startswith("NH:i:")][0][5:])
        by_name.setdefault(f[0], []).append(nh == 1 and bool(int(f[1]) & 2))
    return sum(len(v) == 2 and all(v) for v in by_name.values())
