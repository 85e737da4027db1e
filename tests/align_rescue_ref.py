"""Both fallback tiers of the "hgx" aligner in one call ("Both tiers") as plain Python: the yardstick of the host
route and of the kernels with hgx_align_more.rescue_clip > 0 (AlignIndex.align(rescue=(gap, clip)), aligner name "hgx.rescue").
It imports tests/align_ref.py, tests/align_gap_ref.py and tests/align_clip_ref.py and changes nothing in them.

A read that has an end-to-end alignment (align_ref.align_read) is searched and written exactly as there, NH included.  A read
that has none gets

    C = align_clip_ref.align_read(loci, seq, max_edits, clip)    clipL, clipR, NM_c          cost(C) = clipL + clipR + NM_c
    G = align_gap_ref.align_read(loci, seq, max_edits, gap)      NM_g, the gap counted      cost(G) = NM_g

the number of read bases given up or edited.  The record is G if G exists and (C does not exist or NM_g < cost(C)); otherwise C,
if C exists; otherwise the read is unaligned.  A tie goes to the clip: it claims no variant.  Each tier keeps its own internal
order, pick and NH, and the record is rendered exactly as that tier's statement renders it; a read never carries both a clip and
a novel gap.  Mate fields and concordance come from the two mates' final alignments, whichever tier each came from, by pos0 / end
of the aligned parts.

NM_g >= 1, so a read with cost(C) <= 1 never needs the gap search: it is skipped there, and that is what the gap tier's
`searched` counts.
"""
import align_clip_ref
import align_gap_ref
import align_ref
from align_ref import revcomp

NONE = 1 << 30                       # the cost of a result that does not exist


def cost_clip(c):
    return NONE if c is None else c[3] + c[4] + c[0][0]


def cost_gap(g):
    return NONE if g is None else g[0][0]


def gap_wins(c, g):
    """The rule: the gap statement's result `g` against the clip statement's `c` (either may be None)."""
    return g is not None and cost_gap(g) < cost_clip(c)


def align_read(loci, seq, max_edits, gap, clip, searched=None):
    """None, or (key, end, NH, clipL, clipR, descriptor) with key = (NM, indels, variants, locus, strand, pos0, list) as
    align_ref's, clipL = clipR = 0 unless the clip tier wrote the record, descriptor = None unless the gap tier did.  `searched`,
    a list, receives "clip" / "gap" for each tier's search that ran."""
    a = align_ref.align_read(loci, seq, max_edits)
    if a is not None:
        return a + (0, 0, None)
    c = align_clip_ref.align_read(loci, seq, max_edits, clip)
    if searched is not None:
        searched.append("clip")
    g = None
    if cost_clip(c) >= 2:
        g = align_gap_ref.align_read(loci, seq, max_edits, gap)
        if searched is not None:
            searched.append("gap")
    if gap_wins(c, g):
        return g[:3] + (0, 0, g[3])
    if c is not None:
        return c + (None,)
    return None


def align_text(loci, reads, max_edits=2, max_fragment=1000, gap=0, clip=0, stats=None):
    """The SAM text for `reads` (as align_ref.align_text).  `stats`, a dict, receives clip = dict(searched, clipped, bases) and
    gap = dict(searched, gapped, bases) as hgx_align_last_clip and hgx_align_last_gap count them: reads without an end-to-end
    alignment that have an anchor, and of those the reads the clip statement left unaligned or with a cost of 2 or more; reads
    written with a clip / a gap; bases clipped / gap bases."""
    paired = len(reads) == 2
    lines = ["@SQ\tSN:%s\tLN:%d" % (loc.name, len(loc.bb)) for loc in loci]
    cs = dict(searched=0, clipped=0, bases=0)
    gs = dict(searched=0, gapped=0, bases=0)
    for k in range(len(reads[0])):
        alns = []
        for m in range(len(reads)):
            qname, seq, qual = reads[m][k]
            ran = []
            a = align_read(loci, seq, max_edits, gap, clip, ran)
            if ran and align_clip_ref.has_anchor(loci, seq):
                cs["searched"] += 1
                gs["searched"] += "gap" in ran
            if a is not None and a[3] + a[4] > 0:
                cs["clipped"] += 1
                cs["bases"] += a[3] + a[4]
            if a is not None and a[5] is not None:
                gs["gapped"] += 1
                gs["bases"] += a[5][2]
            alns.append((qname, seq.upper(), qual, a))
        conc = False
        if paired and alns[0][3] is not None and alns[1][3] is not None:
            (k0, e0), (k1, e1) = alns[0][3][:2], alns[1][3][:2]
            if k0[3] == k1[3] and k0[4] != k1[4]:
                plus, minus = (k0, k1) if k0[4] == 0 else (k1, k0)
                conc = plus[5] <= minus[5] and max(e0, e1) - min(k0[5], k1[5]) <= max_fragment
        for m, (qname, seq, qual, a) in enumerate(alns):
            if a is None:
                continue
            key, end, nh, cl, cr, gd = a
            nm, _, _, g, strand, pos0, vl = key
            loc = loci[g]
            s = seq if strand == 0 else revcomp(seq)
            q = ("I" * len(s)) if qual is None else (qual if strand == 0 else qual[::-1])
            flag = 16 if strand else 0
            rnext, pnext, yt = "*", 0, "UU"
            if paired:
                flag |= 1 | (0x40 if m == 0 else 0x80)
                mate = alns[1 - m][3]
                if mate is None:
                    flag |= 8
                    rnext, pnext, yt = "=", pos0 + 1, "UP"
                else:
                    mk = mate[0]
                    flag |= 0x20 if mk[4] else 0
                    rnext, pnext = ("=" if mk[3] == g else loci[mk[3]].name), mk[5] + 1
                    yt = "CP" if conc else "DP"
                    if conc:
                        flag |= 2
            if gd is not None:                                        # as align_gap_ref.align_text renders it
                cigar, md, zs = align_gap_ref.render(loc, s, pos0, vl, gd)
            else:                                                     # as align_clip_ref.align_text does (cl = cr = 0: align_ref's)
                cigar, md, zs = align_ref.render(loc, s[cl:len(s) - cr], pos0, vl)
                cigar = ("%dS" % cl if cl else "") + cigar + ("%dS" % cr if cr else "")
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:%d" % nh, "YT:Z:%s" % yt]
            lines.append("\t".join([qname, str(flag), loc.name, str(pos0 + 1), "60" if nh == 1 else "1", cigar, rnext, str(pnext),
                                    "0", s, q] + tags))
    if stats is not None:
        stats.update(clip=cs, gap=gs)
    return "\n".join(lines) + "\n"
