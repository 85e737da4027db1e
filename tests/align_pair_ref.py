"""Pair-aware placement of the "hgx" aligner (hgx_align_opts.pair = 1) as plain Python over tests/align_ref.py: the
yardstick of the host route's pair pick (csrc/hgx_align_host.cpp) and of k_aln_pair_pick (csrc/hgx_align.hip).  Clarity over speed.

A mate's CANDIDATES are the distinct canon(a) over its anchors (the dict `canons` of align_ref.align_read): key = (NM, indels,
variants, locus, strand, pos0, list) -> end.  A COMBINATION (c1, c2) is one candidate per mate; it is concordant by align_text's
test.  If a concordant combination exists both records are written from the smallest one by (NM1 + NM2, indels1 + indels2,
variants1 + variants2, key of c1, key of c2), as a concordant pair, and NH (the same on both) counts the distinct (placement of c1,
placement of c2) over the concordant combinations of the smallest NM sum, the placements being align_read's clusters of the
candidates those combinations use.  Otherwise, and for single-end input, every record is align_ref.align_text's."""
import align_ref
from align_ref import K, revcomp, render, seed_offsets


def candidates(loci, seq, max_edits, prune=False):
    """{key: end} -- align_ref.align_read's `canons`."""
    seq = seq.upper()
    canons = {}
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        for g, loc in enumerate(loci):
            search = align_ref._Search(loc, s, max_edits, prune)
            for o in seed_offsets(len(s)):
                for b in loc.kmers.get(s[o:o + K], []):
                    c = search.canon(o, b)
                    if c is not None:
                        (nm, ni, nv, pos0, vl), end = c
                        canons[(nm, ni, nv, g, strand, pos0, vl)] = end
    return canons


def placements(cands):
    """{key: placement number} of `cands` = {key: end}, by align_read's rule: sorted by (locus, strand, pos0), a new placement
    starts where the locus or strand changes or pos0 is not below the largest end seen."""
    out, n, cur = {}, -1, None
    for key in sorted(cands, key=lambda k: (k[3], k[4], k[5], cands[k])):
        end = cands[key]
        if cur is None or cur[0] != (key[3], key[4]) or key[5] >= cur[1]:
            n += 1
            cur = [(key[3], key[4]), end]
        else:
            cur[1] = max(cur[1], end)
        out[key] = n
    return out


def independent(canons):
    """None, or (key, end, NH): align_read's answer from its candidates."""
    if not canons:
        return None
    best = min(canons)
    least = {k: e for k, e in canons.items() if k[0] == best[0]}
    return best, canons[best], len(set(placements(least).values()))


def concordant(k0, e0, k1, e1, max_fragment):
    if k0[3] != k1[3] or k0[4] == k1[4]:
        return False
    plus, minus = (k0, k1) if k0[4] == 0 else (k1, k0)
    return plus[5] <= minus[5] and max(e0, e1) - min(k0[5], k1[5]) <= max_fragment


def pair_pick(c1, c2, max_fragment):
    """None (no concordant combination), or ((key1, end1), (key2, end2), NH) of the pair's alignment."""
    combos = [(a, b) for a in c1 for b in c2 if concordant(a, c1[a], b, c2[b], max_fragment)]
    if not combos:
        return None
    a, b = min(combos, key=lambda ab: (ab[0][0] + ab[1][0], ab[0][1] + ab[1][1], ab[0][2] + ab[1][2], ab[0], ab[1]))
    nm = a[0] + b[0]
    least = [(x, y) for x, y in combos if x[0] + y[0] == nm]
    p1 = placements({x: c1[x] for x, _ in least})
    p2 = placements({y: c2[y] for _, y in least})
    return (a, c1[a]), (b, c2[b]), len({(p1[x], p2[y]) for x, y in least})


def align_pairs(loci, reads, max_edits=2, max_fragment=1000, prune=False):
    """Per pair ((a0, a1), placed) with a_m = None or (key, end, NH) of mate m's record and placed = a concordant combination
    exists; for single-end input ((a0,), False)."""
    out = []
    for k in range(len(reads[0])):
        cands = [candidates(loci, reads[m][k][1], max_edits, prune) for m in range(len(reads))]
        alns = [independent(c) for c in cands]
        placed = False
        if len(reads) == 2 and cands[0] and cands[1]:
            pick = pair_pick(cands[0], cands[1], max_fragment)
            if pick is not None:
                (a, ea), (b, eb), nh = pick
                alns, placed = [(a, ea, nh), (b, eb, nh)], True
        out.append((tuple(alns), placed))
    return out


def counters(loci, reads, max_edits=2, max_fragment=1000, prune=False):
    """(searched, placed, changed) as hgx_align_last_pairs counts them."""
    if len(reads) != 2:
        return 0, 0, 0
    searched = placed = changed = 0
    for k, (alns, pl) in enumerate(align_pairs(loci, reads, max_edits, max_fragment, prune)):
        ind = [align_ref.align_read(loci, reads[m][k][1], max_edits, prune) for m in range(2)]
        searched += ind[0] is not None and ind[1] is not None
        placed += pl
        changed += pl and list(alns) != ind
    return searched, placed, changed


def align_text(loci, reads, max_edits=2, max_fragment=1000, prune=False):
    """The SAM text with pair = 1; the lines are written as align_ref.align_text writes them."""
    paired = len(reads) == 2
    lines = ["@SQ\tSN:%s\tLN:%d" % (loc.name, len(loc.bb)) for loc in loci]
    for k, (alns, _) in enumerate(align_pairs(loci, reads, max_edits, max_fragment, prune)):
        conc = paired and alns[0] is not None and alns[1] is not None and concordant(
            alns[0][0], alns[0][1], alns[1][0], alns[1][1], max_fragment)
        for m, a in enumerate(alns):
            if a is None:
                continue
            qname, seq, qual = reads[m][k]
            seq = seq.upper()
            key, end, nh = a
            nm, _, _, g, strand, pos0, vl = key
            loc = loci[g]
            s = seq if strand == 0 else revcomp(seq)
            q = ("I" * len(s)) if qual is None else (qual if strand == 0 else qual[::-1])
            flag = 16 if strand else 0
            rnext, pnext, yt = "*", 0, "UU"
            if paired:
                flag |= 1 | (0x40 if m == 0 else 0x80)
                mate = alns[1 - m]
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
            cigar, md, zs = render(loc, s, pos0, vl)
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:%d" % nh, "YT:Z:%s" % yt]
            lines.append("\t".join([qname, str(flag), loc.name, str(pos0 + 1), "60" if nh == 1 else "1", cigar, rnext, str(pnext),
                                    "0", s, q] + tags))
    return "\n".join(lines) + "\n"
