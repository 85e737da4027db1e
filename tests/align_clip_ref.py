"""The soft-clip tier of the "hgx" aligner ("Soft clips") as a plain-Python exhaustive search: the yardstick of
the host route and of the kernels with hgx_align_opts.clip > 0.  It imports tests/align_ref.py and changes nothing in it.

A read that has an end-to-end alignment (align_ref.align_read) is searched and written exactly as there.  Only a read that has
none may be written with up to `clip` bases soft-clipped in total, by these two additions to the walk:

    right side   at every state (r, p) with r < L there is one more option: stop here.  The L - r remaining bases are clipped and
                 the backbone end is p.  The option exists on ENTRY to a state only (before its known indels), so a way never
                 ends in a known indel; a state with p == len(bb) has this option only (the overhang).
    left side    at every "base r sits on q" with r > 0 there is one more option: the bases < r are clipped and pos0 = q.  No
                 known indel is taken in front of the first aligned base.

An alignment is admissible through an anchor if the anchor's 16 bases are plain matches, NM <= max_edits over the aligned part and
clipL + clipR <= clip.  The order within the tier is (clipL + clipR, NM, indels, variants, locus, strand, pos0, list), and last
clipL: two different anchors of a read in a repeat can reach alignments that tie in all of the former (one more base clipped on
the left, one fewer on the right), and the record needs one of them.  NH counts the placements of the canon(a) that share the
smallest (clip total, NM), by pos0 / end of the aligned parts.

A side's entries with more than `clip` clipped bases or more than max_edits edits are dropped where they arise, which loses no
admissible alignment; nothing else is cut (the enumeration is exhaustive, prune=False semantics: there is no shortcut form).
"""
import align_ref
from align_ref import K, revcomp, seed_offsets


class _ClipSearch(align_ref._Search):
    """All alignments of one oriented read at one locus with up to `clip` clipped bases.
    right(): [(clipR, NM, indels, variants, backbone end)]; left(): [(clipL, NM, indels, pos0, variants)]."""

    def __init__(self, loc, s, max_edits, clip):
        align_ref._Search.__init__(self, loc, s, max_edits, False)
        self.clip = clip

    def right(self, r, p):
        key = (r, p)
        if key in self._right:
            return self._right[key]
        loc, out = self.loc, []
        if r == self.L:
            out.append((0, 0, 0, (), p))
        else:
            if self.L - r <= self.clip:
                out.append((self.L - r, 0, 0, (), p))                 # stop here
            if p < len(loc.bb):
                dels, inss = loc.del_start.get(p, []), loc.ins.get(p, [])
                options = [()] + [(d,) for d in dels] + [(i,) for i in inss]
                options += [(i, d) for d in dels for i in inss]
                for ev in options:
                    rr, pp, ok = r, p, True
                    for v in ev:
                        if loc.variants[v][0] == "deletion":
                            pp += int(loc.variants[v][2])
                        else:
                            n = self.ins_fits(v, rr)
                            if n < 0:
                                ok = False
                                break
                            rr += n
                    if not ok:
                        continue
                    if rr >= self.L:                                  # the insertion ran into the read's right end
                        out.append((0, 0, len(ev), ev, pp))
                        continue
                    if pp >= len(loc.bb):
                        continue
                    nm, single = self.base(rr, pp)
                    for c2, nm2, ni2, vl2, end in self.right(rr + 1, pp + 1):
                        if nm + nm2 <= self.max_edits:
                            out.append((c2, nm + nm2, len(ev) + ni2, ev + single + vl2, end))
        self._right[key] = out
        return out

    def left(self, r, q):
        key = (r, q)
        if key in self._left:
            return self._left[key]
        loc, out = self.loc, []
        if r == 0:
            out.append((0, 0, 0, q, ()))
        else:
            if r <= self.clip:
                out.append((r, 0, 0, q, ()))                          # the bases < r are clipped
            arrivals = [((), r, q)]
            for d in loc.del_end.get(q, []):
                p1 = loc.variants[d][1]
                arrivals.append(((d,), r, p1))
                for i in loc.ins.get(p1, []):
                    n = len(loc.variants[i][2])
                    if r - n >= 1 and self.ins_fits(i, r - n) == n:
                        arrivals.append(((i, d), r - n, p1))
            for i in loc.ins.get(q, []):
                n = len(loc.variants[i][2])
                if r - n >= 1 and self.ins_fits(i, r - n) == n:
                    arrivals.append(((i,), r - n, q))
            for ev, r1, p1 in arrivals:
                if p1 - 1 < 0:
                    continue
                nm, single = self.base(r1 - 1, p1 - 1)
                for c2, nm2, ni2, pos0, vl2 in self.left(r1 - 1, p1 - 1):
                    if nm + nm2 <= self.max_edits:
                        out.append((c2, nm + nm2, len(ev) + ni2, pos0, vl2 + single + ev))
        self._left[key] = out
        return out

    def canon(self, o, b):
        """The smallest alignment admissible through the anchor, or None: ((clip total, NM, indels, variants, pos0, list, clipL), end)."""
        best = None
        for c1, nm1, ni1, pos0, vl1 in self.left(o, b):
            for c2, nm2, ni2, vl2, end in self.right(o + K, b + K):
                if nm1 + nm2 > self.max_edits or c1 + c2 > self.clip:
                    continue
                vl = vl1 + vl2
                cand = ((c1 + c2, nm1 + nm2, ni1 + ni2, len(vl), pos0, vl, c1), end)
                if best is None or cand[0] < best[0]:
                    best = cand
        return best


def has_anchor(loci, seq):
    seq = seq.upper()
    for s in (seq, revcomp(seq)):
        for o in seed_offsets(len(s)):
            if any(s[o:o + K] in loc.kmers for loc in loci):
                return True
    return False


def align_read(loci, seq, max_edits, clip):
    """None, or (key, end, NH, clipL, clipR) with key = (NM, indels, variants, locus, strand, pos0, list) as align_ref's."""
    a = align_ref.align_read(loci, seq, max_edits)
    if a is not None:
        return a + (0, 0)
    if clip <= 0:
        return None
    seq = seq.upper()
    canons = {}
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        for g, loc in enumerate(loci):
            search = _ClipSearch(loc, s, max_edits, clip)
            for o in seed_offsets(len(s)):
                for b in loc.kmers.get(s[o:o + K], []):
                    c = search.canon(o, b)
                    if c is not None:
                        (ct, nm, ni, nv, pos0, vl, cl), end = c
                        canons[(ct, nm, ni, nv, g, strand, pos0, vl, cl)] = end
    if not canons:
        return None
    best = min(canons)
    R = sorted((k[4], k[5], k[6], end) for k, end in canons.items() if k[:2] == best[:2])
    nh, cur = 0, None
    for g, strand, pos0, end in R:
        if cur is None or cur[0] != (g, strand) or pos0 >= cur[1]:
            nh += 1
            cur = [(g, strand), end]
        else:
            cur[1] = max(cur[1], end)
    return best[1:8], canons[best], nh, best[8], best[0] - best[8]


def align_text(loci, reads, max_edits=2, max_fragment=1000, clip=0, stats=None):
    """The SAM text for `reads` (as align_ref.align_text).  `stats`, a dict, receives searched / clipped / bases as
    hgx_align_last_clip counts them: reads without an end-to-end alignment that have an anchor, reads written with a clip, bases
    clipped."""
    paired = len(reads) == 2
    lines = ["@SQ\tSN:%s\tLN:%d" % (loc.name, len(loc.bb)) for loc in loci]
    searched = clipped = bases = 0
    for k in range(len(reads[0])):
        alns = []
        for m in range(len(reads)):
            qname, seq, qual = reads[m][k]
            a = align_read(loci, seq, max_edits, clip)
            if clip > 0 and (a is None or a[3] + a[4] > 0) and has_anchor(loci, seq):
                searched += 1
            if a is not None and a[3] + a[4] > 0:
                clipped += 1
                bases += a[3] + a[4]
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
            key, end, nh, cl, cr = a
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
            # the aligned part alone is rendered (its first base is "base 0" of the walk: no indel in front of it, the first Zs gap
            # counts from it); the clips go around its CIGAR
            cigar, md, zs = align_ref.render(loc, s[cl:len(s) - cr], pos0, vl)
            cigar = ("%dS" % cl if cl else "") + cigar + ("%dS" % cr if cr else "")
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:%d" % nh, "YT:Z:%s" % yt]
            lines.append("\t".join([qname, str(flag), loc.name, str(pos0 + 1), "60" if nh == 1 else "1", cigar, rnext, str(pnext),
                                    "0", s, q] + tags))
    if stats is not None:
        stats.update(searched=searched, clipped=clipped, bases=bases)
    return "\n".join(lines) + "\n"
