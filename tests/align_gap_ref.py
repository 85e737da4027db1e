"""The novel-gap tier of the "hgx" aligner ("Novel gaps") as a plain-Python exhaustive search: the yardstick of
the host route and of the kernels with gap > 0 (hgx_align_more.gap).  It imports tests/align_ref.py and changes nothing in it.

A read that has an end-to-end alignment (align_ref.align_read) is searched and written exactly as there.  Only a read that has
none may be written with ONE novel gap, by this addition to the walk of align_ref:

    on ENTRY to a state (r, p) with 0 < r < L, before the state's known indels, while no novel gap has been taken:
      * a novel deletion of d = 1 .. gap bases leads to the state (r, p + d)
      * a novel insertion of i = 1 .. gap bases leads to the state (r + i, p), and needs r + i < L
    the state reached is entered like any other (its known indels may follow; a second novel gap may not)

so a base follows the gap on both sides.  The left side has the mirror arrivals: the state (r1, p1) from which known events lead to
"base r sits on q" may itself have been reached by a deletion from (r1, p1 - d) or by an insertion from (r1 - i, p1), r1 - i >= 1.
A gap of g bases adds g to NM; admissible means NM <= max_edits with the gap counted.  Through an anchor (o, b) the anchor's 16
bases are plain matches, so the gap lies at r <= o (left side) or r >= o + 16 (right side).

The order within the tier is align_ref's key (NM, known indels, variants, locus, strand, pos0, list) and last the gap descriptor
(read offset of the gap, kind: deletion 0 before insertion 1, length): in a homopolymer or a repeat the leftmost placement of the
gap is the record.  The novel gap does not count into `indels`.  NH counts the placements of the canon(a) that share the smallest
NM, by pos0 / end.  Nothing is cut but entries over the edit budget (the enumeration is exhaustive, prune=False semantics).
"""
import align_ref
from align_ref import K, revcomp, seed_offsets

GAP_MAX = 16
DEL, INS = 0, 1


class _GapSearch(align_ref._Search):
    """All alignments of one oriented read at one locus with exactly one novel gap of up to `gap` bases.
    right_gap(): [(NM, indels, variants, backbone end, descriptor)]; left_gap(): [(NM, indels, pos0, variants, descriptor)]."""

    def __init__(self, loc, s, max_edits, gap):
        align_ref._Search.__init__(self, loc, s, max_edits, False)
        self.gap = min(gap, max_edits)                              # a longer gap alone passes the edit budget
        self._rg, self._lg = {}, {}

    def right_gap(self, r, p):
        key = (r, p)
        if key in self._rg:
            return self._rg[key]
        loc, out = self.loc, []
        if 0 < r < self.L:
            for d in range(1, self.gap + 1):                          # the gap on entry to this state
                for nm2, ni2, vl2, end in self.right(r, p + d):
                    if d + nm2 <= self.max_edits:
                        out.append((d + nm2, ni2, vl2, end, (r, DEL, d)))
            for i in range(1, self.gap + 1):
                if r + i < self.L:
                    for nm2, ni2, vl2, end in self.right(r + i, p):
                        if i + nm2 <= self.max_edits:
                            out.append((i + nm2, ni2, vl2, end, (r, INS, i)))
        if r < self.L and p < len(loc.bb):                            # the gap behind this state's base: the step of align_ref
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
                if not ok or rr >= self.L or pp >= len(loc.bb):
                    continue
                nm, single = self.base(rr, pp)
                for nm2, ni2, vl2, end, gd in self.right_gap(rr + 1, pp + 1):
                    if nm + nm2 <= self.max_edits:
                        out.append((nm + nm2, len(ev) + ni2, ev + single + vl2, end, gd))
        self._rg[key] = out
        return out

    def left_gap(self, r, q):
        key = (r, q)
        if key in self._lg:
            return self._lg[key]
        loc, out = self.loc, []
        if r > 0:
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
                # the state (r1, p1) was reached by the gap: from (r1, p1 - g) or from (r1 - g, p1), entered from the base in front
                pre = [(r1, p1 - g, (r1, DEL, g)) for g in range(1, self.gap + 1)]
                pre += [(r1 - g, p1, (r1 - g, INS, g)) for g in range(1, self.gap + 1) if r1 - g >= 1]
                for rg, pg, gd in pre:
                    if pg - 1 < 0:
                        continue
                    nm, single = self.base(rg - 1, pg - 1)
                    for nm2, ni2, pos0, vl2 in self.left(rg - 1, pg - 1):
                        if gd[2] + nm + nm2 <= self.max_edits:
                            out.append((gd[2] + nm + nm2, len(ev) + ni2, pos0, vl2 + single + ev, gd))
                # the gap further left
                if p1 - 1 < 0:
                    continue
                nm, single = self.base(r1 - 1, p1 - 1)
                for nm2, ni2, pos0, vl2, gd in self.left_gap(r1 - 1, p1 - 1):
                    if nm + nm2 <= self.max_edits:
                        out.append((nm + nm2, len(ev) + ni2, pos0, vl2 + single + ev, gd))
        self._lg[key] = out
        return out

    def canon(self, o, b):
        """The smallest alignment with one gap admissible through the anchor, or None: ((NM, indels, variants, pos0, list, descriptor), end)."""
        best = None
        for left, right in ((self.left_gap(o, b), self.right(o + K, b + K)), (self.left(o, b), self.right_gap(o + K, b + K))):
            for x in left:
                for y in right:
                    if x[0] + y[0] > self.max_edits:
                        continue
                    vl = x[3] + y[2]
                    gd = x[4] if len(x) == 5 else y[4]
                    cand = ((x[0] + y[0], x[1] + y[1], len(vl), x[2], vl, gd), y[3])
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


def align_read(loci, seq, max_edits, gap):
    """None, or (key, end, NH, descriptor) with key = (NM, indels, variants, locus, strand, pos0, list) as align_ref's and
    descriptor = None (end to end) or (read offset, kind, length) of the novel gap in the oriented read."""
    a = align_ref.align_read(loci, seq, max_edits)
    if a is not None:
        return a + (None,)
    if gap <= 0:
        return None
    seq = seq.upper()
    canons = {}
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        for g, loc in enumerate(loci):
            search = _GapSearch(loc, s, max_edits, gap)
            for o in seed_offsets(len(s)):
                for b in loc.kmers.get(s[o:o + K], []):
                    c = search.canon(o, b)
                    if c is not None:
                        (nm, ni, nv, pos0, vl, gd), end = c
                        canons[(nm, ni, nv, g, strand, pos0, vl, gd)] = end
    if not canons:
        return None
    best = min(canons)
    R = sorted((k[3], k[4], k[5], end) for k, end in canons.items() if k[0] == best[0])
    nh, cur = 0, None
    for g, strand, pos0, end in R:
        if cur is None or cur[0] != (g, strand) or pos0 >= cur[1]:
            nh += 1
            cur = [(g, strand), end]
        else:
            cur[1] = max(cur[1], end)
    return best[:7], canons[best], nh, best[7]


def render(loc, s, pos0, vl, gd):
    """(CIGAR, MD, Zs) of the walk with the novel gap `gd`, in the form simulate's synth._align_read writes: I / D in the CIGAR,
    ^bases in MD for the deletion (the 0 between adjacent non-match items kept), nothing in MD for the insertion, no Zs item for
    the gap; inserted bases count into the next Zs item's gap, deleted bases do not."""
    events, singles = {}, {}
    for v in vl:
        t, p, d, vid = loc.variants[v]
        if t == "single":
            singles[p] = vid
        else:
            events.setdefault(p, []).append((t, d, vid))
    bb = loc.bb
    cigar, md, zs = [], [], []
    md_run = gap = 0
    r, p = 0, pos0
    g_r, g_kind, g_len = gd

    def push(op, n):
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += n
        else:
            cigar.append([op, n])

    while r < len(s):
        if r == g_r:                                                  # on entry, before the known indels of the state reached
            g_r = -1
            if g_kind == DEL:
                md.append("%d^%s" % (md_run, bb[p:p + g_len]))
                md_run = 0
                push("D", g_len)
                p += g_len
            else:
                push("I", g_len)
                gap += g_len
                r += g_len
        for t, d, vid in events.pop(p, []) if r > 0 else []:
            if t == "deletion":
                n = int(d)
                md.append("%d^%s" % (md_run, bb[p:p + n]))
                md_run = 0
                push("D", n)
                zs.append("%d|D|%s" % (gap, vid))
                gap = 0
                p += n
            else:
                n = min(len(d), len(s) - r)
                zs.append("%d|I|%s" % (gap, vid))
                gap = n
                push("I", n)
                r += n
        if r >= len(s):
            break
        if s[r] == bb[p]:
            md_run += 1
            gap += 1
        else:
            md.append("%d%s" % (md_run, bb[p]))
            md_run = 0
            if p in singles:
                zs.append("%d|S|%s" % (gap, singles[p]))
                gap = 0
            else:
                gap += 1
        push("M", 1)
        r += 1
        p += 1
    md.append("%d" % md_run)
    return "".join("%d%s" % (n, op) for op, n in cigar), "".join(md), ",".join(zs)


def align_text(loci, reads, max_edits=2, max_fragment=1000, gap=0, stats=None):
    """The SAM text for `reads` (as align_ref.align_text).  `stats`, a dict, receives searched / gapped / bases as
    hgx_align_last_gap counts them: reads without an end-to-end alignment that have an anchor, reads written with a gap, gap
    bases."""
    paired = len(reads) == 2
    lines = ["@SQ\tSN:%s\tLN:%d" % (loc.name, len(loc.bb)) for loc in loci]
    searched = gapped = bases = 0
    for k in range(len(reads[0])):
        alns = []
        for m in range(len(reads)):
            qname, seq, qual = reads[m][k]
            a = align_read(loci, seq, max_edits, gap)
            if gap > 0 and (a is None or a[3] is not None) and has_anchor(loci, seq):
                searched += 1
            if a is not None and a[3] is not None:
                gapped += 1
                bases += a[3][2]
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
            key, end, nh, gd = a
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
            cigar, md, zs = align_ref.render(loc, s, pos0, vl) if gd is None else render(loc, s, pos0, vl, gd)
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:%d" % nh, "YT:Z:%s" % yt]
            lines.append("\t".join([qname, str(flag), loc.name, str(pos0 + 1), "60" if nh == 1 else "1", cigar, rnext, str(pnext),
                                    "0", s, q] + tags))
    if stats is not None:
        stats.update(searched=searched, gapped=gapped, bases=bases)
    return "\n".join(lines) + "\n"
