"""The rules of the "hgx" aligner as a plain-Python exhaustive search: the yardstick of the host route
(csrc/hgx_align_host.cpp) and of the kernels (csrc/hgx_align.hip).  Clarity over speed; nothing here is shared with them.

An alignment of an oriented read `s` at a locus is a start `pos0` plus an ordered list of known variants (indices into the
locus' Var_list).  The walk of simulate._truth_record consumes `s` with them:

    state (r, p): read base r is next, backbone position p is next
      * with r > 0, known indels that START at p may be taken first -- at most one insertion and one deletion per state, the
        insertion first (so that both sit at their database position in the record): a deletion skips int(data) backbone bases; an insertion needs s[r:r+n] == data[:n] with
        n = min(len(data), L - r) and consumes those n read bases (cut off by the read's right end: allowed, and the walk ends)
      * then s[r] sits on the backbone base at p: equal = match; different and equal to the data of a known single at p =
        that single (the first in Var_list order), free; otherwise one unknown edit (NM)

so the singles of an alignment follow from its indels; the search is over pos0 and the indels only.
"""
import gzip
import sys

K = 16
STRIDE = 4
ACGT = frozenset("ACGT")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))


def revcomp(s):
    return "".join(_COMP.get(b, b) for b in reversed(s))


class Locus:
    """name = the backbone's reference name, bb = backbone (upper case), variants = [(type, pos, data, id)] in Var_list order."""

    def __init__(self, name, bb, variants):
        self.name, self.bb, self.variants = name, bb.upper(), [tuple(v) for v in variants]
        self.singles, self.del_start, self.del_end, self.ins = {}, {}, {}, {}
        for i, (t, p, d, _) in enumerate(self.variants):
            if t == "single":
                self.singles.setdefault(p, []).append(i)
            elif t == "deletion":
                self.del_start.setdefault(p, []).append(i)
                self.del_end.setdefault(p + int(d), []).append(i)
            else:
                assert t == "insertion"
                self.ins.setdefault(p, []).append(i)
        self.kmers = {}
        for p in range(len(self.bb) - K + 1):
            w = self.bb[p:p + K]
            if set(w) <= ACGT:
                self.kmers.setdefault(w, []).append(p)


def loci_from_dicts(Genes, Vars, Var_list, refGenes):
    """Loci in the order of `Genes`, variants in Var_list order."""
    out = []
    for g in Genes:
        gv = Vars.get(g, {})
        out.append(Locus(refGenes[g], Genes[g][refGenes[g]], [tuple(gv[vid]) + (vid,) for _, vid in Var_list.get(g, [])]))
    return out


def seed_offsets(L):
    if L < K:
        return []
    return sorted(set(list(range(0, L - K + 1, STRIDE)) + [L - K]))


class _Search:
    """All alignments of one oriented read at one locus, by exhaustive enumeration left and right of an anchor (memoised per
    state; a side whose own NM exceeds max_edits is dropped, which loses no admissible alignment).

    prune=True keeps only the smallest entry of every state's list.  The first three components of the order are sums over the
    steps, lists of equal cost have equal length, and pos0 belongs to the far end of the left side, so the smallest way through a
    state continues the smallest way from it: the result is the same (tests/test_align_ref.py compares the two on every input),
    and a tandem repeat with many known unit indels, where the number of WAYS is exponential, stays polynomial."""

    def __init__(self, loc, s, max_edits, prune=False):
        self.loc, self.s, self.L, self.max_edits, self.prune = loc, s, len(s), max_edits, prune
        self._right, self._left = {}, {}

    def base(self, r, p):
        """(NM, variants) of read base r on backbone base p."""
        c, loc = self.s[r], self.loc
        if c == loc.bb[p]:
            return 0, ()
        if c in ACGT:
            for i in loc.singles.get(p, []):
                if loc.variants[i][2] == c:
                    return 0, (i,)
        return 1, ()

    def ins_fits(self, i, r):
        d = self.loc.variants[i][2].upper()
        n = min(len(d), self.L - r)
        return n if self.s[r:r + n] == d[:n] else -1

    def right(self, r, p):
        """Every way to finish from state (r, p), r > 0: [(NM, indels, variants, backbone end)]."""
        key = (r, p)
        if key in self._right:
            return self._right[key]
        loc, out = self.loc, []
        if r == self.L:
            out.append((0, 0, (), p))
        elif p < len(loc.bb):
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
                    out.append((0, len(ev), ev, pp))
                    continue
                if pp >= len(loc.bb):
                    continue
                nm, single = self.base(rr, pp)
                for nm2, ni2, vl2, end in self.right(rr + 1, pp + 1):
                    if nm + nm2 <= self.max_edits:
                        out.append((nm + nm2, len(ev) + ni2, ev + single + vl2, end))
        if self.prune and out:
            out = [min(out, key=lambda c: (c[0], c[1], len(c[2]), c[2]))]
        self._right[key] = out
        return out

    def left(self, r, q):
        """Every way to have arrived at "read base r sits on backbone base q": [(NM, indels, pos0, variants)] of bases < r."""
        key = (r, q)
        if key in self._left:
            return self._left[key]
        loc, out = self.loc, []
        if r == 0:
            out.append((0, 0, q, ()))
        else:
            # (events, r1, p1): the state (r1, p1), r1 >= 1, from which `events` lead to base r on q
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
                for nm2, ni2, pos0, vl2 in self.left(r1 - 1, p1 - 1):
                    if nm + nm2 <= self.max_edits:
                        out.append((nm + nm2, len(ev) + ni2, pos0, vl2 + single + ev))
        if self.prune and out:
            out = [min(out, key=lambda c: (c[0], c[1], len(c[3]), c[2], c[3]))]
        self._left[key] = out
        return out

    def canon(self, o, b):
        """The smallest alignment admissible through the anchor (read offset o, backbone position b), or None:
        ((NM, indels, variants, pos0, list), end)."""
        best = None
        for nm1, ni1, pos0, vl1 in self.left(o, b):
            for nm2, ni2, vl2, end in self.right(o + K, b + K):
                if nm1 + nm2 > self.max_edits:
                    continue
                vl = vl1 + vl2
                cand = ((nm1 + nm2, ni1 + ni2, len(vl), pos0, vl), end)
                if best is None or cand[0] < best[0]:
                    best = cand
        return best


def align_read(loci, seq, max_edits, prune=False):
    """None, or (key, end, NH) with key = (NM, indels, variants, locus, strand, pos0, list): the read's alignment."""
    seq = seq.upper()
    canons = {}
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        for g, loc in enumerate(loci):
            search = _Search(loc, s, max_edits, prune)
            for o in seed_offsets(len(s)):
                for b in loc.kmers.get(s[o:o + K], []):
                    c = search.canon(o, b)
                    if c is not None:
                        (nm, ni, nv, pos0, vl), end = c
                        canons[(nm, ni, nv, g, strand, pos0, vl)] = end
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
    return best, canons[best], nh


def render(loc, s, pos0, vl):
    """(CIGAR, MD, Zs) of the walk, as simulate._truth_record writes them."""
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

    def push(op, n):
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += n
        else:
            cigar.append([op, n])

    while r < len(s):
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


def read_records(path_or_text):
    """[(qname, seq, qual or None)] of a FASTA / FASTQ file (plain or .gz) or of its text (bytes)."""
    if isinstance(path_or_text, bytes):
        data = path_or_text
    else:
        with open(path_or_text, "rb") as f:
            data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = data.decode().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [l.rstrip("\r") for l in lines]
    out, k = [], 0
    while k < len(lines):
        head = lines[k]
        if head.startswith("@"):
            out.append((head[1:].split()[0] if head[1:].split() else "", lines[k + 1], lines[k + 3]))
            k += 4
        elif head.startswith(">"):
            k += 1
            seq = ""
            while k < len(lines) and not lines[k].startswith(">"):
                seq += lines[k]
                k += 1
            out.append((head[1:].split()[0] if head[1:].split() else "", seq, None))
        else:
            raise ValueError("neither FASTA nor FASTQ: %r" % head[:40])
    return out


def align_text(loci, reads, max_edits=2, max_fragment=1000, prune=False):
    """The SAM text for `reads` = [records of file 1] or [records of file 1, records of file 2]."""
    paired = len(reads) == 2
    lines = ["@SQ\tSN:%s\tLN:%d" % (loc.name, len(loc.bb)) for loc in loci]
    for k in range(len(reads[0])):
        alns = []
        for m in range(len(reads)):
            qname, seq, qual = reads[m][k]
            a = align_read(loci, seq, max_edits, prune)
            alns.append((qname, seq.upper(), qual, a))
        conc = False
        if paired and alns[0][3] is not None and alns[1][3] is not None:
            (k0, e0, _), (k1, e1, _) = alns[0][3], alns[1][3]
            if k0[3] == k1[3] and k0[4] != k1[4]:
                plus, minus = (k0, k1) if k0[4] == 0 else (k1, k0)
                conc = plus[5] <= minus[5] and max(e0, e1) - min(k0[5], k1[5]) <= max_fragment
        for m, (qname, seq, qual, a) in enumerate(alns):
            if a is None:
                continue
            key, end, nh = a
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
            cigar, md, zs = render(loc, s, pos0, vl)
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:%d" % nh, "YT:Z:%s" % yt]
            lines.append("\t".join([qname, str(flag), loc.name, str(pos0 + 1), "60" if nh == 1 else "1", cigar, rnext, str(pnext),
                                    "0", s, q] + tags))
    return "\n".join(lines) + "\n"
