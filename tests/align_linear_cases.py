"""The case table of the "hgx" aligner on a linear index: the smallest shapes at which it can go wrong, used by
tests/test_align_linear_ref.py (the statement itself), tests/test_align_linear_host.py (host route == statement) and
tests/test_gpu_align_linear.py (kernels == statement).  Most families have <= 130 alleles of <= 600 bases; the cases of WIDE reach
the upper bits of the key's fields: position 65 536 and the last accepted one (2^20 - 2), allele 65 536 and above.  The top of the
ALLELE field (2^20 - 1 alleles) would be a header of 20 MB: it is deliberately left to the refusal test of
tests/test_align_linear_host.py (test_limits_of_the_index).  Every case costs the statement less than about 5 s.

A case: dict(name, Genes, refGenes, reads = [records] or [mate-1 records, mate-2 records] with a record = (qname, seq, qual or None),
max_edits, k, decline = the code the kernels' route must report (0: it gives the bytes), budget = the value of the test switch
align_linear_budget (None: the library's budgets)).  ref_text(case) is the statement's text, computed once per process.
"""
import random

import align_linear_ref as ref

DECLINE_READ_LEN, DECLINE_BUDGET, DECLINE_LINE = 2, 3, 4
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def rnd(seed, n):
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(n))


_ACGT_OF_BYTE = bytes(b"ACGT"[b & 3] for b in range(256))


def rnd_long(seed, n):
    """As rnd() for the sequences of 10^5 .. 10^6 bases (one call of the generator, not one per base)."""
    return random.Random(seed).randbytes(n).translate(_ACGT_OF_BYTE).decode()


def mut(s, positions, to=None):
    s = list(s)
    for p in positions:
        s[p] = to if to is not None else _OTHER.get(s[p], "A")
    return "".join(s)


def family(alleles, gene="G"):
    """(Genes, refGenes) of [(name suffix, sequence)]: the backbone entry comes first and is not indexed."""
    Genes = {gene: {"%s*BACKBONE" % gene: alleles[0][1]}}
    for name, seq in alleles:
        Genes[gene]["%s*%s" % (gene, name)] = seq
    return Genes, {gene: "%s*BACKBONE" % gene}


def near_identical(n, length, seed, at=()):
    """n alleles of one random sequence; allele i carries a substitution at at[i % len(at)] + i (none if `at` is empty)."""
    base = rnd(seed, length)
    return [("%03d" % i, mut(base, [(at[i % len(at)] + i) % length]) if at else base) for i in range(n)]


def case(name, alleles, reads, max_edits=2, k=10, decline=0, budget=None, gene="G"):
    Genes, refGenes = alleles if isinstance(alleles, tuple) else family(alleles, gene)
    if reads and isinstance(reads[0], tuple):
        reads = [reads]
    return dict(name=name, Genes=Genes, refGenes=refGenes, reads=reads, max_edits=max_edits, k=k, decline=decline, budget=budget)


def _length_cases():
    out = []
    fam = [("01", rnd(1, 600)), ("02", mut(rnd(1, 600), [300])), ("03", rnd(2, 600)), ("04", rnd(3, 420))]
    a = fam[0][1]
    for L in (15, 16, 47, 48, 100, 251, 256, 257):
        w = a[40:40 + L]
        reads = [("exact", w, None), ("rev", ref.revcomp(w), None), ("mm1", mut(w, [L - 1]), None), ("mm2", mut(w, [L // 2, L - 2]), None),
                 ("mm3", mut(w, [L // 3, L // 2, L - 1]), None), ("junk", rnd(90 + L, L), None)]
        out.append(case("length-%d" % L, fam, reads, decline=DECLINE_READ_LEN if L > 256 else 0))
    return out


def _n_cases():
    fam = [("01", rnd(4, 500)), ("02", mut(rnd(4, 500), [130], "N")), ("03", mut(rnd(4, 500), [140], "R"))]
    w = fam[0][1][100:200]
    reads = [("n-in-seed-1", mut(w, [5], "N"), None), ("n-in-every-seed", mut(w, [5, 20, 40], "N"), None), ("n-outside", mut(w, [60], "N"), None),
             ("n-twice-outside", mut(w, [60, 70], "N"), None), ("n-three", mut(w, [60, 70, 80], "N"), None), ("plain", w, None),
             ("n-at-allele-n", mut(w, [30], "N"), None)]
    return [case("n-bases", fam, reads)]


def _edit_cases():
    fam = [("01", rnd(5, 400)), ("02", mut(rnd(5, 400), [210])), ("03", rnd(6, 400))]
    w = fam[0][1][150:250]
    reads = [("seed1", mut(w, [3]), None), ("seed1-twice", mut(w, [3, 12]), None), ("seed1-and-2", mut(w, [3, 20]), None),
             ("seed2", mut(w, [20]), None), ("seed2-and-3", mut(w, [20, 40]), None), ("seed1-and-3", mut(w, [3, 40]), None),
             ("seed1-2-3", mut(w, [3, 20, 40]), None), ("rev-seed1-and-2", ref.revcomp(mut(w, [3, 20])), None)]
    out = [case("edit-positions", fam, reads)]
    w5 = [mut(w, [3, 20, 40, 52, 70][:n]) for n in range(6)] + [mut(w, [90, 91, 92, 93]), mut(w, [3, 20, 40, 52, 90])]
    reads = [("e%d" % n, s, None) for n, s in enumerate(w5)]
    for me in (0, 4, 1, 3):
        out.append(case("max-edits-%d" % me, fam, reads, max_edits=me))
    return out


def _position_cases():
    u = rnd(7, 48)
    half = rnd(8, 24)
    pal = half + ref.revcomp(half)
    fam = [("01", rnd(9, 300)), ("short", rnd(9, 300)[:40]), ("rep", rnd(10, 60) + u + rnd(11, 50) + u + rnd(12, 30)),
           ("pal", rnd(13, 100) + pal + rnd(14, 100)), ("tail", rnd(15, 200) + u)]
    a = fam[0][1]
    reads = [("at-0", a[:48], None), ("at-end", a[-48:], None), ("at-end-rev", ref.revcomp(a[-48:]), None), ("repeat", u, None), ("palindrome", pal, None),
             ("past-end", a[-40:] + "ACGTACGT", None), ("longer-than-short", a[:48], None)]
    return [case("hit-positions", fam, reads)]


def _bucket_cases():
    out = []
    for n in (1, 63, 64, 65, 129):
        fam = near_identical(n, 200, 20 + n, at=(150,))
        w = fam[0][1][20:120]
        reads = [("shared", w, None), ("shared-mm", mut(w, [50]), None), ("rev", ref.revcomp(w), None)]
        out.append(case("bucket-%d" % n, fam, reads))
    fam = near_identical(129, 200, 20 + 129, at=(150,))
    out.append(case("bucket-129-k200", fam, [("shared", fam[0][1][20:120], None), ("over-snp", fam[0][1][100:200], None)], k=200))
    return out


def _k_cases():
    out = []
    base = rnd(30, 300)
    fam = [("%02d" % i, base) for i in range(10)]
    w = base[100:200]
    for k in (1, 9, 10, 11):
        out.append(case("k-%d-of-10" % k, fam, [("ten", w, None), ("ten-rev", ref.revcomp(w), None)], k=k))
    # four alleles at NM 0, six at NM 1: k = 6 cuts the NM 1 level, which has more hits than are left of k
    fam = [("%02d" % i, base if i % 3 == 0 else mut(base, [150])) for i in range(10)]
    out.append(case("k-cuts-a-level", fam, [("lvl", w, None), ("lvl-mm", mut(w, [10]), None)], k=6))
    return out


def _pair_cases():
    fam = near_identical(12, 400, 40, at=(200,))
    a = fam[0][1]
    junk = rnd(41, 100)
    m1 = [("both", a[10:110], "F" * 100), ("half", a[50:150], "#" * 50 + "F" * 50), ("none", junk, "F" * 100), ("other-half", junk, "F" * 100),
          ("both2", mut(a[20:120], [5]), "ABCDE" * 20)]
    m2 = [("both", ref.revcomp(a[250:350]), "G" * 100), ("half", junk, "G" * 100), ("none", ref.revcomp(junk), "G" * 100),
          ("other-half", ref.revcomp(a[260:360]), "G" * 100), ("both2", ref.revcomp(a[280:380]), "EDCBA" * 20)]
    return [case("pairs", fam, [m1, m2]), case("pairs-k3", fam, [m1, m2], k=3), case("single-end-fastq", fam, [m1])]


def unit_counts(c):
    """Per read (single-end) or pair: (candidates, records bound = sum of min(k, candidates) per read) as the chunk cut counts them."""
    alleles = ref.index_of(c["Genes"], c["refGenes"])
    out = []
    for i in range(len(c["reads"][0])):
        cand = rec = 0
        for m in range(len(c["reads"])):
            n = ref.candidates(alleles, c["reads"][m][i][1], c["max_edits"])
            cand += n
            rec += min(c["k"], n)
        out.append((cand, rec))
    return out


def _chunk_cases():
    """One read below, at and above every cut: the candidate budget, the record budget, the span; the read that alone passes the
    candidate budget or the record budget, or whose record is too long, BEHIND chunks that have run and appended their records (what
    they appended and counted is taken back), and as the first read."""
    out = []
    fam = near_identical(6, 300, 50, at=(250,))
    a = fam[0][1]
    reads = [("r%d" % i, a[10 + 7 * i:110 + 7 * i], None) for i in range(7)] + [("junk", rnd(51, 100), None), ("r8", a[100:200], None)]
    probe = case("probe", fam, reads)
    units = unit_counts(probe)
    c2, r2 = units[0][0] + units[1][0], units[0][1] + units[1][1]
    for d in (-1, 0, 1):
        out.append(case("cut-candidates%+d" % d, fam, reads, budget="%d" % (c2 + d)))
        out.append(case("cut-records%+d" % d, fam, reads, budget="%d,%d" % (1 << 20, r2 + d)))
    for n in (3, 4, 5, 8, 9):
        out.append(case("span-4-reads-%d" % n, fam, reads[:n], budget="%d,%d,4" % (1 << 20, 1 << 20)))
    # the same cuts at the other two slot widths: the kernels keep 4 seed slots per read at max_edits 0 and 1, 8 at 2 and 3, 12 at 4,
    # and a chunk's planes, counts and buckets start at (its first read) x (that width)
    for me in (1, 4):
        units = unit_counts(case("probe", fam, reads, max_edits=me))
        c2 = units[0][0] + units[1][0]
        assert units[2][0] > 1
        for d in (-1, 0, 1):
            out.append(case("cut-candidates%+d-e%d" % (d, me), fam, reads, max_edits=me, budget="%d" % (c2 + d)))
        for n in (3, 4, 5, 8, 9):
            out.append(case("span-4-reads-%d-e%d" % (n, me), fam, reads[:n], max_edits=me, budget="%d,%d,4" % (1 << 20, 1 << 20)))
    m1 =[(q, s, None) for q, s, _ in reads[:6]]
    m2 = [(q, ref.revcomp(a[150 + 5 * i:250 + 5 * i]), None) for i, (q, _, _) in enumerate(m1)]
    pr = case("probe", fam, [m1, m2])
    pu = unit_counts(pr)
    for d in (-1, 0, 1):
        out.append(case("pairs-cut-candidates%+d" % d, fam, [m1, m2], budget="%d" % (pu[0][0] + pu[1][0] + d)))
    out.append(case("pairs-span-4", fam, [m1, m2], budget="%d,%d,4" % (1 << 20, 1 << 20)))
    # a read with twelve times the candidates of the others (both strands of a palindrome in six alleles): behind a span that has
    # run, behind a chunk that the budget closed and that has run, and in front of everything
    half = rnd(52, 50)
    pal = half + ref.revcomp(half)
    famp = [("%02d" % i, rnd(53, 80) + pal + rnd(54, 80)) for i in range(6)] + [("x", rnd(55, 300))]
    x = famp[-1][1]
    small = [("s%d" % i, x[20 * i:100 + 20 * i], None) for i in range(4)]
    big = ("big", pal, None)
    pc = case("probe", famp, small + [big])
    u = unit_counts(pc)
    assert u[4][0] > max(c for c, _ in u[:4]) > 0
    lim = u[4][0] - 1
    assert sum(c for c, _ in u[:4]) <= lim         # the four small reads are ONE chunk of the first span; `big` is the second span's
    out.append(case("budget-decline-behind-a-span", famp, small + [big], budget="%d,%d,4" % (lim, 1 << 20), decline=DECLINE_BUDGET))
    many = [("m%d" % i, x[15 * i:100 + 15 * i], None) for i in range(12)]
    um = unit_counts(case("probe", famp, many))
    assert all(c > 0 for c, _ in um) and sum(c for c, _ in um) > lim > sum(c for c, _ in um[:-1])      # the budget closes a chunk in front of the last
    out.append(case("budget-decline-behind-a-chunk", famp, many + [big], budget="%d" % lim, decline=DECLINE_BUDGET))
    # the record budget: `big` alone would write min(k, candidates) = 10 records, the small reads 3 each
    assert u[4][1] == 10 and all(r == 3 for _, r in u[:4])
    out.append(case("record-budget-decline-behind-chunks", famp, small + [big], budget="%d,9" % (1 << 20), decline=DECLINE_BUDGET))
    # a record longer than the kernels write (a read name of 4 000 bytes), in the second span
    out.append(case("line-decline-behind-a-span", famp, small + [("n" * 4000, x[30:130], None)], budget="%d,%d,4" % (1 << 20, 1 << 20),
                    decline=DECLINE_LINE))
    out.append(case("budget-decline-first", famp, [big] + small, budget="%d" % lim, decline=DECLINE_BUDGET))
    out.append(case("budget-exactly-one-read", famp, small + [big], budget="%d" % u[4][0]))
    return out


def _size_cases():
    """8 191, 8 192 and 8 193 reads on a four-allele family, around the scan tiles: sixteen distinct sequences under distinct names."""
    base = rnd(60, 120)
    fam = [("01", base), ("02", mut(base, [60])), ("03", base[:90]), ("04", rnd(61, 120))]
    pool = [base[3 * i:3 * i + 40] for i in range(8)] + [ref.revcomp(base[5 * i:5 * i + 40]) for i in range(6)] + [mut(base[10:50], [20]), rnd(62, 40)]
    out = []
    for n in (8191, 8192, 8193):
        out.append(case("reads-%d" % n, fam, [("q%d" % i, pool[(i * 7) % 16], None) for i in range(n)]))
    return out


def _spoil(s, seeds):
    """A substitution in the middle of each of the 16-mers `seeds` of s."""
    return mut(s, [16 * j + 7 for j in seeds])


def _border_cases():
    """Windows that would run over an allele's border: the text is the alleles concatenated, so such a window MATCHES; only the test
    0 <= pos0 <= len - L keeps it out.  The first exact seed takes a hit, so a read that starts in front of a border carries a
    substitution in every seed that lies wholly or partly in front of it: else the border-side seeds, which the rule silences, would
    hide a missing test.  Only `control` hits."""
    A, B, C = rnd(100, 200), rnd(101, 200), rnd(102, 200)
    fam = [("A", A), ("B", B), ("C", C)]
    s20, s40 = _spoil(A[-20:] + B[:80], (0, 1)), _spoil(A[-40:] + B[:60], (0, 1, 2))
    reads = [("end-ab", A[-60:] + B[:40], None), ("end-bc-rev", ref.revcomp(B[-60:] + C[:40]), None), ("end-a99", A[-99:] + B[:1], None),
             ("start-20", s20, None), ("start-20-rev", ref.revcomp(s20), None), ("start-40", s40, None), ("start-40-rev", ref.revcomp(s40), None),
             ("start-1", A[-1:] + B[:99], None), ("start-1-spoiled", _spoil(A[-1:] + B[:99], (0,)), None),
             ("seed-2-at-0-of-first", rnd(103, 16) + A[:84], None), ("seed-3-at-0-of-first", rnd(104, 32) + A[:68], None),
             ("past-the-last", C[-60:] + "A" * 40, None), ("past-the-last-rev", ref.revcomp(C[-60:] + "A" * 40), None),
             ("control", B[50:150], None)]
    return [case("borders-e%d" % me, fam, reads, max_edits=me) for me in (2, 4)]


def _end_seed_cases():
    """Reads with ONE seed that is an allele's last or first 16-mer: the ends of the seed table, in the bytes."""
    fam = [("01", rnd(110, 300)), ("02", rnd(111, 250))]
    X, Y = fam[0][1], fam[1][1]
    reads = [("last-16", X[-16:], None), ("last-31", X[-31:], None), ("last-31-mm", mut(X[-31:], [30]), None),
             ("first-16-rev", ref.revcomp(X[:16]), None), ("first-16", X[:16], None), ("last-16-of-2", Y[-16:], None),
             ("last-16-of-2-rev", ref.revcomp(Y[-16:]), None)]
    return [case("one-seed-at-the-ends", fam, reads)]


MIXED_LENGTHS = (100, 16, 256, 31, 64, 15, 65, 40, 128, 129, 17, 192)


def _mixed_length_cases():
    """Reads of different lengths in ONE call, each with a mismatch at its last base (the 16-base read, whose only seed that would
    spoil, is exact): a route that takes another read's length sees no mismatch, or a window of junk.  With the library's budgets,
    with a cut behind (nearly) every read, behind the second read, with spans of 2 and 4 reads; as pairs whose mates differ in length,
    the 15-base mate (no seed) first in one pair and last in another; and with a last read of 257 bases, which declines."""
    T = rnd(120, 700)
    fam = [("01", T), ("02", mut(T, [300])), ("03", rnd(121, 300))]
    reads = []
    for n, L in enumerate(MIXED_LENGTHS):
        w = T[23 * n + 5:23 * n + 5 + L]
        reads.append(("len%d" % L, w if L == 16 else mut(w, [L - 1]), None))
    u = unit_counts(case("probe", fam, reads))
    big = max(c for c, _ in u)
    assert u[5][0] == 0 and min(c for i, (c, _) in enumerate(u) if i != 5) > 0
    out = [case("mixed-lengths", fam, reads),
           case("mixed-lengths-own-chunks", fam, reads, budget="%d" % big),            # (a read without candidates joins the chunk in front)
           case("mixed-lengths-cut-behind-2", fam, reads, budget="%d" % (u[0][0] + u[1][0])),
           case("mixed-lengths-span-2", fam, reads, budget="%d,%d,2" % (1 << 20, 1 << 20)),
           case("mixed-lengths-span-4", fam, reads, budget="%d,%d,4" % (1 << 20, 1 << 20))]
    # spans of four reads AND a cut behind (nearly) every read, at each slot width (4, 8, 12 slots per read): a chunk that starts
    # neither at its span's first read nor at the call's -- the only place where (first - span start) x width differs from both
    for me in (1, 2, 4):
        big = max(c for c, _ in unit_counts(case("probe", fam, reads, max_edits=me)))
        out.append(case("mixed-lengths-span-4-cuts-e%d" % me, fam, reads, max_edits=me, budget="%d,%d,4" % (big, 1 << 20)))
    by = {int(q[3:]): (q, s, None) for q, s, _ in reads}
    pairs = [(100, 16), (256, 31), (15, 64), (65, 40), (128, 129), (17, 192), (64, 15)]
    m1 = [("p%d" % i, by[a][1], None) for i, (a, _) in enumerate(pairs)]
    m2 = [("p%d" % i, ref.revcomp(by[b][1]), None) for i, (_, b) in enumerate(pairs)]
    pu = unit_counts(case("probe", fam, [m1, m2]))
    out += [case("mixed-pairs", fam, [m1, m2]),
            case("mixed-pairs-own-chunks", fam, [m1, m2], budget="%d" % max(c for c, _ in pu)),
            case("mixed-pairs-span-2", fam, [m1, m2], budget="%d,%d,2" % (1 << 20, 1 << 20))]
    out.append(case("mixed-257-last", fam, reads[:5] + [("len257", mut(T[40:297], [256]), None)], decline=DECLINE_READ_LEN))
    return out


def _empty_step_cases():
    """Chunks that append nothing between chunks that do: with spans of two reads, a span whose reads have no candidate (a chunk of
    no candidates), then a read with candidates and no hit in a chunk of its own (a chunk of no hits), then reads with hits again."""
    A, B = rnd(130, 200), rnd(131, 200)
    fam = [("A", A), ("B", B)]
    reads = [("h0", A[10:110], None), ("h1", B[20:120], None), ("junk0", rnd(132, 100), None), ("junk1", rnd(133, 100), None),
             ("straddle", A[-60:] + B[:40], None), ("h2", B[60:160], None), ("h3", A[90:190], None), ("junk2", rnd(134, 100), None)]
    u = [c for c, _ in unit_counts(case("probe", fam, reads))]
    assert u[2] == u[3] == u[7] == 0 and min(u[0], u[1], u[4], u[5], u[6]) > 0
    lim = max(u)
    assert u[0] + u[1] > lim and u[4] + u[5] > lim
    return [case("empty-steps-between-chunks", fam, reads, budget="%d,%d,2" % (lim, 1 << 20))]


def _shift_cases():
    """Windows at every one of the 64 bit offsets of the plane words, one and two words long and at every word count of a read."""
    S = rnd(140, 400)
    fam = [("01", S), ("02", mut(S, [399]))]
    reads = [("at%d" % p, mut(S[p:p + 70], [69]), None) for p in range(64)]
    reads += [("len%d" % L, mut(S[37:37 + L], [0, L - 1]), None) for L in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)]
    return [case("every-shift", fam, reads)]


def _tandem_cases():
    """Short tandem repeats (the CODIS loci): a read inside the repeat has a candidate at every period of every allele."""
    f1, f2 = rnd(150, 40), rnd(151, 40)
    fam = [("%d" % n, f1 + "AGAT" * n + f2) for n in (8, 12, 30, 31)] + [("polyA", "A" * 150)]
    reads = [("repeat", "AGAT" * 20, None), ("anchored", f1[-20:] + "AGAT" * 15, None), ("through-12", f1[-26:] + "AGAT" * 12 + f2[:26], None),
             ("poly-a", "A" * 100, None), ("poly-a-mm", mut("A" * 100, [50]), None), ("phase", "GATA" * 20, None)]
    return [case("tandem", fam, reads), case("tandem-e4-k1000", fam, reads, max_edits=4, k=1000)]


def _n_over_a_cases():
    """A read N where the allele has A (the planes code A as 00: without the mask an N seeds as A), and reads of A alone."""
    X = rnd(160, 300)
    w = X[100:200]

    def n_at(seed):
        return mut(w, [next(i for i in range(16 * seed, 16 * seed + 16) if w[i] == "A")], "N")
    fam = [("01", X), ("02", mut(X, [250])), ("polyA", "A" * 120), ("A-N-A", "A" * 60 + "N" + "A" * 59)]
    reads = [("n-seed-0", n_at(0), None), ("n-seed-1", n_at(1), None), ("n-seed-2", n_at(2), None), ("n-seed-0-rev", ref.revcomp(n_at(0)), None),
             ("n-seed-1-rev", ref.revcomp(n_at(1)), None), ("a16", "A" * 16, None), ("a20", "A" * 20, None), ("a47", "A" * 47, None),
             ("t20", "T" * 20, None), ("a30n", "A" * 30 + "N", None)]
    return [case("n-over-a", fam, reads), case("n-over-a-e4-k200", fam, reads, max_edits=4, k=200)]


def _k_cap_cases():
    """k = 1 024, the cap: a read with exactly 1 024 hits, and one with more."""
    out = []
    for name, n in (("k-cap-exactly-1024-hits", 1024 + 19), ("k-cap-1081-hits", 1100)):
        out.append(case(name, [("01", rnd(170, 100)), ("polyA", "A" * n)], [("a20", "A" * 20, None), ("t20", "T" * 20, None)], k=1024))
    return out


def _short_allele_cases():
    """Alleles of 0, 1, 15 and 16 bases among others (an empty sequence is accepted and gets its @SQ line), lower-case allele text."""
    X, Y, Z = rnd(180, 200), rnd(181, 120), rnd(182, 120)
    fam = [("01", X), ("empty", ""), ("one", "C"), ("fifteen", X[:15]), ("sixteen", X[20:36]), ("lower", Y.lower()),
           ("half-lower", Z[:60].lower() + Z[60:]), ("last", X[100:180])]
    reads = [("in-sixteen", X[20:36], None), ("at-0", X[:16], None), ("in-lower", Y[30:70], None), ("in-lower-mm", mut(Y[30:90], [59]), None),
             ("over-the-case-change", Z[30:90], None), ("over-the-case-change-rev", ref.revcomp(Z[20:100]), None), ("in-last", X[100:180], None),
             ("lower-read", Y[10:60].lower(), None)]
    return [case("short-and-lower-alleles", fam, reads)]


def _wide_cases():
    """The upper bits of the key's position and allele fields."""
    out = []
    W = rnd_long(190, 70000)
    at = lambda p: W[p:p + 100]
    reads = [("at-0", at(0), None), ("at-1023", at(1023), None), ("at-1024", at(1024), None), ("at-65535-mm", mut(at(65535), [50]), None),
             ("at-65536-rev", ref.revcomp(at(65536)), None), ("at-last", W[-100:], None)]
    out.append(case("wide-pos", [("small", rnd(191, 150)), ("wide", W)], reads))
    # 66 000 alleles of 20 bases; alleles 3, 300 and 65 999 are equal: with k = 2 the order over the high allele bits decides
    S = rnd_long(192, 20 * 66000)
    al = [S[20 * i:20 * i + 20] for i in range(66000)]
    al[300] = al[65999] = al[3]
    fam = [("%05d" % i, s) for i, s in enumerate(al)]
    reads = [("a0", al[0], None), ("a255", al[255], None), ("a256-rev", ref.revcomp(al[256]), None), ("a65535", al[65535], None),
             ("a65536", al[65536], None), ("triple", al[3], None), ("triple-mm", mut(al[3], [19]), None)]
    out.append(case("wide-alleles", fam, reads, k=2))
    # the longest allele the index takes, behind a short one: positions with the field's top bit set, and the last window
    T = rnd_long(193, (1 << 20) - 1)
    out.append(case("top-of-pos-field", [("short", rnd(194, 77)), ("longest", T)],
                    [("at-524288", T[524288:524388], None), ("last-100-rev", ref.revcomp(T[-100:]), None)], max_edits=0))
    return out


LINE_MAX = 4000                # HGX_ALNL_LINE_MAX: the bytes of the longest record, its '\n' counted, that the kernels write


def _line_limit_cases():
    """A record of exactly LINE_MAX bytes (the kernels give the bytes) and of one byte more (LINE), sized from the statement's line."""
    fam = [("01", rnd(200, 300)), ("02", rnd(201, 300))]
    a = fam[0][1]
    front = ("front", a[10:110], None)
    line = ref.align_text(ref.index_of(*family(fam)), [[("n", a[100:200], None)]]).split("\n")[3]
    assert line.startswith("n\t0\t")
    out = []
    for name, extra, decline in (("line-exactly-at-the-limit", 0, 0), ("line-one-byte-above-the-limit", 1, DECLINE_LINE)):
        qname = "n" * (LINE_MAX - len(line) - 1 + 1 + extra)
        out.append(case(name, fam, [front, (qname, a[100:200], None)], decline=decline))
    return out


def _all():
    out = []
    for f in (_length_cases, _n_cases, _edit_cases, _position_cases, _bucket_cases, _k_cases, _pair_cases, _chunk_cases, _size_cases,
              _border_cases, _end_seed_cases, _mixed_length_cases, _empty_step_cases, _shift_cases, _tandem_cases, _n_over_a_cases,
              _k_cap_cases, _short_allele_cases, _wide_cases, _line_limit_cases):
        out += f()
    return out


CASES = _all()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c["name"] for c in CASES]
SMALL = [n for n in NAMES if not n.startswith("reads-")]

_REF = {}


def ref_text(name):
    """The statement's text of the case, as bytes; computed once per process and not changed afterwards."""
    if name not in _REF:
        c = BY_NAME[name]
        _REF[name] = ref.align_text(ref.index_of(c["Genes"], c["refGenes"]), c["reads"], c["max_edits"], c["k"]).encode()
    return _REF[name]


def fasta(records):
    return "".join(">%s\n%s\n" % (q, s) for q, s, _ in records).encode()


def fastq(records):
    return "".join("@%s\n%s\n+\n%s\n" % (q, s, ql if ql is not None else "I" * len(s)) for q, s, ql in records).encode()


def texts(c):
    """The case's inputs as in-memory texts: FASTQ where its records carry qualities, else FASTA."""
    return [fastq(r) if r and r[0][2] is not None else fasta(r) for r in c["reads"]]
