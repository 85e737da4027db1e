"""The case table of the "hgx" aligner on a linear index: the smallest shapes at which it can go wrong, used by
tests/test_align_linear_ref.py (the statement itself), tests/test_align_linear_host.py (host route == statement) and
tests/test_gpu_align_linear.py (kernels == statement).  Families have <= 130 alleles of <= 600 bases.

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
    out.append(case("max-edits-0", fam, reads, max_edits=0))
    out.append(case("max-edits-4", fam, reads, max_edits=4))
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
    m1 = [(q, s, None) for q, s, _ in reads[:6]]
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


def _all():
    out = []
    for f in (_length_cases, _n_cases, _edit_cases, _position_cases, _bucket_cases, _k_cases, _pair_cases, _chunk_cases, _size_cases):
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
