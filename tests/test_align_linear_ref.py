"""The plain statement of the "hgx" aligner on a linear index (tests/align_linear_ref.py) checked against itself: the seeded hits
against the seedless brute force where the pigeonhole argument makes them equal, and the whole text against records written by
hand for a three-allele family."""
import random

import pytest

import align_linear_cases as lc
import align_linear_ref as ref


@pytest.mark.parametrize("name", [n for n in lc.SMALL])
def test_seeded_hits_equal_the_brute_force_where_seeds_are_implied(name):
    c = lc.BY_NAME[name]
    alleles = ref.index_of(c["Genes"], c["refGenes"])
    checked = 0
    for recs in c["reads"]:
        for _, seq, _ in recs:
            if len(seq) >= ref.K * (c["max_edits"] + 1):
                assert ref.hits(alleles, seq, c["max_edits"]) == ref.hits_brute(alleles, seq, c["max_edits"])
                checked += 1
            else:
                assert set(ref.hits(alleles, seq, c["max_edits"])) <= set(ref.hits_brute(alleles, seq, c["max_edits"]))
    assert checked or name in ("length-15", "length-16", "length-47", "one-seed-at-the-ends", "k-cap-exactly-1024-hits", "k-cap-1081-hits",
                               "wide-alleles")           # (every read of these is shorter than 16 (max_edits + 1) bases)


def test_the_cases_hold_what_their_names_say():
    """What the table's border, k-cap, empty-step, wide and record-length cases rest on, stated on the statement's own results."""
    def hits_by_read(name):
        c = lc.BY_NAME[name]
        alleles = ref.index_of(c["Genes"], c["refGenes"])
        return {q: ref.hits(alleles, s, c["max_edits"]) for recs in c["reads"] for q, s, _ in recs}
    for name in ("borders-e2", "borders-e4"):
        h = hits_by_read(name)
        assert [q for q in h if h[q]] == ["control"] and h["control"] == [(0, 1, 50, 0)]
        c = lc.BY_NAME[name]                          # ... and every other read's window DOES match where the alleles are one text
        text = "".join(s for _, s in ref.index_of(c["Genes"], c["refGenes"])) + "A" * 64
        one = [("all", text)]
        for q in ("end-ab", "end-bc-rev", "end-a99", "start-20", "start-20-rev", "start-1", "start-1-spoiled", "past-the-last", "past-the-last-rev"):
            assert ref.hits(one, dict((r[0], r[1]) for r in c["reads"][0])[q], c["max_edits"]), q
    assert len(hits_by_read("borders-e4")) == 14
    h = hits_by_read("k-cap-exactly-1024-hits")
    assert len(h["a20"]) == 1024 == len(h["t20"])
    assert len(hits_by_read("k-cap-1081-hits")["a20"]) == 1081
    h = hits_by_read("empty-steps-between-chunks")
    assert [bool(h[q]) for q in ("h0", "h1", "junk0", "junk1", "straddle", "h2", "h3", "junk2")] == [True, True, False, False, False, True, True, False]
    h = hits_by_read("wide-pos")
    assert [h[q][0][1:] for q in h] == [(1, 0, 0), (1, 1023, 0), (1, 1024, 0), (1, 65535, 0), (1, 65536, 1), (1, 69900, 0)]
    h = hits_by_read("wide-alleles")
    assert [x[1] for x in h["triple"]] == [3, 300, 65999] and [x[1] for x in h["a65536"]] == [65536]
    assert hits_by_read("top-of-pos-field") == {"at-524288": [(0, 1, 524288, 0)], "last-100-rev": [(0, 1, (1 << 20) - 1 - 100, 1)]}
    h = hits_by_read("every-shift")
    assert all(h["at%d" % p] == [(1, 0, p, 0), (1, 1, p, 0)] for p in range(64))
    for name, n in (("line-exactly-at-the-limit", lc.LINE_MAX), ("line-one-byte-above-the-limit", lc.LINE_MAX + 1)):
        assert max(len(l) + 1 for l in lc.ref_text(name).decode().split("\n")[:-1]) == n
    h = hits_by_read("mixed-lengths")
    assert [q for q in h if not h[q]] == ["len15"]


def test_random_reads_against_the_brute_force():
    rng = random.Random(5)
    base = lc.rnd(70, 300)
    alleles = [("X*%d" % i, lc.mut(base, rng.sample(range(300), 3))) for i in range(8)]
    for me in (0, 1, 2, 3, 4):
        for _ in range(6):
            L = rng.randrange(16 * (me + 1), 120)
            p = rng.randrange(0, 300 - L)
            s = lc.mut(alleles[rng.randrange(8)][1][p:p + L], rng.sample(range(L), rng.randrange(0, me + 2)))
            if rng.random() < 0.5:
                s = ref.revcomp(s)
            assert ref.hits(alleles, s, me) == ref.hits_brute(alleles, s, me)


def test_below_the_pigeonhole_length_the_seeded_set_is_the_rule():
    a = lc.rnd(71, 200)
    alleles = [("X*1", a)]
    w = a[50:97]                                     # 47 bases: two seeds, max_edits = 2
    both_seeds_hit = lc.mut(w, [3, 20])              # a mismatch in each seed: a hit for the brute force, none for the rule
    assert ref.hits_brute(alleles, both_seeds_hit, 2) == [(2, 0, 50, 0)] and ref.hits(alleles, both_seeds_hit, 2) == []
    assert ref.hits(alleles, lc.mut(w, [3, 40]), 2) == [(2, 0, 50, 0)]
    assert ref.hits(alleles, a[:15], 2) == [] and ref.hits_brute(alleles, a[:15], 2) == []


def test_three_allele_family_by_hand():
    a1 = "ACGTTGCAAGGCTTAACCGGATATCGCGTTAACCAGTCAGGATCCATGCA"          # 50 bases
    a2 = a1[:20] + "G" + a1[21:]                                         # A -> G at 20
    a3 = a1[10:45]                                                       # 35 bases: a1's middle
    Genes = {"T": {"T*BACKBONE": a1.lower(), "T*01": a1.lower(), "T*02": a2, "T*03": a3}}
    refGenes = {"T": "T*BACKBONE"}
    alleles = ref.index_of(Genes, refGenes)
    assert alleles == [("T*01", a1), ("T*02", a2), ("T*03", a3)]
    r1 = a1[12:44]                                                       # 32 bases over position 20: exact on T*01 and T*03, one edit on T*02
    r2 = ref.revcomp(a2[0:32])                                           # reverse strand, exact on T*02 at 1, one edit on T*01; T*03 is too far right
    r3 = "N" + a1[1:20]                                                  # 20 bases, N in the only seed: no hit
    m1 = [("p1", r1, "A" * 31 + "B"), ("p2", r3, "C" * 20)]
    m2 = [("p1", r2, "D" * 31 + "E"), ("p2", a3[:16], "F" * 16)]
    got = ref.align_text(alleles, [m1, m2], max_edits=1, k=2)
    rc2 = ref.revcomp(r2)
    want = "\n".join([
        "@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:T*01\tLN:50", "@SQ\tSN:T*02\tLN:50", "@SQ\tSN:T*03\tLN:35",
        # p1/1: hits (0, T*01, 12, +), (0, T*03, 2, +), (1, T*02, 12, +): three hits, k = 2
        "p1\t65\tT*01\t13\t1\t32M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:32\tNH:i:2" % (r1, "A" * 31 + "B"),
        "p1\t321\tT*03\t3\t1\t32M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:32\tNH:i:2" % (r1, "A" * 31 + "B"),
        # p1/2: hits (0, T*02, 0, -), (1, T*01, 0, -)
        "p1\t145\tT*02\t1\t1\t32M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:32\tNH:i:2" % (rc2, "E" + "D" * 31),
        "p1\t401\tT*01\t1\t1\t32M\t*\t0\t0\t%s\t%s\tAS:i:-6\tNM:i:1\tMD:Z:20A11\tNH:i:2" % (rc2, "E" + "D" * 31),
        # p2/1 has no hit; p2/2 (16 bases of T*03 = T*01[10:26], not T*02's): 0x80 + 0x1 + 0x8
        "p2\t137\tT*01\t11\t1\t16M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:16\tNH:i:2" % (a3[:16], "F" * 16),
        "p2\t393\tT*03\t1\t1\t16M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:16\tNH:i:2" % (a3[:16], "F" * 16),
    ]) + "\n"
    assert got == want
    assert ref.counters(alleles, [m1, m2], 1, 2) == (4, 3, 6)
    # one hit: MAPQ 60, single-end flags
    solo = ref.align_text(alleles, [[("s", a1[0:25], None)]], max_edits=0, k=10).split("\n")[4:]
    assert solo == ["s\t0\tT*01\t1\t60\t25M\t*\t0\t0\t%s\t%s\tAS:i:0\tNM:i:0\tMD:Z:25\tNH:i:1" % (a1[0:25], "I" * 25), ""]
