"""The plain-Python statement of the "hgx" aligner's rules (tests/align_ref.py) pinned: against the alignment each simulated read
of tests/golden/selftest_loop.json.gz was cut from, by a verifier of its own that rebuilds SEQ from a record, and on hand-made
loci whose records are written out by hand (tests/align_cases.py).  No GPU, no native code."""
import re

import pytest

import align_cases
import align_ref
from hisatgenotype_amd import simulate

GOLDEN = {"pairs_two_genes": 3, "single_test_id_and_list": 2, "basic_with_errors": 4}


def _truth_lines(Genes, Vars, refGenes, reads):
    """The lines simulate.truth_align writes for these mate files, and each read's true (NM, indels, variants)."""
    lines, cost = [], []
    for k in range(len(reads[0])):
        recs = []
        for m in range(2):
            qname, seq, _ = reads[m][k]
            s = align_ref.revcomp(seq) if m == 1 else seq
            recs.append((qname, s) + simulate._truth_record(qname, s, Genes, Vars, refGenes))
        for m, (qname, s, gene, pos0, cigar, md, zs, nm) in enumerate(recs):
            tags = ["NM:i:%d" % nm, "MD:Z:%s" % md] + (["Zs:Z:%s" % zs] if zs else []) + ["NH:i:1", "YT:Z:CP"]
            lines.append("\t".join([qname, str(99 if m == 0 else 147), refGenes[gene], str(pos0 + 1), "60", cigar, "=",
                                    str(recs[1 - m][3] + 1), "0", s, "I" * len(s)] + tags))
            items = zs.split(",") if zs else []
            cost.append((nm, sum("|S|" not in it for it in items), len(items)))
    return lines, cost


def _cost_of(line):
    f = line.split("\t")
    zs = [t[5:] for t in f[11:] if t.startswith("Zs:Z:")]
    items = zs[0].split(",") if zs else []
    return (int(f[11][5:]), sum("|S|" not in it for it in items), len(items))


def _own(line):
    """The columns of a record that do not depend on its mate: everything but the pair bits of FLAG, RNEXT, PNEXT and YT."""
    f = line.split("\t")
    return [f[0], int(f[1]) & 0xD0] + f[2:6] + f[9:-1]


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_fixture_reads_come_out_as_cut_or_cheaper(case):
    """Every simulated read whose true alignment has NM <= 2 is aligned, and its record is the one truth_align writes unless the
    aligner's (NM, indels, variants) is strictly smaller than the truth's -- never larger.  The columns that describe the MATE
    (pair bits of FLAG, RNEXT, PNEXT, YT) are compared where the mate came out as cut too: then the whole line is truth_align's.
    Error-free cases: at most 1 read in 100 differs."""
    n = differ = whole = 0
    for call in range(GOLDEN[case]):
        d, texts, me = align_cases.inputs()["%s-%d" % (case, call)]
        Genes, Vars, _, refGenes = d
        reads = [align_ref.read_records(t) for t in texts]
        truth, cost = _truth_lines(Genes, Vars, refGenes, reads)
        got = {}
        for line in align_cases.ref_text("%s-%d" % (case, call)).decode().split("\n"):
            if line and not line.startswith("@"):
                f = line.split("\t")
                got[(f[0], int(f[1]) & 0xC0)] = line
        same = []
        for k, t in enumerate(truth):
            f = t.split("\t")
            line = got.get((f[0], int(f[1]) & 0xC0))
            same.append(line is not None and _own(line) == _own(t))
            if cost[k][0] > 2:
                continue
            n += 1
            assert line is not None, "unaligned: %s" % f[0]
            if not same[k]:
                differ += 1
                print("%s-%d differs\n  aligner %s\n  truth   %s" % (case, call, line, t))
                assert _cost_of(line) < cost[k], "not cheaper than the truth: %s" % f[0]
        for k, t in enumerate(truth):
            if same[k] and same[k ^ 1]:
                assert got[(t.split("\t")[0], int(t.split("\t")[1]) & 0xC0)] == t
                whole += 1
    assert n > 300 and whole > 300
    if case != "basic_with_errors":
        assert differ * 100 <= n, (differ, n)


def _verify(line, loci):
    """Rebuild SEQ from the backbone, CIGAR, MD and Zs of one record (a verifier of its own, not the renderer backwards)."""
    f = line.split("\t")
    loc = {l.name: l for l in loci}[f[2]]
    by_id = {vid: (t, p, d) for t, p, d, vid in loc.variants}
    tags = dict((t[:2], t[5:]) for t in f[11:])
    seq, p, r = f[9], int(f[3]) - 1, 0
    zs = [it.split("|") for it in tags["Zs"].split(",")] if "Zs" in tags else []
    md = re.findall(r"(\d+)|(\^[A-Z]+)|([A-Z])", tags["MD"])
    md = [("run", int(a)) if a else ("del", b[1:]) if b else ("sub", c) for a, b, c in md]
    subs, dels, q = {}, {}, p                   # what MD says, by backbone position
    for kind, v in md:
        if kind == "run":
            q += v
        elif kind == "del":
            dels[q] = v
            q += len(v)
        else:
            subs[q] = v
            q += 1
    built, nm, zi = [], 0, 0
    for n, op in re.findall(r"(\d+)([MID])", f[5]):
        n = int(n)
        if op == "M":
            for _ in range(n):
                if p in subs:
                    assert subs[p] == loc.bb[p] != seq[r]
                    if zi < len(zs) and zs[zi][1] == "S" and by_id[zs[zi][2]][1] == p:
                        assert by_id[zs[zi][2]][0] == "single"
                        built.append(by_id[zs[zi][2]][2])
                        zi += 1
                    else:
                        built.append(seq[r])            # an unknown edit: nothing to rebuild it from
                        nm += 1
                else:
                    built.append(loc.bb[p])
                p += 1
                r += 1
        elif op == "D":
            t, vp, d = by_id[zs[zi][2]]
            assert zs[zi][1] == "D" and t == "deletion" and vp == p and int(d) == n and dels[p] == loc.bb[p:p + n]
            zi += 1
            p += n
        else:
            t, vp, d = by_id[zs[zi][2]]
            assert zs[zi][1] == "I" and t == "insertion" and vp == p
            built.append(d[:n])
            assert n == min(len(d), len(seq) - r)
            zi += 1
            r += n
    assert zi == len(zs) and "".join(built) == seq and nm == int(tags["NM"]) and q == p and len(subs) + 0 >= nm
    assert len(f[10]) == len(seq)


@pytest.mark.parametrize("key", [k for k in align_cases.INPUT_IDS if not k.startswith("empty")])
def test_every_record_rebuilds_its_read(key):
    d, _, me = align_cases.inputs()[key]
    loci = align_ref.loci_from_dicts(*d)
    n = 0
    for line in align_cases.ref_text(key).decode().split("\n"):
        if line and not line.startswith("@"):
            _verify(line, loci)
            assert int(line.split("\t")[11][5:]) <= me
            n += 1
    assert n > 0


@pytest.mark.parametrize("k", range(7))
def test_hand_made_loci(k):
    title, loci, reads, max_edits, expected = align_cases.hand_cases()[k]
    got = align_ref.align_text(loci, [[(n, s, None) for n, s in reads]], max_edits)
    assert got == align_cases.expected_text(loci, reads, expected), title


def test_pair_flags():
    """FLAG and YT of every pair case, written down by hand (align_cases.pair_reads)."""
    m1, m2, flags = align_cases.pair_reads()
    loci = align_cases.pair_loci()
    text = align_ref.align_text(loci, [[(n, s, None) for n, s in m1], [(n, s, None) for n, s in m2]])
    recs = [l.split("\t") for l in text.split("\n") if l and not l.startswith("@")]
    assert [(int(r[1]), r[-1][5:]) for r in recs] == flags
    by = {(r[0], int(r[1]) & 0xC0): r for r in recs}
    assert by[("fr", 0x40)][6:9] == ["=", "301", "0"] and by[("fr", 0x80)][6:9] == ["=", "101", "0"]
    assert by[("loci", 0x40)][6:8] == ["P2*BACKBONE", "301"] and by[("loci", 0x80)][6:8] == ["P1*BACKBONE", "101"]
    assert by[("half", 0x40)][6:8] == ["=", "501"]


def test_seed_offsets_and_short_reads():
    assert align_ref.seed_offsets(15) == [] and align_ref.seed_offsets(16) == [0] and align_ref.seed_offsets(19) == [0, 3]
    assert align_ref.seed_offsets(100) == list(range(0, 85, 4)) and align_ref.seed_offsets(101) == list(range(0, 85, 4)) + [85]
    loc = align_cases.length_locus()
    assert align_ref.align_read([loc], loc.bb[20:35], 2) is None
    assert align_ref.align_read([loc], loc.bb[20:36], 2)[0][5] == 20
