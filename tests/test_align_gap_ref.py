"""The plain-Python statement of the gap tier (tests/align_gap_ref.py) pinned: on hand-made loci whose records are written out by
hand (tests/align_gap_cases.py), against align_ref on every input of its own suites (only the mate fields of a pair with a newly
aligned mate may differ), by a verifier that rebuilds SEQ from a gapped record, and through the host front end, which must keep
gapped records.  The statement offers no pruned form (the enumeration is exhaustive), so there is no shortcut to compare.  No GPU;
native code only in the front-end test."""
import re

import pytest

import align_cases
import align_gap_cases as gc
import align_gap_ref
import align_ref
from test_align_ref import _verify


def _plain(reads):
    return [[(n, s, None) for n, s in reads]]


@pytest.mark.parametrize("k", range(gc.N_HAND))
def test_hand_made_loci(k):
    title, loci, reads, max_edits, gap, expected = gc.hand_cases()[k]
    st = {}
    got = align_gap_ref.align_text(loci, _plain(reads), max_edits, gap=gap, stats=st)
    assert got == align_cases.expected_text(loci, reads, expected), title
    assert align_gap_ref.align_text(loci, _plain(reads), max_edits, gap=0) == align_ref.align_text(loci, _plain(reads), max_edits)
    # the records align_ref writes are the reads that align end to end: the tier never ran for them
    e2e = align_ref.align_text(loci, _plain(reads), max_edits).count("\n") - len(loci)
    assert st["gapped"] == sum(e is not None for e in expected) - e2e and st["gapped"] <= st["searched"] <= len(reads) - e2e
    assert st["searched"] == sum(align_gap_ref.has_anchor(loci, s) for _, s in reads) - e2e


def test_a_known_deletion_is_not_a_novel_one():
    """`same` of the known-indel case lacks exactly the bases of hv3: end to end, NM 0, and not counted as searched."""
    _, loci, reads, me, gap, _ = gc.hand_cases()[7]
    st = {}
    text = align_gap_ref.align_text(loci, _plain(reads[2:]), me, gap=gap, stats=st)
    assert "NM:i:0" in text and "50|D|hv3" in text and st == dict(searched=0, gapped=0, bases=0)
    assert text == align_ref.align_text(loci, _plain(reads[2:]), me)


def test_the_budget_counts_the_gap():
    """gap = 16 with max_edits 2 is a gap of at most 2; gap = 1 takes only the one-base gaps whatever the budget."""
    _, loci, reads, _, _, _ = gc.hand_cases()[0]
    cig = lambda t: [l.split("\t")[5] for l in t.split("\n") if l and l[0] != "@"]
    assert cig(align_gap_ref.align_text(loci, _plain(reads), 2, gap=16)) == ["50M1D50M", "50M1I49M"]
    assert cig(align_gap_ref.align_text(loci, _plain(reads), 5, gap=1)) == ["50M1D50M", "50M1I49M"]
    wide = cig(align_gap_ref.align_text(loci, _plain(reads), 5, gap=16))       # (the four-base gaps have a placement further left)
    assert len(wide) == 6 and "4D" in wide[2] and "4I" in wide[5] and wide[:2] + wide[3:5] == ["50M1D50M", "50M3D50M", "50M1I49M", "50M3I47M"]


def _fields(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("@")]


def test_a_gapped_mate_turns_up_into_cp():
    loci, m1, m2 = gc.pair_case()
    reads = [[(n, s, None) for n, s in m1], [(n, s, None) for n, s in m2]]
    before = _fields(align_ref.align_text(loci, reads))
    after = _fields(align_gap_ref.align_text(loci, reads, gap=gc.GAP))
    assert [(f[0], int(f[1]), f[-1]) for f in before] == [("up", 73, "YT:Z:UP"), ("cp", 99, "YT:Z:CP"), ("cp", 147, "YT:Z:CP")]
    assert [(f[0], int(f[1]), f[5], f[-1]) for f in after] == [("up", 99, "100M", "YT:Z:CP"), ("up", 147, "50M1D50M", "YT:Z:CP"),
                                                             ("cp", 99, "100M", "YT:Z:CP"), ("cp", 147, "100M", "YT:Z:CP")]
    assert after[0][6:9] == ["=", "401", "0"] and after[1][3] == "401" and after[1][6:9] == ["=", "251", "0"]
    assert after[2:] == before[1:]


def _own(f):
    """The columns of a record that do not depend on its mate."""
    return [f[0], int(f[1]) & ~(0x2 | 0x8 | 0x20)] + f[2:6] + f[8:-1]


@pytest.mark.parametrize("key", [k for k in align_cases.INPUT_IDS])
def test_align_refs_inputs_change_only_in_mate_fields(key):
    """Under gap = 16 every record align_ref writes is written again; it differs only in FLAG 0x8 / 0x20 / 0x2, RNEXT, PNEXT and YT,
    and only where its mate is written now and was not before.  Every other record is new and gapped."""
    before = _fields(align_cases.ref_text(key).decode())
    after = _fields(gc.ref_text(key).decode())
    paired = len(align_cases.inputs()[key][1]) == 2
    if not paired:                                                            # (single-end files may repeat a name: the record's SEQ tells)
        before, after = ([[f[0] + "/" + f[9]] + f[1:] for f in x] for x in (before, after))
    old = {(f[0], int(f[1]) & 0xC0): f for f in before}
    new = {(f[0], int(f[1]) & 0xC0): f for f in after}
    assert len(old) == len(before) and len(new) == len(after)
    assert [k for k in new if k in old] == list(old)                          # all kept, in order
    mate_of = {}                                                              # (the mates of a fixture pair have names of their own)
    if paired:
        r1, r2 = (align_ref.read_records(x) for x in align_cases.inputs()[key][1])
        for (n1, _, _), (n2, _, _) in zip(r1, r2):
            mate_of[(n1, 0x40)], mate_of[(n2, 0x80)] = (n2, 0x80), (n1, 0x40)
    for k, f in new.items():
        if k not in old:
            assert gc.is_gapped("\t".join(f))
            continue
        mate = mate_of.get(k)
        if f != old[k]:
            assert paired and mate in new and mate not in old, f
            assert _own(f) == _own(old[k])
            assert int(old[k][1]) & 0x8 and old[k][-1] == "YT:Z:UP" and not int(f[1]) & 0x8 and f[-1] in ("YT:Z:CP", "YT:Z:DP")
        else:
            assert not (paired and mate in new and mate not in old)
    st = {}
    gc.ref_text(key, stats=st)
    assert st["gapped"] == len(after) - len(before)


def _verify_gapped(line, loci):
    """Rebuild SEQ from the backbone, CIGAR, MD and Zs of a record with ONE novel gap (a verifier of its own, not the renderer
    backwards): an I / D op that no Zs item stands for is the gap; the Zs gap counts are checked too (inserted bases count into the
    next item's, deleted bases do not).  Returns (gap length, read offset of the gap)."""
    f = line.split("\t")
    loc = {l.name: l for l in loci}[f[2]]
    by_id = {vid: (t, p, d) for t, p, d, vid in loc.variants}
    tags = dict((t[:2], t[5:]) for t in f[11:])
    seq, p, r = f[9], int(f[3]) - 1, 0
    zs = [it.split("|") for it in tags["Zs"].split(",")] if "Zs" in tags else []
    md = re.findall(r"(\d+)|(\^[A-Z]+)|([A-Z])", tags["MD"])
    assert "".join(a or b or c for a, b, c in md) == tags["MD"] and re.fullmatch(r"\d+(?:(?:\^[A-Z]+|[A-Z])\d+)*", tags["MD"])
    md = [("run", int(a)) if a else ("del", b[1:]) if b else ("sub", c) for a, b, c in md]
    subs, dels, q = {}, {}, p
    for kind, v in md:
        if kind == "run":
            q += v
        elif kind == "del":
            dels[q] = v
            q += len(v)
        else:
            subs[q] = v
            q += 1
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", f[5])]
    assert "".join("%d%s" % o for o in ops) == f[5] and ops[0][1] == "M" and ops[-1][1] == "M"
    built, nm, zi, since, novel = [], 0, 0, 0, []

    def known(kind, n):
        if zi >= len(zs) or zs[zi][1] != kind:
            return False
        t, vp, d = by_id[zs[zi][2]]
        return vp == p and (int(d) == n if kind == "D" else d[:n] == seq[r:r + n]) and int(zs[zi][0]) == since

    for n, op in ops:
        if op == "M":
            for _ in range(n):
                if p in subs:
                    assert subs[p] == loc.bb[p] != seq[r]
                    if zi < len(zs) and zs[zi][1] == "S" and by_id[zs[zi][2]][1] == p:
                        assert by_id[zs[zi][2]][0] == "single" and int(zs[zi][0]) == since
                        built.append(by_id[zs[zi][2]][2])
                        zi += 1
                        since = 0
                    else:
                        built.append(seq[r])            # an unknown edit: nothing to rebuild it from
                        nm += 1
                        since += 1
                else:
                    built.append(loc.bb[p])
                    since += 1
                p += 1
                r += 1
        elif op == "D":
            assert dels[p] == loc.bb[p:p + n]
            if known("D", n):
                zi += 1
                since = 0
            else:
                novel.append((n, r))
                nm += n
            p += n
        else:
            if known("I", n):
                built.append(by_id[zs[zi][2]][2][:n])
                zi += 1
                since = n
            else:
                novel.append((n, r))
                built.append(seq[r:r + n])              # novel bases: nothing to rebuild them from
                nm += n
                since += n
            r += n
    assert zi == len(zs) and "".join(built) == seq and nm == int(tags["NM"]) and q == p and len(f[10]) == len(seq)
    assert len(novel) == 1 and 0 < novel[0][1] < len(seq)
    return novel[0]


@pytest.mark.parametrize("key", gc.INPUT_IDS + ["basic_with_errors-0", "synth-err1"])
def test_every_gapped_record_rebuilds_its_read(key):
    d, texts, me, gap = gc.inputs()[key] if key in gc.inputs() else align_cases.inputs()[key] + (gc.GAP,)
    loci = align_ref.loci_from_dicts(*d)
    st, n, bases = {}, 0, 0
    for line in gc.records(gc.ref_text(key, stats=st)):
        if gc.is_gapped(line):
            g, _ = _verify_gapped(line, loci)
            assert 0 < g <= min(gap, me) and int(line.split("\t")[11][5:]) <= me
            n += 1
            bases += g
        else:
            _verify(line, loci)
    assert (n, bases) == (st["gapped"], st["bases"]) and st["searched"] >= n
    assert n > 0 or key in ("ghand1", "basic_with_errors-0", "synth-err1")


def test_random_loci_rebuild_their_reads():
    """The seeded random loci: every seed gives a gapped record, and every gapped record rebuilds its read."""
    for seed, loci, reads, me, gap, text, st in gc.random_cases():
        n = 0
        for line in gc.records(text):
            if gc.is_gapped(line):
                g, _ = _verify_gapped(line, loci)
                assert g <= min(gap, me)
                n += 1
        assert n == st["gapped"] > 0, seed
    assert len(gc.random_cases()) == 60


def test_the_leftmost_gap_in_a_repeat_on_both_strands():
    """The homopolymer read and its reverse complement give the same record: the gap is leftmost on the BACKBONE's strand."""
    _, loci, reads, me, gap, _ = gc.hand_cases()[4]
    for name, s in reads:
        fw = _fields(align_gap_ref.align_text(loci, [[(name, s, None)]], me, gap=gap))
        rv = _fields(align_gap_ref.align_text(loci, [[(name, align_ref.revcomp(s), None)]], me, gap=gap))
        assert len(fw) == len(rv) == 1 and int(rv[0][1]) == 16 and fw[0][2:6] == rv[0][2:6] and fw[0][9:] == rv[0][9:]


def test_the_host_front_end_keeps_gapped_records():
    """hgx_parse_sam (host route) takes the gap statement's text of the synth pairs with novel indels without a decline and keeps
    every pair whose records are both written with NM <= num_editdist: more pairs than from align_ref's text."""
    from hisatgenotype_amd import engine, locus as hl, synth
    loc = synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11)
    pl = hl.PackedLocus.from_synth(loc)
    pairs, want = {}, {}
    for gap in (0, gc.GAP):
        text = gc.ref_text("novel-err0", gap=gap)
        recs = [l.split("\t") for l in gc.records(text)]
        assert all(int(f[11][5:]) <= 2 for f in recs)
        names = [f[0] for f in recs if f[-1] == "YT:Z:CP" and f[-2] == "NH:i:1"]
        want[gap] = len(set(n for n in names if names.count(n) == 2))
        with engine.test_switches(front="host"):
            b = pl.parse_sam(text, num_editdist=2, simulation=False)
        assert engine.front_last() == (0, 0)
        pairs[gap] = b.n_pairs
        b.close()
    assert sum(gc.is_gapped(l) for l in gc.records(gc.ref_text("novel-err0"))) >= 10
    assert pairs[gc.GAP] > pairs[0] > 0
    assert pairs == want
