"""The plain-Python statement of the clip tier (tests/align_clip_ref.py) pinned: on hand-made loci whose records are written out by
hand (tests/align_clip_cases.py), against align_ref on every input of its own suites (only the mate fields of a pair with a newly
aligned mate may differ), by a verifier that rebuilds SEQ from a clipped record, and through the host front end, which must keep
clipped records.  The statement offers no pruned form (the enumeration is exhaustive), so there is no shortcut to compare.  No GPU;
native code only in the front-end test."""
import re

import pytest

import align_cases
import align_clip_cases as cc
import align_clip_ref
import align_ref
from test_align_ref import _verify


@pytest.mark.parametrize("k", range(7))
def test_hand_made_loci(k):
    title, loci, reads, max_edits, clip, expected = cc.hand_cases()[k]
    plain = [[(n, s, None) for n, s in reads]]
    got = align_clip_ref.align_text(loci, plain, max_edits, clip=clip)
    assert got == align_cases.expected_text(loci, reads, expected), title
    # every read of these cases needs the tier: with clip = 0 none is written, and the text is align_ref's
    assert align_clip_ref.align_text(loci, plain, max_edits, clip=0) == align_ref.align_text(loci, plain, max_edits)
    assert align_ref.align_text(loci, plain, max_edits).count("\n") == len(loci)


def test_the_overhang_budget_is_the_total():
    """clip = 21 takes 10 + 11 at the two ends of the short locus, not 10 + 12; clip = 1 takes only the one-base overhangs."""
    _, loci, reads, me, _, _ = cc.hand_cases()[1]
    plain = [[(n, s, None) for n, s in reads]]
    assert align_clip_ref.align_text(loci, plain, me, clip=21).count("\n") == len(loci)
    assert "10S60M12S" in align_clip_ref.align_text(loci, plain, me, clip=22)
    _, loci, reads, me, _, _ = cc.hand_cases()[0]
    text = align_clip_ref.align_text(loci, [[(n, s, None) for n, s in reads]], me, clip=1)
    assert [l.split("\t")[5] for l in text.split("\n") if l and l[0] != "@"] == ["1S99M", "99M1S"]


def _fields(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("@")]


def test_a_clipped_mate_turns_up_into_cp():
    loci, m1, m2 = cc.pair_case()
    reads = [[(n, s, None) for n, s in m1], [(n, s, None) for n, s in m2]]
    before = _fields(align_ref.align_text(loci, reads))
    after = _fields(align_clip_ref.align_text(loci, reads, clip=cc.CLIP))
    assert [(f[0], int(f[1]), f[-1]) for f in before] == [("up", 73, "YT:Z:UP"), ("cp", 99, "YT:Z:CP"), ("cp", 147, "YT:Z:CP")]
    assert [(f[0], int(f[1]), f[5], f[-1]) for f in after] == [("up", 99, "100M", "YT:Z:CP"), ("up", 147, "80M20S", "YT:Z:CP"),
                                                             ("cp", 99, "100M", "YT:Z:CP"), ("cp", 147, "100M", "YT:Z:CP")]
    assert after[0][6:9] == ["=", "421", "0"] and after[1][3] == "421" and after[1][6:9] == ["=", "251", "0"]
    assert after[2:] == before[1:]


def _own(f):
    """The columns of a record that do not depend on its mate."""
    return [f[0], int(f[1]) & ~(0x2 | 0x8 | 0x20)] + f[2:6] + f[8:-1]


@pytest.mark.parametrize("key", [k for k in align_cases.INPUT_IDS])
def test_align_refs_inputs_change_only_in_mate_fields(key):
    """Under clip = 32 every record align_ref writes is written again; it differs only in FLAG 0x8 / 0x20 / 0x2, RNEXT, PNEXT and YT,
    and only where its mate is written now and was not before.  Every other record is new and clipped."""
    before = _fields(align_cases.ref_text(key).decode())
    after = _fields(cc.ref_text(key).decode())
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
            assert "S" in f[5]
            continue
        mate = mate_of.get(k)
        if f != old[k]:
            assert paired and mate in new and mate not in old, f
            assert _own(f) == _own(old[k])
            assert int(old[k][1]) & 0x8 and old[k][-1] == "YT:Z:UP" and not int(f[1]) & 0x8 and f[-1] in ("YT:Z:CP", "YT:Z:DP")
        else:
            assert not (paired and mate in new and mate not in old)
    st = {}
    cc.ref_text(key, stats=st)
    assert st["clipped"] == len(after) - len(before)


def _verify_clipped(line, loci):
    """test_align_ref's verifier on the aligned part: the S ops carry nothing to rebuild, so they are cut off CIGAR, SEQ and QUAL
    after their lengths are checked."""
    f = line.split("\t")
    m = re.fullmatch(r"(?:(\d+)S)?((?:\d+[MID])+)(?:(\d+)S)?", f[5])
    assert m, f[5]
    cl, cr = int(m.group(1) or 0), int(m.group(3) or 0)
    inner = re.findall(r"(\d+)([MID])", m.group(2))
    assert inner[0][1] == "M" and (inner[-1][1] == "M" or cr == 0)            # no indel at a clip boundary
    assert cl + cr + sum(int(n) for n, op in inner if op in "MI") == len(f[9]) == len(f[10])
    f[5] = m.group(2)
    f[9], f[10] = f[9][cl:len(f[9]) - cr], f[10][cl:len(f[10]) - cr]
    _verify("\t".join(f), loci)
    return cl + cr


@pytest.mark.parametrize("key", cc.INPUT_IDS + ["basic_with_errors-0", "synth-err1"])
def test_every_clipped_record_rebuilds_its_read(key):
    d, texts, me, clip = cc.inputs()[key] if key in cc.inputs() else align_cases.inputs()[key] + (cc.CLIP,)
    loci = align_ref.loci_from_dicts(*d)
    st, n, bases = {}, 0, 0
    for line in cc.records(cc.ref_text(key, stats=st)):
        if cc.is_clipped(line):
            c = _verify_clipped(line, loci)
            assert 0 < c <= clip and int(line.split("\t")[11][5:]) <= me
            n += 1
            bases += c
        else:
            _verify(line, loci)
    assert n > 0 and (n, bases) == (st["clipped"], st["bases"]) and st["searched"] >= n


def test_both_strands_and_a_tie_between_anchors():
    """A read inside a homopolymer-flanked repeat reaches two alignments that tie in everything but clipL; the smaller clipL is
    written (the tie-break the statement adds behind the list)."""
    bb = align_cases._bb(120, 100) + "A" * 40
    loc = align_ref.Locus("T1*BACKBONE", bb, [])
    # 30 bases + 30 A + 9 junk on the right end: every shift of the A-run inside the backbone's 40 A gives clip 9 ... but the left
    # part pins the diagonal, so exactly one alignment exists; its reverse complement gives the same record with flag 16
    read = bb[70:100] + "A" * 30 + "C" + align_cases._bb(121, 8)
    for s, flag in ((read, 0), (align_ref.revcomp(read), 16)):
        f = _fields(align_clip_ref.align_text([loc], [[("t", s, None)]], 0, clip=cc.CLIP))
        assert len(f) == 1 and (int(f[0][1]), f[0][3], f[0][5], f[0][9]) == (flag, "71", "60M9S", read)
    # all-A read longer than the run, hanging over the right end: anchors on many diagonals, ties broken by pos0 then clipL
    loc2 = align_ref.Locus("T2*BACKBONE", "A" * 40, [])
    a = align_clip_ref.align_read([loc2], "A" * 44, 0, cc.CLIP)
    key, end, nh, cl, cr = a
    assert (key[5], end, nh, cl, cr) == (0, 40, 1, 0, 4)


def test_the_host_front_end_keeps_clipped_records():
    """hgx_parse_sam (host route) takes the clip statement's text of the overhang pairs without a decline, keeps more pairs than
    from align_ref's text, and a clipped record's aligned part stands in the kept trace."""
    from hisatgenotype_amd import engine, locus as hl
    loc, d, m1, m2 = cc.overhang_pairs(0.0)
    pl = hl.PackedLocus.from_synth(loc)
    traces, pairs = {}, {}
    for clip in (0, cc.CLIP):
        text = cc.ref_text("overhang-err0", clip=clip)
        with engine.test_switches(front="host"):
            b = pl.parse_sam(text, num_editdist=2, simulation=False, keep_trace=True)
        assert engine.front_last() == (0, 0)
        traces[clip], pairs[clip] = b.trace_text().split("\n"), b.n_pairs
        b.close()
    assert cc.ref_text("overhang-err0", clip=0) == align_ref.align_text(
        align_ref.loci_from_dicts(*d), [[(n, s, None) for n, s in m] for m in (m1, m2)]).encode()
    assert pairs[cc.CLIP] > pairs[0] > 0
    seen = 0
    for line in cc.records(cc.ref_text("overhang-err0")):
        f = line.split("\t")
        m = re.fullmatch(r"(?:\d+S)?(\d+)M(?:\d+S)?", f[5])
        if cc.is_clipped(line) and m and f[11] == "NM:i:0" and f[-1] == "YT:Z:CP" and f[-2] == "NH:i:1" and not any(
                t.startswith("Zs:Z:") for t in f[11:]):
            head = "match:%d:%s\t" % (int(f[3]) - 1, m.group(1))
            assert any(t.startswith(head) for t in traces[cc.CLIP]), head
            seen += 1
    assert seen >= 5
