"""The plain-Python statement of "both tiers in one call" (tests/align_rescue_ref.py) pinned: on the hand-written records
(tests/align_rescue_cases.py); against the two tiers' own statements, read by read, with the cost rule recomputed here; against
align_ref on every input of its own suites (only the mate fields of a pair with a newly aligned mate may differ); by the verifiers
that rebuild SEQ from a clipped and from a gapped record; and through the host front end, which must keep rescued pairs.  No GPU;
native code only in the front-end test."""
import pytest

import align_cases
import align_clip_ref
import align_gap_ref
import align_ref
import align_rescue_cases as rc
import align_rescue_ref as rr
from test_align_clip_ref import _verify_clipped
from test_align_gap_ref import _fields, _own, _verify_gapped
from test_align_ref import _verify


def _plain(reads):
    return [[(n, s, None) for n, s in reads]]


@pytest.mark.parametrize("k", range(rc.N_HAND))
def test_hand_made_records(k):
    title, loci, reads, max_edits, gap, clip, expected, searched = rc.hand_cases()[k]
    st = {}
    got = rr.align_text(loci, _plain(reads), max_edits, gap=gap, clip=clip, stats=st)
    assert got == align_cases.expected_text(loci, reads, expected), title
    assert (st["clip"]["searched"], st["gap"]["searched"]) == searched
    cig = [e[4] for e in expected if e is not None]
    assert st["clip"]["clipped"] == sum("S" in c for c in cig) and st["gap"]["gapped"] == sum("D" in c or "I" in c for c in cig)


def test_neither_fixed_order_of_the_tiers_gives_the_hand_records():
    """The one-base overhang under the gap statement alone is a novel insertion; the deletion three bases from the end under the clip
    statement alone loses a base and spends two mismatches: the rule picks the other one each time."""
    _, loci, reads, me, gap, clip, _, _ = rc.hand_cases()[0]
    g = align_gap_ref.align_read(loci, reads[0][1], me, gap)
    assert g is not None and g[0][0] == 1 and g[3] == (98, align_gap_ref.INS, 1)
    _, loci, reads, me, gap, clip, _, _ = rc.hand_cases()[2]
    c = align_clip_ref.align_read(loci, reads[0][1], me, clip)
    assert c is not None and (c[3], c[4], c[0][0]) == (0, 1, 2)
    # the tie at cost 2: both exist, the clip is written
    _, loci, reads, me, gap, clip, _, _ = rc.hand_cases()[1]
    c, g = align_clip_ref.align_read(loci, reads[0][1], me, clip), align_gap_ref.align_read(loci, reads[0][1], me, gap)
    assert rr.cost_clip(c) == rr.cost_gap(g) == 2 and not rr.gap_wins(c, g)


def test_cost_1_skips_the_gap_search_and_cost_2_runs_it():
    loc = rc.locus()
    bb = loc.bb
    x = rc._not(bb[399])
    for seq, ran in ((bb[301:400] + bb[399], ["clip"]), (bb[301:400] + x, ["clip"]), (bb[302:400] + x + x, ["clip", "gap"]), (bb[200:300], [])):
        got = []
        rr.align_read([loc], seq, 2, rc.GAP, rc.CLIP, got)
        assert got == ran


def test_a_clipped_and_a_gapped_mate_make_a_concordant_pair():
    loci, m1, m2 = rc.pair_case()
    reads = [[(n, s, None) for n, s in m1], [(n, s, None) for n, s in m2]]
    before = _fields(align_ref.align_text(loci, reads))
    assert [(f[0], int(f[1])) for f in before] == [("cp", 99), ("cp", 147)]
    for kw, flag, cigar in ((dict(clip=rc.CLIP), 73, "3S97M"), (dict(gap=rc.GAP), 153, "50M1D50M")):
        alone = _fields((align_clip_ref if "clip" in kw else align_gap_ref).align_text(loci, reads, **kw))
        assert [(f[0], int(f[1]), f[5], f[-1]) for f in alone[:1]] == [("up", flag, cigar, "YT:Z:UP")] and alone[1:] == before
    after = _fields(rr.align_text(loci, reads, gap=rc.GAP, clip=rc.CLIP))
    assert [(f[0], int(f[1]), f[5], f[-1]) for f in after] == [("up", 99, "3S97M", "YT:Z:CP"), ("up", 147, "50M1D50M", "YT:Z:CP"),
                                                             ("cp", 99, "100M", "YT:Z:CP"), ("cp", 147, "100M", "YT:Z:CP")]
    assert after[0][3] == "1" and after[0][6:9] == ["=", "401", "0"] and after[1][3] == "401" and after[1][6:9] == ["=", "1", "0"]
    assert after[2:] == before


def _record_of(statement_text, name_and_seq):
    """The own columns of the single-end record of one read in a tier's statement text (None: unaligned)."""
    f = _fields(statement_text)
    assert len(f) <= 1
    return _own(f[0]) if f else None


@pytest.mark.parametrize("key", rc.INPUT_IDS + ["basic_with_errors-0", "synth-err1"])
def test_every_rescued_record_is_one_tiers_record_chosen_by_the_cost_rule(key):
    """Per read without an end-to-end alignment: the record is, up to the mate fields, the clip statement's or the gap statement's for
    that read alone, by costs recomputed here from the two results."""
    d, texts, me, gap, clip = rc._input(key)
    loci = align_ref.loci_from_dicts(*d)
    files = [align_ref.read_records(t) for t in texts]
    got = {}
    for f in _fields(rc.ref_text(key).decode()):
        got.setdefault((f[0], f[9]), _own(f))
    n_clip = n_gap = 0
    for m, recs in enumerate(files):
        for name, seq, qual in recs:
            s = seq.upper()
            if align_ref.align_read(loci, s, me) is not None:
                continue
            one = [[(name, seq, qual)]]
            c, g = align_clip_ref.align_read(loci, s, me, clip), align_gap_ref.align_read(loci, s, me, gap)
            cost_c = None if c is None else c[3] + c[4] + c[0][0]
            cost_g = None if g is None else g[0][0]
            if cost_g is not None and (cost_c is None or cost_g < cost_c):
                want = _record_of(align_gap_ref.align_text(loci, one, me, gap=gap), None)
                n_gap += 1
            elif cost_c is not None:
                want = _record_of(align_clip_ref.align_text(loci, one, me, clip=clip), None)
                n_clip += 1
            else:
                want = None
            have = [v for k, v in got.items() if k[0] == name and k[1] in (s, align_ref.revcomp(s))]
            if want is None:
                assert not have, name
            else:
                want[1] |= (0x1 | (0x40 if m == 0 else 0x80)) if len(files) == 2 else 0
                assert want in have, name
    st = {}
    rc.ref_text(key, stats=st)
    assert (st["clip"]["clipped"], st["gap"]["gapped"]) == (n_clip, n_gap)


@pytest.mark.parametrize("key", [k for k in align_cases.INPUT_IDS])
def test_align_refs_inputs_change_only_in_mate_fields(key):
    """Under rescue = (16, 32) every record align_ref writes is written again; it differs only in FLAG 0x8 / 0x20 / 0x2, RNEXT, PNEXT
    and YT, and only where its mate is written now and was not before.  Every other record is new and clipped or gapped."""
    before = _fields(align_cases.ref_text(key).decode())
    after = _fields(rc.ref_text(key).decode())
    paired = len(align_cases.inputs()[key][1]) == 2
    if not paired:                                                            # (single-end files may repeat a name: the record's SEQ tells)
        before, after = ([[f[0] + "/" + f[9]] + f[1:] for f in x] for x in (before, after))
    old = {(f[0], int(f[1]) & 0xC0): f for f in before}
    new = {(f[0], int(f[1]) & 0xC0): f for f in after}
    assert len(old) == len(before) and len(new) == len(after)
    assert [k for k in new if k in old] == list(old)                          # all kept, in order
    mate_of = {}
    if paired:
        r1, r2 = (align_ref.read_records(x) for x in align_cases.inputs()[key][1])
        for (n1, _, _), (n2, _, _) in zip(r1, r2):
            mate_of[(n1, 0x40)], mate_of[(n2, 0x80)] = (n2, 0x80), (n1, 0x40)
    for k, f in new.items():
        if k not in old:
            line = "\t".join(f)
            assert rc.is_clipped(line) != rc.is_gapped(line)                  # one of them, never both
            continue
        mate = mate_of.get(k)
        if f != old[k]:
            assert paired and mate in new and mate not in old, f
            assert _own(f) == _own(old[k])
            assert int(old[k][1]) & 0x8 and old[k][-1] == "YT:Z:UP" and not int(f[1]) & 0x8 and f[-1] in ("YT:Z:CP", "YT:Z:DP")
        else:
            assert not (paired and mate in new and mate not in old)
    st = {}
    rc.ref_text(key, stats=st)
    assert st["clip"]["clipped"] + st["gap"]["gapped"] == len(after) - len(before)


@pytest.mark.parametrize("key", rc.INPUT_IDS + ["basic_with_errors-0", "synth-err1"])
def test_every_record_rebuilds_its_read(key):
    d, texts, me, gap, clip = rc._input(key)
    loci = align_ref.loci_from_dicts(*d)
    st, n = {}, dict(clipped=0, cbases=0, gapped=0, gbases=0)
    for line in rc.records(rc.ref_text(key, stats=st)):
        assert int(line.split("\t")[11][5:]) <= me
        if rc.is_clipped(line):
            assert not rc.is_gapped(line)                                     # never both in one record
            c = _verify_clipped(line, loci)
            assert 0 < c <= clip
            n["clipped"] += 1
            n["cbases"] += c
        elif rc.is_gapped(line):
            g, _ = _verify_gapped(line, loci)
            assert 0 < g <= min(gap, me)
            n["gapped"] += 1
            n["gbases"] += g
        else:
            _verify(line, loci)
    assert (n["clipped"], n["cbases"]) == (st["clip"]["clipped"], st["clip"]["bases"])
    assert (n["gapped"], n["gbases"]) == (st["gap"]["gapped"], st["gap"]["bases"])
    assert st["gap"]["searched"] <= st["clip"]["searched"] and n["clipped"] + n["gapped"] <= st["clip"]["searched"]


def test_the_random_seeds_have_the_properties_they_were_chosen_for():
    """Every seed writes a clipped and a gapped record; at least ten differ from chaining the tiers gap first and at least ten from
    clip first; every record rebuilds its read and none carries both a clip and a gap."""
    assert len(rc.random_cases()) == len(rc.RANDOM_SEEDS) == 40
    ngf, ncf = [], []
    for seed, loci, reads, me, gap, clip, text, st in rc.random_cases():
        assert st["clip"]["clipped"] > 0 and st["gap"]["gapped"] > 0, seed
        ch = rc.choices(loci, reads, me, gap, clip)
        assert sum(c[0] == "clip" for c in ch) == st["clip"]["clipped"] and sum(c[0] == "gap" for c in ch) == st["gap"]["gapped"]
        if any(c[0] != c[1] for c in ch):
            ngf.append(seed)
        if any(c[0] != c[2] for c in ch):
            ncf.append(seed)
        for line in rc.records(text):
            if rc.is_clipped(line):
                _verify_clipped(line, loci)
            elif rc.is_gapped(line):
                _verify_gapped(line, loci)
    assert ngf == rc.NOT_GAP_FIRST and ncf == rc.NOT_CLIP_FIRST and len(ngf) >= 10 and len(ncf) >= 10


def test_the_host_front_end_keeps_rescued_pairs():
    """hgx_parse_sam (host route) takes the statement's text of the mixed synth pairs without a decline and keeps every pair whose
    records are both written: more than from either tier's text."""
    from hisatgenotype_amd import engine, locus as hl, synth
    import align_clip_cases as cc
    import align_gap_cases as gc
    d, texts, me, gap, clip = rc.inputs()["mixed-err1"]
    loci = align_ref.loci_from_dicts(*d)
    files = [align_ref.read_records(t) for t in texts]
    pl = hl.PackedLocus.from_synth(synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11))
    pairs = {}
    for which, text in (("rescue", rc.ref_text("mixed-err1")), ("clip", align_clip_ref.align_text(loci, files, me, clip=clip).encode()),
                        ("gap", align_gap_ref.align_text(loci, files, me, gap=gap).encode())):
        recs = [l.split("\t") for l in rc.records(text)]
        names = [f[0] for f in recs if f[-1] == "YT:Z:CP" and f[-2] == "NH:i:1"]
        want = len(set(n for n in names if names.count(n) == 2))
        with engine.test_switches(front="host"):
            b = pl.parse_sam(text, num_editdist=2, simulation=False)
        assert engine.front_last() == (0, 0)
        pairs[which] = b.n_pairs
        assert b.n_pairs == want, which
        b.close()
    assert pairs["rescue"] > pairs["clip"] > 0 and pairs["rescue"] > pairs["gap"] > 0
