"""tests/route_ref.py (the plain-Python statement of an alignment set's routing) pinned on hand-made BAM files at the edges of the
overlap rule: region "R1:101-200" is [left0, right0] = [100, 199] in 0-based coordinates."""
from hisatgenotype_amd import bamio

import route_ref

REFS = [("R1", 1000), ("R2", 1000)]
SEQ10 = "ACGTACGTAC"


def _rec(name, flag, rname, pos1, cigar, seq=SEQ10):
    return "\t".join([name, str(flag), rname, str(pos1), "60", cigar, "*", "0", "0", seq, "*"])


# name, flag, rname, 1-based pos, cigar                            0-based span
EDGE = [
    _rec("ends_at_left0", 0, "R1", 92, "10M"),                     # [91, 100]: its last base is left0
    _rec("ends_before_left0", 0, "R1", 91, "10M"),                 # [90, 99]
    _rec("starts_at_right0", 0, "R1", 200, "10M"),                 # [199, 208]: its first base is right0
    _rec("starts_after_right0", 0, "R1", 201, "10M"),              # [200, 209]
    _rec("inside", 0, "R1", 150, "4M2D4M2I"),                      # D counts, I does not: [149, 158]
    _rec("skip_reaches", 0, "R1", 50, "5M45N5M"),                  # N counts: [49, 103]
    _rec("clip_does_not_reach", 0, "R1", 86, "5M5S"),              # S does not: [85, 89]
    _rec("unmapped_nowhere", 4, "*", 0, "*"),                      # refID -1
    _rec("unmapped_placed_in", 4, "R1", 100, "10M"),               # FLAG 4: one base, [99, 99]
    _rec("unmapped_placed_at", 4, "R1", 101, "10M"),               # ... [100, 100]
    _rec("empty_cigar_at_right0", 0, "R1", 200, "*"),              # span 1: [199, 199]
    _rec("empty_cigar_after", 0, "R1", 201, "*"),                  # [200, 200]
    _rec("other_reference", 0, "R2", 150, "10M"),
]


def _names(lines):
    return [l.split("\t")[0] for l in lines]


def _bam(tmp_path, name, lines, refs=REFS):
    p = str(tmp_path / name)
    bamio.write_bam(p, "\n".join(lines) + "\n", refs)
    return p


def test_overlap_rule_at_its_edges(tmp_path):
    p = _bam(tmp_path, "edge.bam", EDGE)
    (got,), = route_ref.route([p], ["R1:101-200"])
    assert _names(got) == ["ends_at_left0", "starts_at_right0", "inside", "skip_reaches", "unmapped_placed_at", "empty_cigar_at_right0"]
    assert got == bamio.read_bam(p, ["R1:101-200"])                  # (the decoder's own region filter agrees)
    assert route_ref.kept_counts([p], ["R1:101-200"]) == [[6]]


def test_whole_reference_unmapped_and_no_filter(tmp_path):
    p = _bam(tmp_path, "edge.bam", EDGE)
    whole, other, none, everything = route_ref.route([p], ["R1", "R2", "R3", ""])
    assert _names(whole[0]) == [n for n in _names(EDGE) if n not in ("unmapped_nowhere", "other_reference")]
    assert _names(other[0]) == ["other_reference"]
    assert none[0] == []                                             # a reference no header names
    assert _names(everything[0]) == _names(EDGE)                     # no region: nothing is filtered, not even refID -1
    for region, got in (("R1", whole), ("R2", other), ("R3", none)):
        assert got[0] == bamio.read_bam(p, [region])
    assert everything[0] == bamio.read_bam(p)


def test_open_ended_spans_and_a_record_in_several_slots(tmp_path):
    p = _bam(tmp_path, "edge.bam", EDGE)
    regions = ["R1:201", "R1:-100", "R1:101-200", "R1:101-200"]
    kept = route_ref.route([p], regions)
    assert _names(kept[0][0]) == ["starts_at_right0", "starts_after_right0", "empty_cigar_after"]      # [200, inf)
    assert _names(kept[1][0]) == ["ends_at_left0", "ends_before_left0", "skip_reaches", "clip_does_not_reach", "unmapped_placed_in"]     # [0, 99]
    assert kept[2] == kept[3] and len(kept[2][0]) == 6               # the same region asked twice: both slots get the records
    assert "skip_reaches" in _names(kept[1][0]) and "skip_reaches" in _names(kept[2][0])
    for region, got in zip(regions, kept):
        assert got[0] == bamio.read_bam(p, [region])


def test_per_file_order_and_headers_in_different_orders(tmp_path):
    a = _bam(tmp_path, "a.bam", EDGE)
    b = _bam(tmp_path, "b.bam", list(reversed(EDGE)), refs=list(reversed(REFS)))      # R2 is refID 0 here
    c = _bam(tmp_path, "c.bam", [l for l in EDGE if "\tR1\t" not in l])               # a file without a record of R1
    kept = route_ref.route([a, b, c], ["R1:101-200", "R2"])
    assert _names(kept[0][1]) == list(reversed(_names(kept[0][0]))) and kept[0][2] == []
    assert [_names(v) for v in kept[1]] == [["other_reference"]] * 3
    assert route_ref.kept_counts([a, b, c], ["R1:101-200", "R2"]) == [[6, 6, 0], [1, 1, 1]]
