"""tests/region_ref.py -- "region after region, duplicates kept" in plain Python -- held to bamio.read_bam(path, regions) and to the
native host reader (typing.read_alignment_text(native=True): its stable name sort over that list) at the rule's edges.  These pin the
specification the device front end's region-list kernels are held to (tests/test_gpu_region_lists.py)."""
import sys

import pytest

import hisatgenotype_amd  # noqa: F401
from hisatgenotype_amd import bamio

import region_ref

htyping = sys.modules["hisatgenotype_amd.typing"]
SEQ = "ACGT" * 5
REFS = [("6", 100000), ("A*BACKBONE", 4000), ("HLA:1-5", 3000), ("HLA", 3000)]


def rec(name, rname, pos, cigar="20M", flag=0):
    return "%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*" % (name, flag, rname, pos, cigar, SEQ)


def edge_records():
    """Names descend so that the stable name sort has to move every record."""
    rows = [
        ("6", 1000, "20M", 0),          # [999, 1018]: in 6:1000-1100 only
        ("6", 1050, "20M", 0),          # in both overlapping spans
        ("6", 1150, "20M", 0),          # in 6:1060-1200 only
        ("6", 1300, "20M", 0),          # in neither
        ("6", 980, "20M", 0),           # end0 = 998 = left0 - 1 of 6:1000-1100: out
        ("6", 981, "20M", 0),           # end0 = 999 = left0: in
        ("6", 1101, "20M", 0),          # pos0 = 1100 = right0 + 1 of 6:1000-1100: out of it (in 6:1060-1200)
        ("6", 1100, "20M", 0),          # pos0 = 1099 = right0: in
        ("6", 1201, "20M", 0),          # pos0 = 1200 > right0 of 6:1060-1200: out
        ("6", 990, "5M10D5M", 0),       # deletion counts: [989, 1008]
        ("6", 990, "5M3I5M5S", 0),      # insertions and clips do not: [989, 998]: out
        ("6", 900, "10M200N10M", 0),    # a spliced record spanning both
        ("6", 1045, "10=5X5M", 0),      # = and X consume the reference: [1044, 1063]
        ("6", 1005, "*", 4),            # unmapped with a position: one base
        ("6", 999, "20M", 4),           # unmapped: the CIGAR does not count, one base at 998: out
        ("6", 1070, "*", 0),            # empty CIGAR: one base
        ("*", 0, "*", 4),               # refID -1: in no region
        ("A*BACKBONE", 10, "20M", 0),
        ("A*BACKBONE", 3000, "20M", 0),
        ("HLA:1-5", 700, "20M", 0),     # a whole name that contains ':' digits
        ("HLA", 3, "20M", 0),           # ... and the reference its span reading names
        ("HLA", 700, "20M", 0),
    ]
    n = len(rows)
    return [rec("r%03d" % (n - i), rn, pos, cg, fl) for i, (rn, pos, cg, fl) in enumerate(rows)]


REGION_LISTS = [
    ["6:1000-1100", "6:1060-1200"],                     # two overlapping spans on one reference
    ["6:1060-1200", "6:1000-1100"],                     # ... in the other order
    ["6:1000-1100", "A*BACKBONE"],                      # the genotype-genome pair
    ["6:1000-1100", "B*BACKBONE"],                      # ... with a backbone the file does not have
    ["B*BACKBONE", "6:1000-1100"],
    ["HLA:1-5"],                                        # the whole name and the span reading, side by side
    ["HLA:1-5", "HLA", "6"],
    ["6", "6:1,000-1,100", "6:1100", "6:-1000"],        # a whole reference, commas, open ends
    ["6:1000-1100"] * 8,                                # every record of the span in every region
    ["nothing:1-5", "nothing"],                         # regions that keep nothing
    ["6:1000-1100", "6:1060-1200", "A*BACKBONE", "HLA", "HLA:1-5", "6:1-10", "6:1201", "6:990-999", "A*BACKBONE:1-20"],   # nine
]
HEADERS = [REFS, [REFS[2], REFS[0], REFS[3], REFS[1]], REFS[:1] + REFS[2:]]       # orders; the last lacks A*BACKBONE


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("region_ref")
    out = []
    for k, refs in enumerate(HEADERS):
        have = {n for n, _ in refs}
        lines = [l for l in edge_records() if l.split("\t")[2] in have or l.split("\t")[2] == "*"]
        bam, sam = str(d / ("h%d.bam" % k)), str(d / ("h%d.sam" % k))
        bamio.write_bam(bam, "\n".join(lines) + "\n", refs)
        with open(sam, "w") as f:
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "\n".join(lines) + "\n")
        out.append((bam, sam, lines))
    return out


def test_edges_by_hand():
    lines = edge_records()
    m = region_ref.mask(lines, ["6:1000-1100", "6:1060-1200"])
    assert m[:9] == [[0], [0, 1], [1], [], [], [0], [1], [0, 1], []]
    assert m[9] == [0] and m[10] == [] and m[11] == [0, 1] and m[12] == [0, 1]
    assert m[13] == [0] and m[14] == [] and m[15] == [0, 1] and m[16] == []
    m = region_ref.mask(lines, ["HLA:1-5", "HLA"])
    assert m[19] == [0] and m[20] == [0, 1] and m[21] == [1]
    assert region_ref.parse("HLA:1-5") == ("HLA:1-5", "HLA", 0, 4)
    assert region_ref.parse("A*BACKBONE")[1] is None and region_ref.parse("6:,")[1] is None and region_ref.parse("6:-")[1] is None
    assert region_ref.parse("6:1,000-")[1:] == ("6", 999, region_ref.OPEN_END)
    kept = region_ref.kept(lines, ["6:1000-1100"] * 8)
    assert len(kept) == 8 * region_ref.kept_counts(lines, ["6:1000-1100"])[0]
    assert region_ref.kept(lines, None) == lines and region_ref.kept(lines, ["nothing"]) == []


@pytest.mark.parametrize("regions", REGION_LISTS, ids=lambda r: "+".join(r)[:40])
def test_held_to_bamio(files, regions):
    for bam, _, lines in files:
        assert bamio.read_bam(bam) == lines
        assert bamio.read_bam(bam, regions) == region_ref.kept(lines, regions)
        assert bamio.read_bam(bam, "\n".join(regions)) == region_ref.kept(lines, regions)


@pytest.mark.parametrize("regions", REGION_LISTS, ids=lambda r: "+".join(r)[:40])
def test_held_to_the_native_host_reader(files, regions):
    for bam, sam, lines in files:
        want = "".join(l + "\n" for l in region_ref.name_sorted(region_ref.kept(lines, regions))).encode()
        for path in (bam, sam):
            assert htyping.read_alignment_text(path, regions, native=True) == want, path
            assert htyping.read_alignment_text(path, regions, native=False) == want, path
