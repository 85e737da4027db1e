"""The statement of the coordinate order itself (tests/align_resident_ref.py) on hand-written records.  No GPU, no library."""
from align_resident_ref import coordinate_order

HEADER = b"@SQ\tSN:L0\tLN:500\n@SQ\tSN:L1\tLN:500\n@SQ\tSN:L2\tLN:500\n"


def _rec(name, flag, rname, pos, tag=b"x"):
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % pos, b"60", b"4M", b"=", b"1", b"0", b"ACGT", b"IIII", b"NM:i:0", tag]) + b"\n"


def test_mate_two_left_of_mate_one():
    m1, m2 = _rec(b"p", 83, b"L0", 120), _rec(b"p", 163, b"L0", 20)
    assert coordinate_order(HEADER + m1 + m2) == HEADER + m2 + m1


def test_mates_on_loci_two_and_zero():
    m1, m2 = _rec(b"p", 65, b"L2", 5), _rec(b"p", 129, b"L0", 400)
    assert coordinate_order(HEADER + m1 + m2) == HEADER + m2 + m1
    # the locus' place is the header's, not its name's: with the @SQ lines the other way round nothing moves
    rev = b"".join(reversed(HEADER.splitlines(True)))
    assert coordinate_order(rev + m1 + m2) == rev + m1 + m2


def test_positions_are_numbers_not_text():
    a, b = _rec(b"a", 0, b"L1", 10), _rec(b"b", 0, b"L1", 9)
    assert coordinate_order(HEADER + a + b) == HEADER + b + a
    assert coordinate_order(HEADER + b + a) == HEADER + b + a


def test_ties_keep_the_order_they_came_in():
    recs = [_rec(b"same", 0, b"L1", 7, b"t%d" % k) for k in range(5)]
    assert coordinate_order(HEADER + b"".join(recs)) == HEADER + b"".join(recs)
    first = _rec(b"z", 0, b"L0", 300)
    assert coordinate_order(HEADER + b"".join(recs) + first) == HEADER + first + b"".join(recs)


def test_header_untouched_and_alone():
    assert coordinate_order(HEADER) == HEADER
    other = b"@HD\tVN:1.0\n" + HEADER + b"@PG\tID:z\n"
    rec = _rec(b"a", 0, b"L2", 1)
    assert coordinate_order(other + rec) == other + rec
