"""The case table of the linear route's edges (tests/linear_cases.py) on the host route (front=host, no GPU): every case gives
what the plain statement (tests/linear_ref.py) gives on its lines -- counts and classes in dict order, or the exception type --
and damage the statement cannot see raises with the library's message.  This keeps the table honest where there is no GPU and
pins the host route as the finisher of every decline (tests/test_gpu_linear_edges.py runs the same table on the device)."""
import pytest

import linear_cases as LC
from hisatgenotype_amd.locus import PackedLocus


@pytest.fixture(autouse=True)
def _library():
    try:
        from hisatgenotype_amd import capi
        capi.lib()
    except (ImportError, OSError) as e:
        pytest.skip("libhgx.so does not load here: %s" % e)


@pytest.fixture(scope="module")
def packed():
    pls = {}

    def get(kind):
        if kind not in pls:
            pls[kind] = PackedLocus.from_synth(LC.locus(kind))
        return pls[kind]
    yield get
    for pl in pls.values():
        pl.close()


def test_builders_write_what_they_say():
    """The record builder against the project's own BAM reader: a record with CIGAR, aux data of every kind and a long name reads
    back as the printed line that comes with it."""
    import extract_bam_cases as X
    a = LC.alleles("str")
    tags = LC.bowtie2_tags(-7) + [LC.T("XB", "B", ("s", (-300, 2, 3))), LC.T("XF", "f", 1.5), LC.T("XH", "H", "1AE3")]
    pairs = [LC.bam_record("str", "q" * n, 256 * (n & 1), a[n % 3], tags, n_cigar=c, l_seq=l)
             for n, c, l in ((1, 0, 0), (7, 1, 5), (254, 3, 20))] + [LC.bam_record("str", "u", 4, None, l_seq=5)]
    data = X.bgzf(X.header(LC.refs("str")) + b"".join(r for r, _ in pairs), 700)[0]
    assert X.bam_lines(data).encode() == b"".join(l for _, l in pairs)
    assert LC.sam_line("r", "+0", "x", ["AS:i:1", LC.T("NM", 0)], sep=" \t") == " \t".join(
        ["r", "+0", "x", "1", "60", "20M", "*", "0", "0", "ACGT" * 5, "I" * 20, "AS:i:1", "NM:i:0"])


def test_cases_that_are_to_stay_on_the_device_hold_nothing_to_decline():
    for c in LC.cases():
        if not c.get("decline"):
            LC.assert_nothing_to_decline(c)


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_host_route_equals_the_statement(family, packed, tmp_path):
    for case in LC.cases():
        if case["family"] == family:
            LC.check(case, packed(case["locus"]), "host", tmp_path)


@pytest.mark.parametrize("s", LC.SIZES)
def test_sized_inputs_reach_their_sizes_and_the_host_route_agrees(s, packed, tmp_path):
    for shape in LC.SHAPES:
        text = LC.sized_sam(shape, s)
        n = LC.sized_counts(text)
        assert n[LC.SHAPES.index(shape)] == s + (37 if shape == "lines" else 0), (shape, n)
        if shape == "lines":
            assert n[1] == s
        case = LC.sam_case("size_%s_%d" % (shape, s), "sizes", text, kind="hla")
        LC.assert_nothing_to_decline(case)
        LC.check(case, packed("hla"), "host", tmp_path)
