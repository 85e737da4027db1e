"""The linear route's kernels (csrc/hgx_linear.hip; k_rec_heads / k_rec_gstart of csrc/hgx_records.hpp) on records shaped as
real aligners write them and at their edges (tests/linear_cases.py), against the plain statement (tests/linear_ref.py): counts
and classes as ordered lists, and the route the call reports -- (2, 0) for a case that is to stay on the device, so that no
fallback can pass for the kernel, (0, code) for a case the kernels are to decline.  Integers and strings only: no tolerance."""
import pytest

import linear_cases as LC
from hisatgenotype_amd import capi
from hisatgenotype_amd.locus import PackedLocus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def packed():
    capi.set_device(0)
    pls = {}

    def get(kind):
        if kind not in pls:
            pls[kind] = PackedLocus.from_synth(LC.locus(kind))
        return pls[kind]
    yield get
    for pl in pls.values():
        pl.close()


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_device_route_equals_the_statement(family, packed, tmp_path):
    tally = {}
    for case in LC.cases():
        if case["family"] == family:
            route = LC.check(case, packed(case["locus"]), "device", tmp_path)
            tally[route] = tally.get(route, 0) + 1
    print("family %s: %s" % (family, ", ".join("%d cases (route, decline) = %s" % (n, r) for r, n in sorted(tally.items(), reverse=True))))


@pytest.mark.parametrize("s", LC.SIZES)
def test_scanned_sizes_at_the_scan_edges(s, packed, tmp_path):
    """Lines, kept records, groups and classes at s: see linear_cases.sized_sam."""
    for shape in LC.SHAPES:
        case = LC.sam_case("size_%s_%d" % (shape, s), "sizes", LC.sized_sam(shape, s), kind="hla")
        assert LC.check(case, packed("hla"), "device", tmp_path) == (2, 0)
