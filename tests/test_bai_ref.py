"""tests/bai_ref.py pinned by brute force: for a grid of regions over a small coordinate-sorted BAM, every record that overlaps the
region (full decode + bamio.region_hit) lies inside a chunk the query returns, and every chunk begins and ends on a record boundary."""
import pytest

from hisatgenotype_amd import bamio

import bai_cases
import bai_ref


@pytest.fixture(scope="module", params=bai_cases.BLOCK_SIZES)
def fixture(request, tmp_path_factory):
    path = bai_cases.write_fixture(tmp_path_factory.mktemp("bai_ref"), request.param)
    refs, recs, v_end = bai_ref.read(path)
    return path, refs, recs, v_end, bai_ref.parse(bai_ref.build(path))


def test_binning_scheme():
    assert bai_ref.reg2bin(0, 1) == 4681 and bai_ref.reg2bin(0, 1 << 14) == 4681 and bai_ref.reg2bin(0, (1 << 14) + 1) == 585
    assert bai_ref.reg2bin((1 << 29) - 1, 1 << 29) == 37448 and bai_ref.reg2bin(0, 1 << 29) == 0
    for beg, end in ((0, 1), (16383, 16385), (5 << 14, 8 << 14), (123456, 123457), (0, 1 << 29)):
        bins = bai_ref.reg2bins(beg, end)
        assert len(set(bins)) == len(bins) and max(bins) <= 37448
        for b, e in ((beg, beg + 1), (end - 1, end), (beg, end)):              # whatever lies inside the region sits in one of its bins
            assert bai_ref.reg2bin(b, e) in bins


def test_every_overlapping_record_lies_in_a_chunk(fixture):
    path, refs, recs, v_end, ix = fixture
    starts = {r["voff"] for r in recs} | {v_end}
    n_placed = sum(1 for r in recs if r["ref"] >= 0)
    assert ix["n_no_coor"] == len(recs) - n_placed == 3
    assert ix["refs"][2] == {"bins": {}, "ioffset": []}                        # a reference without records
    for R in ix["refs"]:
        for chunks in R["bins"].values():
            for beg, end in chunks:
                assert beg < end and beg in starts and end in starts           # record boundaries
    W = bai_cases.W
    grid = [(0, b, b + n) for b in (0, 1, W - 51, W - 50, W - 1, W, W + 1, 2 * W - 1, 2 * W, 5 * W - 101, 5 * W - 100, 7 * W, 9 * W + 4, 9 * W + 5, 150000, 199999)
            for n in (1, 50, 700, W, 3 * W)]
    grid += [(1, b, b + n) for b in (0, 199, 200, 39800, 49999) for n in (1, 250, 50000)] + [(2, 0, 1000), (0, 0, 1 << 29), (1, 0, 1 << 29)]
    for ref, beg, end in grid:
        chunks = bai_ref.query(ix, ref, beg, end)
        reg = ("", refs[ref][0], beg, end - 1)
        want = [r for r in recs if r["ref"] >= 0 and bamio.region_hit(reg, r["rname"], r["pos"], r["end"] - 1)]
        for r in want:
            assert any(b <= r["voff"] < e for b, e in chunks), (ref, beg, end, r)
    # the spliced record sits in a parent bin and begins three windows before the region that finds it
    spliced = [r for r in recs if r["qname"] == "spliced"][0]
    assert bai_ref.reg2bin(spliced["pos"], spliced["end"]) < 4681 and spliced["pos"] >> 14 == 4 and (spliced["end"] - 1) >> 14 == 7
    got = bai_ref.records_in(path, bai_ref.query(ix, 0, 7 * W + 10, 7 * W + 20))
    assert spliced["voff"] in {r["voff"] for r in got}


def test_parse_and_variants(fixture):
    path, refs, recs, v_end, ix = fixture
    data = bai_ref.build(path)
    assert bai_ref.dump(bai_ref.parse(data)) == data
    for cut in range(0, len(data) - 8, 97):
        with pytest.raises(ValueError):
            bai_ref.parse(data[:cut])
    assert bai_ref.parse(data[:-8])["n_no_coor"] is None
    for variant in (bai_ref.with_pseudo_bin(data), bai_ref.with_zero_linear(data), bai_ref.without_no_coor(data)):
        v = bai_ref.parse(variant)
        for ref, beg, end in ((0, bai_cases.W, bai_cases.W + 600), (0, 0, 1 << 29), (1, 100, 4000)):
            want = {r["voff"] for r in bai_ref.records_in(path, bai_ref.query(ix, ref, beg, end)) if r["ref"] == ref and r["pos"] < end and r["end"] > beg}
            got = {r["voff"] for r in bai_ref.records_in(path, bai_ref.query(v, ref, beg, end))}
            assert want <= got
