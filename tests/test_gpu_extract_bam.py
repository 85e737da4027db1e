"""Read extraction from a BAM's deflated bytes on the device (csrc/hgx_extract.hip: inflate, record walk, k_ext_bam_records,
k_ext_emit<BAM>): Extractor.feed_bam against the lines `samtools view` prints for the same records through the text route and
the spec (tests/extract_ref.py)."""
import struct

import pytest

import extract_bam_cases as X
import extract_cases
import extract_ref
from hisatgenotype_amd import capi, engine, extract

pytestmark = pytest.mark.gpu


def _block_ends(data):
    ends, off = [], 0
    while off < len(data):
        off += struct.unpack_from("<H", data, off + 16)[0] + 1
        ends.append(off)
    return ends


@pytest.mark.parametrize("name", X.bam_names())
def test_fixture_in_pieces(name):
    """Records and the BAM header straddle blocks; the feeds cut block headers, blocks and records anywhere."""
    fx, regions, fams, expect = X.fixture(name)
    a = fx["args"]
    n_rec = sum(1 for l in fx["sam"].splitlines() if l and not l.startswith("@"))
    for block_size in (300, 4096):
        data = X.sam_to_bam(fx["sam"], block_size)
        ends = _block_ends(data)
        # a block boundary exactly behind the last record of a group: the stream re-blocked with a cut there
        raw = X.inflate_all(data)
        p = len(X.header())
        assert raw[:p] == X.header()
        cuts, prev = [], None
        while p < len(raw):
            bs, l_rn = struct.unpack_from("<i", raw, p)[0], raw[p + 12]
            nm = raw[p + 36:p + 36 + l_rn]
            if prev is not None and nm != prev:
                cuts.append(p)
            prev = nm
            p += 4 + bs
        whole, st, exc, _ = X.run("feed_bam", regions, fams, a, data, [len(data)], front="device")
        assert X.kind(exc) == fx["exception"]
        assert {k: v.decode() for k, v in whole.items()} == expect
        if exc is None:
            assert st["route"] == 2 and st["chunks_host"] == 0 and st["records"] == n_rec, st
        patterns = [[1], [17], [333], [65536], [ends[len(ends) // 2], 1 << 30]]
        for sizes in patterns:
            got, st, exc, _ = X.run("feed_bam", regions, fams, a, data, sizes, front="device")
            assert X.kind(exc) == fx["exception"], (block_size, sizes)
            assert got == whole, (block_size, sizes)
            if exc is None:
                assert st["route"] == 2 and st["chunks_host"] == 0 and st["records"] == n_rec, (block_size, sizes, st)
        if cuts:
            cut = cuts[len(cuts) // 2]
            data2, at = X.bgzf(raw, block_size, cuts=[cut])
            got, st, exc, _ = X.run("feed_bam", regions, fams, a, data2, [at[cut], 1 << 30], front="device")
            assert X.kind(exc) == fx["exception"] and got == whole, (block_size, "group boundary")


def _synth(n_pairs):
    fx = extract_ref.load("big_random")
    dbl = []
    regions = extract_ref.region_table(fx["locus"], dbl)
    big = [(f, c, l * 1000, r * 1000) for f, c, l, r in regions]
    return fx["args"], big, dbl, extract.synth_stream(n_pairs, big, seed=11, hit_fraction=0.05, read_len=50).decode()


@pytest.mark.parametrize("which", ["big_random", "synth", "long_group"])
def test_chunks_carry(which):
    """>= 5 chunks (extract_bam_piece): the carry joins them; a read with 300 records spans more than a chunk."""
    if which == "big_random":
        fx, regions, fams, _ = X.fixture("big_random")
        a, sam = fx["args"], fx["sam"]
    else:
        a, regions, fams, sam = _synth(9500)
        if which == "long_group":
            lines = sam.splitlines(True)
            mid = [l for l in lines if l.split("\t")[2] != "*"][0].split("\t")
            many = "".join("\t".join(["longread", str(0x143 if k else 0x43)] + mid[2:]) for k in range(299)) + "\t".join(["longread", "131"] + mid[2:])
            sam = "".join(lines[:2000]) + many + "".join(lines[2000:4000])
    refs = [(str(i + 1), 200000000) for i in range(22)] + [("X", 200000000)] if which != "big_random" else X.REFS
    data = X.sam_to_bam(sam, 0xff00 if which == "synth" else 2000, refs=refs)
    n_rec = sum(1 for l in sam.splitlines() if l and not l.startswith("@"))
    if which == "synth":
        assert n_rec >= 19000
    want, want_exc = X.spec(sam, regions, fams, a)
    assert want_exc is None
    one, st, exc, _ = X.run("feed_bam", regions, fams, a, data, [len(data)], front="device")
    assert exc is None and st["chunks_device"] == 1 and st["records"] == n_rec and one == want, st
    piece = len(data) // (40 if which == "long_group" else 6)
    with engine.test_switches(extract_bam_piece=str(piece)):
        got, st, exc, _ = X.run("feed_bam", regions, fams, a, data, [len(data)], front="device")
    assert exc is None and st["chunks_device"] > 1 and st["chunks_host"] == 0 and st["records"] == n_rec, st
    assert got == one


@pytest.mark.parametrize("case", X.CASES, ids=[c["name"] for c in X.CASES])
def test_records_assembled_by_hand(case):
    """Bases and qualities, the aux scan, reference ids and damaged input (tests/extract_bam_cases.py: CASES)."""
    X.check_case(case, "device", ([1 << 30], [333], [1]))


def test_device_bytes_are_the_deflated_ones():
    a, regions, fams, sam = _synth(3000)
    refs = [(str(i + 1), 200000000) for i in range(22)] + [("X", 200000000)]
    sam = sam.replace("\n", "\tZZ:Z:" + "A" * 300 + "\n")              # text that deflates well
    data = X.sam_to_bam(sam, refs=refs)
    inflated = len(X.inflate_all(data))
    assert inflated >= 3 * len(data)
    _, st, exc, _ = X.run("feed_bam", regions, fams, a, data, [len(data)], front="device")
    assert exc is None and st["chunks_device"] == 1
    assert engine.front_last()[0] == 2
    assert 0 < engine.front_last_bytes() < inflated


def test_text_and_bam_do_not_mix():
    fx, regions, fams, _ = X.fixture("two_families")
    a = fx["args"]
    data = X.sam_to_bam(fx["sam"])
    for first, second in (("feed", "feed_bam"), ("feed_bam", "feed")):
        ex = extract.Extractor(regions, fams, a["aligner"], a["paired"], a["simulation"], a["fastq"])
        try:
            getattr(ex, first)(fx["sam"].encode() if first == "feed" else data[:100])
            with pytest.raises(capi.HgxError) as e:
                getattr(ex, second)(fx["sam"].encode() if second == "feed" else data[:100])
            assert e.value.code == -1
        finally:
            ex.close()


def test_through_extract_reads(tmp_path, monkeypatch):
    fx = extract_ref.load("big_random")
    from hisatgenotype_amd import bamio
    monkeypatch.setattr(bamio, "write_bam", lambda path, sam, _w=bamio.write_bam: _w(path, sam, X.REFS, block_size=1000))
    monkeypatch.setattr(extract, "FEED_BYTES", 4096)
    with engine.test_switches(front="device"):
        got = extract_cases.run_fixture(fx, tmp_path, alignment="bam")
    extract_cases.check_against_fixture(fx, got)
    assert got[4]["chunks_device"] >= 1 and got[4]["chunks_host"] == 0, got[4]


def test_file_entry_point():
    """hgx_extract_file on BAM files (Extractor.feed_file): blocks of extract_bam_piece through hgx_extract_feed_bam."""
    X.check_file_entry("device")
