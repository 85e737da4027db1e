"""Read extraction on the device (csrc/hgx_extract.hip) against the fixtures recorded from the real reference, the host route and
the spec (tests/extract_ref.py)."""
import pytest

import extract_cases
import extract_ref
from hisatgenotype_amd import engine, extract

pytestmark = pytest.mark.gpu
NAMES = extract_ref.fixture_names()
REFS = [(c, 100000000) for c in ["1", "2", "6", "7", "18", "22", "X"]]
# what a BAM cannot hold: a record with fewer than 11 columns, a tag value that is no integer (bamio refuses both)
NOT_IN_BAM = {"error_short_line", "error_tag_value"}


@pytest.mark.parametrize("name", NAMES)
def test_sam_fixture_on_device(name, tmp_path):
    fx = extract_ref.load(name)
    with engine.test_switches(front="device"):
        got = extract_cases.run_fixture(fx, tmp_path)
    extract_cases.check_against_fixture(fx, got)
    stats = got[4]
    if fx["exception"] is None and not fx["pre_existing"]:
        assert stats["route"] == 2 and stats["chunks_host"] == 0, stats
        assert stats["records"] == sum(1 for l in fx["sam"].splitlines() if not l.startswith("@"))


@pytest.mark.parametrize("name", [n for n in NAMES if n not in NOT_IN_BAM])
def test_bam_fixture_on_device(name, tmp_path, monkeypatch):
    fx = extract_ref.load(name)
    if name == "reverse_with_n":
        # BAM's 4-bit codes have no lower case: acgt are stored as N, so the expectation is the spec's on that text
        fx = dict(fx, sam=fx["sam"].replace("acgt", "NNNN"))
        files, exc, _ = extract_cases.spec_files(fx)
        fx["files"] = files
        assert exc is None
    from hisatgenotype_amd import bamio
    monkeypatch.setattr(bamio, "write_bam", lambda path, sam, _w=bamio.write_bam: _w(path, sam, REFS))
    with engine.test_switches(front="device"):
        got = extract_cases.run_fixture(fx, tmp_path, alignment="bam")
    extract_cases.check_against_fixture(fx, got)
    if fx["exception"] is None and not fx["pre_existing"]:
        assert got[4]["route"] == 2 and got[4]["chunks_host"] == 0, got[4]


@pytest.mark.parametrize("name", NAMES)
def test_host_route_same_bytes(name, tmp_path):
    fx = extract_ref.load(name)
    with engine.test_switches(front="host"):
        got = extract_cases.run_fixture(fx, tmp_path)
    extract_cases.check_against_fixture(fx, got)
    if got[4] is not None:
        assert got[4]["route"] == 0


def _feed(regions, families, a, data, sizes):
    """Feed `data` in blocks of the given sizes (cycled); -> ({(family, mate): bytes}, stats)."""
    ex = extract.Extractor(regions, families, a["aligner"], a["paired"], a["simulation"], a["fastq"])
    out = {(f, m): [] for f in range(len(families)) for m in range(2 if a["paired"] else 1)}
    p, k = 0, 0
    try:
        while p < len(data):
            n = sizes[k % len(sizes)]
            ex.feed(data[p:p + n], last=p + n >= len(data))
            p += n
            k += 1
            for key in out:
                out[key].append(ex.take(*key))
        return {key: b"".join(v) for key, v in out.items()}, ex.stats()
    finally:
        ex.close()


def test_chunked_feed_is_the_single_feed():
    fx = extract_ref.load("big_random")
    a = fx["args"]
    dbl = []
    regions = extract_ref.region_table(fx["locus"], dbl)
    data = fx["sam"].encode()
    lines = data.split(b"\n")
    first_len = len(lines[0]) + 1
    recs = [l for l in lines if l and not l.startswith(b"@")]
    # a block that ends exactly on a group boundary: behind the last record of the 40th group
    cut_at, seen, off = None, 0, 0
    for i, l in enumerate(lines[:-1]):
        off += len(l) + 1
        if l.startswith(b"@"):
            continue
        if l.split(b"\t")[0] != lines[i + 1].split(b"\t")[0]:
            seen += 1
            if seen == 40:
                cut_at = off
                break
    with engine.test_switches(front="device"):
        whole, st = _feed(regions, dbl, a, data, [len(data)])
        assert st["route"] == 2 and st["chunks_device"] == 1
        expect = {extract_ref.file_name(fx["base"], dbl[f], m, True): t.decode() for (f, m), t in whole.items()}
        assert expect == fx["files"]
        for sizes in ([first_len + 17], [1000], [4096, 333], [65536], [cut_at, 7777], [len(data) // 2 + 5], [50001, 1]):
            got, st = _feed(regions, dbl, a, data, sizes)
            assert got == whole, sizes
            assert st["records"] == len(recs) and st["chunks_host"] == 0, (sizes, st)
    with engine.test_switches(front="host"):
        got, st = _feed(regions, dbl, a, data, [4096, 333])
        assert got == whole and st["chunks_device"] == 0


def test_generated_stream_above_the_gate():
    """>= 200 000 records, no switch: the gate sends it to the device; device == host == spec."""
    fx = extract_ref.load("big_random")
    a = fx["args"]
    dbl = []
    regions = extract_ref.region_table(fx["locus"], dbl)
    big_regions = [(f, c, l * 1000, r * 1000) for f, c, l, r in regions]
    data = extract.synth_stream(101000, big_regions, seed=7, hit_fraction=0.02, read_len=60)
    n_rec = data.count(b"\n")
    assert n_rec >= 200000
    dev, st = _feed(big_regions, dbl, a, data, [len(data)])
    assert st["route"] == 2 and st["records"] == n_rec, st
    dev2, st2 = _feed(big_regions, dbl, a, data, [8 << 20])
    assert st2["route"] == 2 and st2["chunks_device"] > 1 and dev2 == dev
    with engine.test_switches(front="host"):
        host, sth = _feed(big_regions, dbl, a, data, [len(data)])
    assert sth["route"] == 0 and sth["groups"] == st["groups"] and sth["written"] == st["written"]
    assert host == dev
    texts, exc = extract_ref.extract(data.decode(), big_regions, dbl, a["aligner"], a["paired"], a["simulation"], a["fastq"])
    assert exc is None
    assert {(dbl[f], m): t.decode() for (f, m), t in dev.items()} == texts
    assert sum(st["written"].values()) > 1000
