"""The alignment reader's hand-overs and line tables on a CPU (csrc/hgx_bam.cpp): tools/reader_host_check.cpp -- the reader's host units
linked into a program of their own, with callbacks that record what they are given -- is run over the cases of
tools/reader_host_check.py, and parts of its record are held to the Python statements of the formats the project already has:
region_ref (what a region list keeps), bamio (the BAM and BGZF formats) and a stable sort by name.  What the GPU tests see only through
the kernels' results -- what the host TELLS the device -- is pinned here."""
import os
import re
import struct
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bai_cases  # noqa: E402
import region_ref  # noqa: E402
import reader_host_check as rhc  # noqa: E402
from hisatgenotype_amd import bamio, build as hb  # noqa: E402

INT64_MAX = (1 << 63) - 1
BAM_HANDOVERS = ("index, splice taken", "bgzf, inflate taken", "bgzf, inflate refused", "raw bam, handed over")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reader_host"))
    # (the library's own objects of the reader's units are linked where the build left them fresh, not compiled again)
    fresh = all(hb._object_fresh(os.path.join(rhc.CSRC, u + ".cpp")) for u in rhc.UNITS)
    exe = rhc.build(os.path.join(d, "reader_host_check"), sanitize=False, objects=fresh)
    cases = rhc.parse(rhc.run(exe, d, rhc.write_cases(d, big=False)))
    lines = list(bai_cases.sam_lines())
    return {"dir": d, "cases": cases, "lines": lines, "stream": rhc.inflated(os.path.join(d, "fx.bam"))}


def field(case, prefix, key):
    """The value of `key=` on the case's first line that starts with `prefix`."""
    for line in case:
        if line.startswith(prefix):
            m = re.search(r"(?:^|\s)%s=(\[[^\]]*\]|\S*)" % re.escape(key), line)
            assert m, (prefix, key, line)
            return m.group(1)
    raise AssertionError((prefix, case))


def line(case, prefix):
    return [l for l in case if l.startswith(prefix)][0]


def crc(data):
    return "%08x" % (zlib.crc32(data) & 0xffffffff)


def table_crc(lines):
    """The line table's checksum as the program makes it: per line its length, name length, key (the name's first 8 bytes, big endian,
    zero padded) and CRC-32."""
    rows = []
    for l in lines:
        b = l.encode()
        name = b.split(b"\t", 1)[0]
        rows.append("%d %d %016x %s\n" % (len(b), len(name), int.from_bytes(name[:8].ljust(8, b"\0"), "big"), crc(b)))
    return crc("".join(rows).encode())


def header_length(stream):
    p = 12 + struct.unpack_from("<i", stream, 4)[0]
    for _ in range(struct.unpack_from("<i", stream, p - 4)[0]):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    return p


def test_regions_of_a_handed_over_bam_are_region_refs(dump):
    """ref_action and the spans of every region, on every route that hands a BAM over, against tests/region_ref.py."""
    refs = [n for n, _ in bai_cases.REFS]
    for route in BAM_HANDOVERS:
        for sname, regs in rhc.region_sets().items():
            case = dump["cases"]["%s / %s" % (route, sname)]
            if sname == "too many" or (regs is None and route.startswith("index")):
                continue                                   # (no hand-over: below / no region list, no index)
            if sname == "unknown" and route.startswith("index"):
                assert field(case, "deferred", "on") == "0"                # (the index names no block: nothing to hand over)
                continue
            assert field(case, "deferred", "on") == "1" and field(case, "deferred", "text") == "0", (route, sname)
            assert field(case, "deferred", "regions") == str(len(regs or []))
            if regs is None:
                assert field(case, "  keep-all", "action") == "1" * len(refs)
            for g, r in enumerate(regs or []):
                whole, name, left0, right0 = region_ref.parse(r)
                want = "".join("1" if n == whole else "2" if n == name else "0" for n in refs)
                assert field(case, "  region %d" % g, "action") == want, (route, sname, g)
                if name is not None:
                    assert int(field(case, "  region %d" % g, "left0")) == left0
                    assert int(field(case, "  region %d" % g, "right0")) == (INT64_MAX if right0 == region_ref.OPEN_END else right0)


def test_regions_of_a_handed_over_text_are_region_refs(dump):
    for sname, regs in rhc.region_sets().items():
        case = dump["cases"]["sam text, handed over / %s" % sname]
        if sname == "too many":
            continue
        assert field(case, "deferred", "on") == "1" and field(case, "deferred", "text") == "1"
        for g, r in enumerate(regs or []):
            whole, name, left0, right0 = region_ref.parse(r)
            assert field(case, "  region %d" % g, "whole") == "[%s]" % whole and field(case, "  region %d" % g, "name") == "[%s]" % (name or "")
            if name is not None:
                assert (int(field(case, "  region %d" % g, "left0")), int(field(case, "  region %d" % g, "right0"))) == (left0, right0)
        with open(os.path.join(dump["dir"], "fx.sam"), "rb") as f:
            assert field(case, "binary", "raw_crc") == crc(f.read())


def test_more_regions_than_the_device_takes_are_never_handed_over(dump):
    for route in rhc.ROUTES:
        case = dump["cases"]["%s / too many" % route]
        assert field(case, "rc", "rc") == "0" and field(case, "deferred", "on") == "0", route
        assert not any(l.startswith("cb inflate_dev") or l.startswith("cb splice_dev") for l in case), route


def test_body0_and_the_handed_over_stream(dump):
    """body0 = the header's length; the stream handed over (or inflated from the table the callback got) = the file's inflated bytes."""
    stream, body0 = dump["stream"], header_length(dump["stream"])
    for route in ("bgzf, inflate taken", "bgzf, inflate refused", "raw bam, handed over"):
        case = dump["cases"][route + " / none"]
        assert int(field(case, "deferred", "body0")) == body0, route
        assert field(case, "binary", "ref_names") == "[%s]" % ",".join(n for n, _ in bai_cases.REFS)
        assert int(field(case, "binary", "raw_bytes")) == len(stream)
        if route != "bgzf, inflate taken":
            assert field(case, "deferred", "on_device") == "0" and field(case, "binary", "raw_crc") == crc(stream), route
        if route.startswith("bgzf"):
            assert field(case, "cb inflate_dev", "total") == str(len(stream))
            assert field(case, "  inflate_dev", "inflates") == "1" and field(case, "  inflate_dev", "bytes") == crc(stream)
    taken = dump["cases"]["bgzf, inflate taken / none"]
    assert field(taken, "deferred", "on_device") == "1" and field(taken, "binary", "raw") == "null"
    assert line(taken, "events") == "events= comp_early inflate_dev return"
    refused = dump["cases"]["bgzf, inflate refused / none"]                # (comp_sync behind comp_early and before the return)
    assert line(refused, "events") == "events= comp_early inflate_dev on_raw comp_sync return"
    assert field(refused, "cb on_raw", "tiles") == "1"
    sam = dump["cases"]["bgzipped sam text"]                          # (never offered to the device)
    assert not any("comp_early" in l or "inflate_dev" in l for l in sam)


def bam_records(data):
    """(name, flag, reference id, pos0) of the records of an inflated stream that begins at a record."""
    out, q = [], 0
    while q < len(data):
        bs = struct.unpack_from("<i", data, q)[0]
        rid, pos, l_rn, _mapq, _bin, _ncig, flag = struct.unpack_from("<iiBBHHH", data, q + 4)
        out.append((data[q + 36:q + 36 + l_rn - 1].decode(), flag, rid, pos))
        q += 4 + bs
    assert q == len(data)
    return out


def test_index_route_splices_a_superset_of_the_region(dump):
    names = [n for n, _ in bai_cases.REFS]
    regs = rhc.region_sets()["span"]
    case = dump["cases"]["index, splice taken / span"]
    assert field(case, "index ", "used") == "1" and field(case, "index ", "why") == "0", line(case, "index ")
    assert field(case, "deferred", "on_device") == "1" and field(case, "deferred", "body0") == "0"
    part_file = [f for f in os.listdir(dump["dir"]) if f.startswith("parts_")]
    assert len(part_file) == 2                              # (splice_dev was asked on two routes: it took the blocks, it refused them)
    want = set()
    for l in region_ref.kept(dump["lines"], regs):
        f = l.split("\t")
        want.add((f[0], int(f[1]), names.index(f[2]), int(f[3]) - 1))
    assert want
    for pf in part_file:
        with open(os.path.join(dump["dir"], pf), "rb") as f:
            data = f.read()
        got = bam_records(data)
        assert want <= set(got) and len(got) < len(dump["lines"])
    assert field(case, "  dense", "bytes") == field(case, "binary", "raw_bytes")
    refused = dump["cases"]["index, splice refused / span"]           # the host inflates the same segments, header in front
    assert int(field(refused, "binary", "raw_bytes")) == int(field(case, "binary", "raw_bytes")) + header_length(dump["stream"])
    assert field(refused, "deferred", "on") == "1" and field(refused, "deferred", "on_device") == "0"
    empty = dump["cases"]["index that names no block"]
    assert field(empty, "index ", "used") == "1" and field(empty, "deferred", "on") == "0" and field(empty, "lines", "n") == "0"


def test_line_tables_are_the_python_readers_in_name_order(dump):
    fx = os.path.join(dump["dir"], "fx.bam")
    for sname, regs in rhc.region_sets().items():
        want = region_ref.name_sorted(bamio.read_bam(fx, regs))
        assert want == region_ref.name_sorted(region_ref.kept(dump["lines"], regs))
        for route in ("bgzf, host text", "sam text, host"):
            case = dump["cases"]["%s / %s" % (route, sname)]
            assert (field(case, "lines", "n"), field(case, "lines", "table")) == (str(len(want)), table_crc(want)), (route, sname)
        for route in ("bgzf, host walk", "raw bam, host walk", "index, no defer_walk"):      # (binary records: their count)
            assert field(dump["cases"]["%s / %s" % (route, sname)], "lines", "n") == str(len(want)), (route, sname)
    one = field(dump["cases"]["chain in ranges, fx.bam, 1 threads"], "lines", "table")
    assert one == table_crc(region_ref.name_sorted(dump["lines"]))
    for nt in (2, 3, 7):
        assert field(dump["cases"]["chain in ranges, fx.bam, %d threads" % nt], "lines", "table") == one
    for nt in (1, 2, 3, 7):
        assert field(dump["cases"]["chain in ranges, decoy.bam, %d threads" % nt], "lines", "n") == "7"
