"""The name-order stage of the device front end at its edges: the order check that also collects the varying bits of the names, the
sort keys made of them (packed words, or 8-byte chunks under front=name_chunks), the stable radix passes, the task key.  One
implementation serves BAM records and SAM text lines, so every case runs on both.  The expectation is never the stage itself: the
host front end's batch (pl.parse_alignment_file) and the dict statement of tests/region_ref.py ("region after region, then a stable
sort by name") fed to pl.parse_sam, compared array for array.  A few hundred records per case, forced onto the device with
front=device."""
import random
import string

import pytest

from hisatgenotype_amd import bamio, capi, engine

import region_ref
from test_gpu_region_lists import _by_coordinate, _chrom, _edge_lists, _lines, _loci, _pls, _spans, _want, _write_sam, same_batch, same_many

pytestmark = pytest.mark.gpu
SWITCHES = ("device", "device,name_chunks")
KINDS = ("bam", "sam")
ALL = ["6"]                                      # one region that keeps every record: filter, scan and compaction run


def _grouped(n, shift=0):
    """`n` records of the name-grouped stream (mates side by side), `shift` records into it."""
    lines = list(_lines()["A"][shift:shift + n])
    assert len(lines) == n
    return lines


def _rename(lines, name_of):
    """Read k of `lines` (consecutive records of one name: the mates) gets the name name_of(k)."""
    out, k, prev = [], -1, None
    for l in lines:
        name, rest = l.split("\t", 1)
        if name != prev:
            k, prev = k + 1, name
        out.append(name_of(k) + "\t" + rest)
    return out


def _n_reads(lines):
    return len({l.split("\t", 1)[0] for l in lines})


def _names(lines):
    return [l.split("\t", 1)[0] for l in lines]


def _write(path, kind, lines, newline_at_end=True):
    if kind == "bam":
        bamio.write_bam_native(path, ("\n".join(lines) + "\n").encode(), [_chrom()])       # (file order = the order of `lines`)
    elif newline_at_end:
        _write_sam(path, lines, [_chrom()])
    else:
        with open(path, "w") as f:
            f.write("@SQ\tSN:%s\tLN:%d\n" % _chrom() + "\n".join(lines))


def _check(tmp_path, kind, lines, regions=ALL, newline_at_end=True, host_too=True):
    capi.set_device(0)
    pl, loc, left = _pls()[0], _loci()[0], _spans()["A"][0]
    path = str(tmp_path / ("names." + kind))
    _write(path, kind, lines, newline_at_end)
    want = _want(pl, lines, regions, left)
    if host_too:
        same_batch(pl.parse_alignment_file(path, regions, base_locus=left), want, len(loc.backbone))
    for sw in SWITCHES:
        with engine.test_switches(front=sw):
            dev = pl.parse_alignment_file_dev(path, regions, base_locus=left)
            route = engine.front_last()
        print(kind, sw, "records", len(lines), "route", route)
        same_batch(dev.to_host(), want, len(loc.backbone))
        assert route == (2, 0), (kind, sw, route)


LENGTHS = [1, 2, 63, 64, 65, 256, 257]


@pytest.mark.parametrize("n,inverted", [(n, False) for n in LENGTHS] + [(n, True) for n in LENGTHS if n > 1])
@pytest.mark.parametrize("kind", KINDS)
def test_list_lengths(tmp_path, kind, n, inverted):
    """Lists around a wavefront (64) and a workgroup (256) of the order check, in name order and with ONE inversion, between the last
    two records: for 65 and 257 records the one lane that sees it is the first of a wavefront / of a workgroup."""
    # (an odd shift for even n: the stream then ends ... mate | mate | first mate of the last read, so the last two records are two reads)
    lines = _grouped(n, shift=1 - n % 2)
    last = _n_reads(lines) - 1
    lines = _rename(lines, lambda k: "read_%07d" % (10 * k + (85 if inverted and k == last else 100)))
    names = _names(lines)
    out_of_order = [i for i in range(1, n) if names[i].encode() < names[i - 1].encode()]
    assert out_of_order == ([n - 1] if inverted else []), out_of_order
    _check(tmp_path, kind, lines)


def test_a_last_line_without_a_newline(tmp_path):
    """SAM text whose only record line ends with the file."""
    _check(tmp_path, "sam", _rename(_grouped(1), lambda k: "read_%07d" % k), newline_at_end=False)


@pytest.mark.parametrize("kind", KINDS)
def test_a_varying_bit_that_one_lane_sees(tmp_path, kind):
    """Two groups of names that differ in ONE byte of the second 8-byte chunk (p / q), counters behind it that overlap; the q group
    comes first and has 64 records, so the only neighbours that differ in that byte are records 63 | 64 -- the first lane of the
    second wavefront.  Without that bit in the key the counters alone would interleave the groups."""
    lines = _grouped(64 + 40)
    assert _n_reads(lines[:64]) == 32 and lines[63].split("\t", 1)[0] != lines[64].split("\t", 1)[0]
    lines = _rename(lines, lambda k: "grp_name%s%04d" % ("q", k) if k < 32 else "grp_name%s%04d" % ("p", k - 32))
    names = _names(lines)
    assert [i for i in range(1, len(names)) if names[i][8] != names[i - 1][8]] == [64]
    _check(tmp_path, kind, lines)


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_edges(tmp_path, kind):
    """Names of exactly 8 and 9 bytes with the same first 8 (a name that is a prefix of another comes first; one chunk against two),
    the longer one first in the file; and names of at most 8 bytes alone (one chunk: the keys are the names, nothing is packed)."""
    lines = _grouped(120)
    n = _n_reads(lines)
    lines89 = _rename(lines, lambda k: "nm%06d" % (k // 2) + ("x" if k % 2 == 0 else ""))
    assert {len(x) for x in _names(lines89)} == {8, 9}
    _check(tmp_path, kind, lines89)
    rng = random.Random(3)
    short = set()
    while len(short) < n:
        short.add("".join(rng.choice("ab") for _ in range(rng.randint(1, 8))))
    short = sorted(short)
    rng.shuffle(short)
    assert any(a != b and b.startswith(a) for a in short for b in short)
    _check(tmp_path, kind, _rename(lines, lambda k: short[k]))


@pytest.mark.parametrize("kind", KINDS)
def test_more_than_64_varying_bits(tmp_path, kind):
    """Random 24-character names: more varying bits than one packed word holds (two sort passes, least significant word first)."""
    rng = random.Random(4)
    lines = _grouped(300)
    names = ["".join(rng.choice(string.ascii_letters + string.digits) for _ in range(24)) for _ in range(_n_reads(lines))]
    assert len(set(names)) == len(names)
    varying = 0
    for c in range(24):
        x = 0
        for name in names:
            x |= ord(name[c]) ^ ord(names[0][c])
        varying += bin(x).count("1")
    assert varying > 64
    _check(tmp_path, kind, _rename(lines, lambda k: names[k]))


@pytest.mark.parametrize("kind", KINDS)
def test_the_longest_names(tmp_path, kind):
    """254-byte names (the longest a BAM record holds; 32 chunks, the most the packed key covers) with a common 240-byte prefix."""
    rng = random.Random(5)
    lines = _grouped(100)
    names = ["L" * 240 + "".join(rng.choice(string.ascii_lowercase + string.digits) for _ in range(14)) for _ in range(_n_reads(lines))]
    assert len(set(names)) == len(names) and all(len(x) == 254 for x in names)
    _check(tmp_path, kind, _rename(lines, lambda k: names[k]))
    if kind == "sam":
        # one byte more than a QNAME may have: the device's line table declines such text in front of the name-order stage, the call
        # takes the host's line table instead and still ends on the record kernels -- (2, 0) and the host front end's batch
        _check(tmp_path, kind, _rename(lines, lambda k: "L" + names[k]))


@pytest.mark.parametrize("kind", KINDS)
def test_equal_names_keep_region_order_then_file_order(tmp_path, kind):
    """A coordinate-sorted file and two regions that share records: the records of one name come out region after region, file order
    inside a region (every sort pass is stable over the region-major list).  (The host front end raises on SAM TEXT that holds a line twice --
    "not enough values to unpack" on the second copy -- so for SAM text the dict statement alone is the expectation, as in test_partition_edges.)"""
    n = 200
    lines = _by_coordinate(_lines()["A"])[:n]
    regions = _edge_lists(lines, n, 1024)[2]
    both = [i for i, m in enumerate(region_ref.mask(lines, regions)) if m == [0, 1]]
    assert {63, 64, n - 1} <= set(both) and len(region_ref.kept(lines, regions)) == n + len(both)
    _check(tmp_path, kind, lines, regions, host_too=(kind == "bam"))


def test_tasks(tmp_path):
    """Two files with the same read names, one sorted by coordinate and one name-grouped, as two tasks of one pass (name sort over
    both, then the stable task key), and as an AlignmentSet: there the stage reads the set's own index list, which must still be
    what it was for the second call."""
    capi.set_device(0)
    pl, left = _pls()[0], _spans()["A"][0]
    grouped = _rename(_grouped(300), lambda k: "read_%07d" % k)
    paths = [str(tmp_path / "by_coordinate.bam"), str(tmp_path / "grouped.bam")]
    bamio.write_bam_native(paths[0], ("\n".join(grouped) + "\n").encode(), [_chrom()], sort_by_coordinate=True)
    bamio.write_bam_native(paths[1], ("\n".join(grouped) + "\n").encode(), [_chrom()])
    by_pos = bamio.read_bam(paths[0])
    assert _names(by_pos) != _names(grouped) and sorted(_names(by_pos)) == _names(grouped)
    per_file = [pl.parse_alignment_file(p, ALL, base_locus=left) for p in paths]
    same_batch(per_file[0], _want(pl, by_pos, ALL, left), len(_loci()[0].backbone))
    host = engine.ManyBatch(pl, per_file)
    for sw in SWITCHES:
        with engine.test_switches(front=sw):
            dev = engine.ManyBatch.from_files(pl, paths, regions=["6", "6"], base_locus=left)
            assert engine.front_last() == (2, 0), (sw, engine.front_last())
            same_many(dev, host)
            with engine.AlignmentSet(paths) as aset:
                assert aset.resident
                aset.route([ALL])
                assert aset.kept == [[300, 300]]
                first = engine.ManyBatch.from_set(pl, aset, 0, base_locus=left)
                assert engine.front_last() == (2, 0) and engine.front_last_bytes() == 0
                second = engine.ManyBatch.from_set(pl, aset, 0, base_locus=left)
                assert engine.front_last() == (2, 0) and engine.front_last_bytes() == 0
            same_many(first, host)
            same_many(second, first)
