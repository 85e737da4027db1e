"""A samtools region LIST of several regions through the device front end (genotype-genome mode: `samtools view F chr:l-r ref_allele`,
typing_core.py:436-444): region mask per record (k_bam_filter / k_sam_line_info), the stable multi-way partition by region
(k_part_counts / k_part_scatter), the stable name sort over it.  Held to tests/region_ref.py ("region after region, duplicates kept")
and to the host front end's batch, array for array, on every entry point: the path call, the resident file, many files in one pass,
the panel set.  Small inputs, forced onto the device with front=device."""
import functools
import os
import struct
import sys
import zlib

import numpy as np
import pytest

import hisatgenotype_amd as hgx
from hisatgenotype_amd import bamio, capi, engine, locus as hl, synth

import region_ref

htyping = sys.modules["hisatgenotype_amd.typing"]
pytestmark = pytest.mark.gpu
GAP = 300
BIG = 1 << 30


def same_batch(a, b, length):
    assert (a.n_reads, a.n_pairs, a.n_pieces, a.n_refs, a.n_mask_u32) == (b.n_reads, b.n_pairs, b.n_pieces, b.n_refs, b.n_mask_u32)
    for k in ("pieces", "masks", "pair_off", "pair_ref"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    na, ca = a.pileup(length)
    nb, cb = b.pileup(length)
    assert np.array_equal(na, nb) and np.array_equal(ca, cb)


def same_many(dev, host):
    assert dev.n_tasks == host.n_tasks
    assert (dev.n_pieces, dev.n_pairs, dev.n_refs, dev.n_reads) == (host.n_pieces, host.n_pairs, host.n_refs, host.n_reads)
    assert dev.pair_base == host.pair_base
    assert dev.task_reads == host.task_reads and dev.task_pieces == host.task_pieces and dev.task_refs == host.task_refs
    a, b = dev.merged(), host.merged()
    for k in ("pieces", "masks", "pair_off", "pair_ref"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


@functools.lru_cache(maxsize=None)
def _loci():
    specs = [("A", 600, 3569, 1300, 0), ("B", 800, 4081, 1500, 5000)]
    return [synth.make_hla_like_locus(gene=g, n_alleles=n, length=ln, n_vars=v, seed=300 + k, var_id_base=base)
            for k, (g, n, ln, v, base) in enumerate(specs)]


@functools.lru_cache(maxsize=None)
def _spans():
    """gene -> (left0, right0) on chromosome 6: spacer, A, spacer, B, spacer."""
    out, at = {}, GAP
    for loc in _loci():
        out[loc.gene] = (at, at + len(loc.backbone) - 1)
        at += len(loc.backbone) + GAP
    return out


def _chrom():
    return ("6", _spans()["B"][1] + GAP + 1)


@functools.lru_cache(maxsize=None)
def _lines(sample=0, n_pairs=1200):
    """gene -> that sample's records on chromosome coordinates (name-grouped, names carry the gene)."""
    out = {}
    for k, loc in enumerate(_loci()):
        left = _spans()[loc.gene][0]
        sam = synth.simulate_sam_fast(loc, synth.pick_sample(loc, 40 + 7 * sample + k), n_pairs + 50 * k, err_rate=0.003, seed=50 + 10 * sample + k)
        rows = []
        for l in sam.split("\n"):
            if l:
                f = l.split("\t")
                f[0], f[2], f[3], f[7] = "%s_%s" % (loc.gene, f[0]), "6", str(int(f[3]) + left), str(int(f[7]) + left)
                rows.append("\t".join(f))
        out[loc.gene] = tuple(rows)
    return out


def _by_coordinate(lines):
    return sorted(lines, key=lambda l: int(l.split("\t")[3]))


def _genome_regions(gene):
    left, right = _spans()[gene]
    return ["6:%d-%d" % (left + 1, right + 1), "%s*BACKBONE" % gene]


def _write_sam(path, lines, refs):
    with open(path, "w") as f:
        f.write("".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "\n".join(lines) + "\n")


def _pls():
    return [hl.PackedLocus.from_synth(loc) for loc in _loci()]


def _want(pl, lines, regions, left):
    """The batch of the list region_ref states: region after region, duplicates kept, the stable name sort over it."""
    return pl.parse_sam("".join(l + "\n" for l in region_ref.name_sorted(region_ref.kept(lines, regions))), base_locus=left)


@pytest.fixture(scope="module")
def wgs(tmp_path_factory):
    """Two loci on chromosome 6 in one coordinate-sorted BAM and one SAM text, as test_genotyping_locus_genotype_genome_mode makes them."""
    d = tmp_path_factory.mktemp("wgs")
    lines = _by_coordinate(_lines()["A"] + _lines()["B"])
    bam, sam = str(d / "wgs.bam"), str(d / "wgs.sam")
    bamio.write_bam_native(bam, ("\n".join(lines) + "\n").encode(), [_chrom()])
    _write_sam(sam, lines, [_chrom()])
    return {"bam": bam, "sam": sam, "lines": lines}


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_path_call(wgs, kind):
    capi.set_device(0)
    path = wgs[kind]
    for pl, loc in zip(_pls(), _loci()):
        regions, left = _genome_regions(loc.gene), _spans()[loc.gene][0]
        host = pl.parse_alignment_file(path, regions, base_locus=left)               # the host front end: reader, lists, sort, stages
        with engine.test_switches(front="host"):
            pl.parse_alignment_file_dev(path, regions, base_locus=left)
            assert engine.front_last() == (0, -1)
        with engine.test_switches(front="device"):
            dev = pl.parse_alignment_file_dev(path, regions, base_locus=left)
            route, sent = engine.front_last(), engine.front_last_bytes()
            with engine.Alignment(path) as al:
                inflated = al.stream_bytes
        print(kind, loc.gene, "route", route, "bytes sent", sent, "stream", inflated)
        same_batch(dev.to_host(), host, len(loc.backbone))
        same_batch(host, _want(pl, wgs["lines"], regions, left), len(loc.backbone))
        assert route == (2, 0), route
        if kind == "bam":
            assert 0 < sent < inflated / 2, (sent, inflated)       # the file travels deflated: no host inflate, no upload of the stream


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_resident_file(wgs, kind):
    capi.set_device(0)
    path = wgs[kind]
    with engine.test_switches(front="device"):
        with engine.Alignment(path) as al:
            assert al.resident
            for pl, loc in zip(_pls(), _loci()):
                regions, left = _genome_regions(loc.gene), _spans()[loc.gene][0]
                got = al.parse_dev(pl, regions, base_locus=left)
                route, sent = engine.front_last(), engine.front_last_bytes()
                assert route == (2, 0) and sent == 0, (route, sent)
                same_batch(got.to_host(), pl.parse_alignment_file_dev(path, regions, base_locus=left).to_host(), len(loc.backbone))


def _edge_lists(lines, n, T):
    """Region lists over the coordinate-sorted records `lines[:n]`: the records from index 63 to index T (or the last) lie in BOTH
    regions of the pair -- a record in two regions on a wavefront boundary (63 | 64) and, past a tile, on a tile boundary (T - 1 | T)."""
    pos = [int(l.split("\t")[3]) for l in lines[:n]]
    pair = ["6:1-%d" % pos[min(n - 1, T)], "6:%d-%d" % (pos[min(n - 1, 63)], BIG)]
    eight = pair + ["NOPE*BACKBONE", "6:1-5", "6", "6:%d" % pos[n // 2], "A*BACKBONE", "6:-%d" % pos[n // 3]]
    return {1: ["6:%d-%d" % (pos[n // 4], pos[3 * n // 4])], 2: pair, 8: eight, "8 x all": ["6"] * 8, 9: eight + ["6:1000-2000"]}


@pytest.mark.parametrize("count", ["63", "64", "65", "T-1", "T", "T+1", "2T+1"])
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_partition_edges(tmp_path, count, kind):
    capi.set_device(0)
    T = engine.AlignmentSet([]).route_tile
    assert T == 1024
    n = {"63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[count]
    lines = _by_coordinate(_lines()["A"])[:n]
    assert len(lines) == n
    left = _spans()["A"][0]
    path = str(tmp_path / ("edge." + kind))
    if kind == "bam":
        bamio.write_bam_native(path, ("\n".join(lines) + "\n").encode(), [_chrom()])
    else:
        _write_sam(path, lines, [_chrom()])
    pl, loc = _pls()[0], _loci()[0]
    for what, regions in _edge_lists(lines, n, T).items():
        kept = region_ref.kept(lines, regions)
        if what == "8 x all":
            assert len(kept) == 8 * n
        if what == 8:
            counts = region_ref.kept_counts(lines, regions)
            assert counts[2] == 0 and counts[3] == 0 and counts[4] == n and counts[6] == 0       # regions that keep nothing, one that keeps all
        if what == 2:
            both = [i for i, m in enumerate(region_ref.mask(lines, regions)) if m == [0, 1]]
            assert {min(n - 1, 63), min(n - 1, 64), min(n - 1, T - 1), min(n - 1, T)} <= set(both)
        want = _want(pl, lines, regions, left)
        with engine.test_switches(front="device"):
            dev = pl.parse_alignment_file_dev(path, regions, base_locus=left)
            route = engine.front_last()
            print(kind, count, what, "kept", len(kept), "route", route)
            same_batch(dev.to_host(), want, len(loc.backbone))
            if what != 9:                                   # (nine regions decline to the per-path call: the host reader's lists)
                assert route == (2, 0), (what, route)
            if kind == "bam":
                # the kept counts, straight from the partition: one slot with this list
                with engine.AlignmentSet([path]) as aset:
                    aset.route([regions])
                    if what != 9:
                        assert aset.kept == [[len(kept)]], what


def test_many_files(tmp_path):
    """Per-file lists of 1, 2 and 3 regions, headers in different orders."""
    capi.set_device(0)
    loc, pl = _loci()[0], _pls()[0]
    left, right = _spans()["A"]
    mid = (left + right) // 2
    refs = [_chrom(), (loc.ref_allele, len(loc.backbone)), ("DECOY", 5000)]
    orders = [[0, 1, 2], [2, 0, 1], [1, 2, 0]]
    lists = [["6:%d-%d" % (left + 1, right + 1)],
             ["6:%d-%d" % (left + 1, mid + 200), "6:%d-%d" % (mid - 200, right + 1)],
             ["6:%d-%d" % (left + 1, mid + 1), loc.ref_allele, "6:%d-%d" % (mid, right + 1)]]
    paths = []
    for f in range(3):
        lines = list(_lines(sample=f, n_pairs=700)["A"]) + ["decoy%d\t0\tDECOY\t%d\t60\t100M\t*\t0\t0\t%s\t*" % (i, 1 + 7 * i, "ACGT" * 25) for i in range(20)]
        paths.append(str(tmp_path / ("s%d.bam" % f)))
        bamio.write_bam_native(paths[-1], ("\n".join(lines) + "\n").encode(), [refs[i] for i in orders[f]], sort_by_coordinate=(f != 1))
    regions = ["\n".join(r) for r in lists]
    # the host front end, file by file (the reader's lists and sort, the host stages), merged
    host = engine.ManyBatch(pl, [pl.parse_alignment_file(p, r, base_locus=left) for p, r in zip(paths, lists)])
    with engine.test_switches(front="device"):
        dev = engine.ManyBatch.from_files(pl, paths, regions=regions, base_locus=left)
        assert engine.front_last() == (2, 0), engine.front_last()
        assert 0 < engine.front_last_bytes() <= sum(os.path.getsize(p) for p in paths) + 4096      # the files, deflated: no stream went up
    same_many(dev, host)
    assert all(n > 0 for n in dev.task_reads)


@pytest.fixture(scope="module")
def set_files(tmp_path_factory):
    """Three files of both loci's records; the first holds exactly one tile of records (a change of file on a tile boundary)."""
    d = tmp_path_factory.mktemp("set")
    T = 1024
    paths, all_lines = [], []
    for f in range(3):
        lines = _by_coordinate(_lines(sample=f, n_pairs=700)["A"] + _lines(sample=f, n_pairs=700)["B"])
        if f == 0:
            lines = lines[:T]
        paths.append(str(d / ("s%d.bam" % f)))
        bamio.write_bam_native(paths[-1], ("\n".join(lines) + "\n").encode(), [_chrom()], sort_by_coordinate=(f != 2))
        all_lines.append(bamio.read_bam(paths[-1]))
    return paths, all_lines


def test_set_of_pairs(set_files):
    """Three files x three slots of two regions each: nine (slot, region) pairs."""
    capi.set_device(0)
    paths, all_lines = set_files
    la, ra = _spans()["A"]
    mid = (la + ra) // 2
    slots = [_genome_regions("A"), _genome_regions("B"), ["6:%d-%d" % (la + 1, mid + 150), "6:%d-%d" % (mid - 150, ra + 1)]]
    pls = _pls()
    who = [(pls[0], la), (pls[1], _spans()["B"][0]), (pls[0], la)]
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths) as aset:
            assert aset.resident and aset.n_records == sum(map(len, all_lines)) and len(all_lines[0]) == aset.route_tile
            aset.route(slots)
            assert aset.kept == [[len(region_ref.kept(lines, r)) for lines in all_lines] for r in slots]
            assert sum(aset.kept[2]) > sum(aset.kept[0])                        # (the overlap's records: once per region)
            for slot, (pl, left) in enumerate(who):
                got = engine.ManyBatch.from_set(pl, aset, slot, base_locus=left)
                assert engine.front_last() == (2, 0) and engine.front_last_bytes() == 0, (slot, engine.front_last(), engine.front_last_bytes())
                same_many(got, engine.ManyBatch.from_files(pl, paths, regions=["\n".join(slots[slot])] * 3, base_locus=left))
                with engine.test_switches(front="host"):
                    host = engine.ManyBatch.from_files(pl, paths, regions=["\n".join(slots[slot])] * 3, base_locus=left)
                same_many(got, host)


def test_set_with_more_pairs_than_the_mask_holds(set_files):
    """33 slots x 2 regions = 66 pairs: the 32 slots that fit stay resident, the last takes the per-path fallback; all batches equal."""
    capi.set_device(0)
    paths, all_lines = set_files
    pl, (la, ra) = _pls()[0], _spans()["A"]
    slots = [["6:%d-%d" % (la + 1 + 40 * k, la + 900 + 40 * k), "6:%d-%d" % (la + 700 + 40 * k, la + 1500 + 40 * k)] for k in range(33)]
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths) as aset:
            aset.route(slots)
            assert aset.kept[:32] == [[len(region_ref.kept(lines, r)) for lines in all_lines] for r in slots[:32]]
            for slot in (0, 31, 32):
                got = engine.ManyBatch.from_set(pl, aset, slot, base_locus=la)
                assert engine.front_last() == (2, 0), (slot, engine.front_last())
                assert (engine.front_last_bytes() == 0) == (slot < 32), (slot, engine.front_last_bytes())
                same_many(got, engine.ManyBatch.from_files(pl, paths, regions=["\n".join(slots[slot])] * 3, base_locus=la))


def test_end_to_end_genotype_genome_mode(tmp_path):
    """hgx.genotyping_locus on a genotype-genome index and the two-locus BAM: the report of the host front end, both loci out of the file
    opened once, on the device."""
    capi.set_device(0)
    a, b = _loci()
    ix_dir = str(tmp_path / "ix")
    spans = synth.write_genome_index([a, b], ix_dir, "genotype_genome", "hla", chrom="6", gap=GAP, seed=4)
    lines = []
    for k, loc in enumerate((a, b)):
        al = synth.simulate_pairs(loc, synth.pick_sample(loc, 60 + k), 500, err_rate=0.002, seed=90 + k)
        for l in synth.sam_text(loc, al, base_locus=spans[loc.gene][0]).split("\n"):
            if l:
                f = l.split("\t")
                f[0], f[2] = "%s_%s" % (loc.gene, f[0]), "6"
                lines.append("\t".join(f))
    lines = _by_coordinate(lines)
    reports = {}
    opened = []
    real_open = engine.Alignment.__init__

    def counting_open(self, path, *args, **kw):
        opened.append(path)
        real_open(self, path, *args, **kw)
    for front in ("host", "device"):
        out = tmp_path / front
        out.mkdir()
        bam = out / "wgs.bam"
        bamio.write_bam(str(bam), "\n".join(lines) + "\n", [("6", spans["B"][1] + GAP + 1)])
        del opened[:]
        engine.Alignment.__init__ = counting_open
        try:
            with engine.test_switches(front=front):
                hgx.genotyping_locus("hla", ["A", "B"], "genotype_genome", ix_dir, [], True, [["hisat2", "graph"]], ["wgs.fq"], True,
                                     str(bam), 1, 10, 150, 400, False, 2, 0.0, 0.0, [], False, "assembly_graph", True, True, False,
                                     False, True, [], 0, False, str(out), True, {})
        finally:
            engine.Alignment.__init__ = real_open
        reports[front] = (out / "assembly_graph-genotype_genome.wgs.report").read_text()
        if front == "device":
            assert [p["gene"] for p in htyping.last_profile] == ["A", "B"]
            assert all(p["front_end_route"] == [2, 0] for p in htyping.last_profile), htyping.last_profile
            assert opened == [str(bam)]                                         # the file is opened once for both loci
    assert "(count:" in reports["host"] and reports["device"] == reports["host"]


def _rewrite_bgzf(src, dst, edit):
    """The BAM at `src` with its inflated stream passed through `edit(bytearray)`."""
    with open(src, "rb") as f:
        raw = bytearray(b"".join(bamio._bgzf_blocks(f.read())))
    edit(raw)
    with open(dst, "wb") as fo:
        for i in range(0, len(raw), 0xff00):
            part = bytes(raw[i:i + 0xff00])
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            cdata = comp.compress(part) + comp.flush()
            fo.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata +
                     struct.pack("<II", zlib.crc32(part) & 0xffffffff, len(part)))
        fo.write(bamio._BGZF_EOF)


def test_declines(tmp_path):
    """A malformed QNAME (no terminator) in a record that only the SECOND region keeps declines the call -- the per-path reader takes it;
    the same record kept by no region does not."""
    capi.set_device(0)
    loc, pl = _loci()[0], _pls()[0]
    left, right = _spans()["A"]
    lines = _by_coordinate(_lines()["A"])[:600]
    bad_pos = right + 150                                                       # in the spacer behind the locus
    lines.append("ZZBADNAME\t0\t6\t%d\t60\t20M\t*\t0\t0\t%s\t*" % (bad_pos, "ACGT" * 5))
    good, bad = str(tmp_path / "good.bam"), str(tmp_path / "bad.bam")
    bamio.write_bam(good, "\n".join(lines) + "\n", [_chrom()])

    def edit(raw):
        at = raw.find(b"ZZBADNAME\0")
        assert at > 0 and raw.find(b"ZZBADNAME\0", at + 1) < 0
        raw[at + 9] = ord("X")
    _rewrite_bgzf(good, bad, edit)
    first = "6:%d-%d" % (left + 1, right + 1)
    with engine.test_switches(front="device"):
        for second, takes in (("6:%d-%d" % (bad_pos - 10, bad_pos + 10), False), ("6:%d-%d" % (bad_pos + 100, bad_pos + 200), True)):
            with engine.Alignment(bad) as al:
                assert al.resident
                try:
                    al.parse_dev(pl, [first, second], base_locus=left)
                    took = engine.front_last() == (2, 0) and engine.front_last_bytes() == 0
                except capi.HgxError:
                    took = False                                                # (the host reader words the error)
                assert took == takes, (second, engine.front_last(), engine.front_last_bytes())
