"""A region read through the BAM's index (.bai) gives exactly what the full read gives -- hgx_read_alignments the same bytes,
hgx_parse_alignment_file the same batch -- while it reads a fraction of the file; an index that is truncated, malformed, stale or
built for another file is dropped (the full read answers); hgx_bam_index_build writes tests/bai_ref.py's bytes.  Host only."""
import os
import random
import shutil
import sys

import numpy as np
import pytest

import hisatgenotype_amd as hgx                                   # noqa: F401
from hisatgenotype_amd import bamio, capi, engine

import bai_cases
import bai_ref

htyping = sys.modules["hisatgenotype_amd.typing"]


def text(path, regions):
    return htyping.read_alignment_text(path, regions)


def put_index(path, data):
    with open(path + ".bai", "wb") as f:
        f.write(data)


def same_batch(a, b, length):
    assert (a.n_reads, a.n_pairs, a.n_pieces, a.n_refs, a.n_mask_u32) == (b.n_reads, b.n_pairs, b.n_pieces, b.n_refs, b.n_mask_u32)
    for k in ("pieces", "masks", "pair_off", "pair_ref"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    na, ca = a.pileup(length)
    nb, cb = b.pileup(length)
    assert np.array_equal(na, nb) and np.array_equal(ca, cb)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """block size -> (path, the reference index's bytes); the index lies beside the file."""
    d = tmp_path_factory.mktemp("bam_index")
    out = {}
    for bs in bai_cases.BLOCK_SIZES:
        path = bai_cases.write_fixture(d, bs)
        data = bai_ref.build(path)
        put_index(path, data)
        out[bs] = (path, data)
    return out


@pytest.fixture(scope="module")
def full(files):
    """(block size, case) -> the full read's text, made once with the index switched off."""
    out = {}
    with engine.test_switches(bai="off"):
        for bs, (path, _) in files.items():
            for name, regions in bai_cases.region_grid().items():
                out[bs, name] = text(path, regions)
                assert engine.bam_index_last() == {"used": False, "n_used": 0, "why_not": "off", "file_bytes_read": 0, "n_segments": 0, "n_blocks": 0}
    return out


@pytest.mark.parametrize("bs", bai_cases.BLOCK_SIZES)
def test_region_grid_reads_the_same_bytes(files, full, bs):
    path, _ = files[bs]
    size = os.path.getsize(path)
    kept_some = 0
    for name, regions in bai_cases.region_grid().items():
        with engine.test_switches(bai="force"):
            got = text(path, regions)
            rep = engine.bam_index_last()
        print(bs, name, len(got), rep)
        assert got == full[bs, name], name
        assert rep["used"] and rep["why_not"] == "used", (name, rep)
        if not name.startswith("whole") and not (bs == 0xff00 and name == "nine"):     # (nine regions over most of a file of eight blocks)
            assert 0 < rep["file_bytes_read"] < size, (name, rep)
        kept_some += bool(got)
    assert kept_some >= 14
    assert full[bs, "nothing there"] == full[bs, "beyond the end"] == full[bs, "no records"] == full[bs, "unknown"] == b""
    assert b"spliced\t" in full[bs, "spliced, from a later window"] and b"unmapped_placed\t" in full[bs, "unmapped but placed"]
    two = full[bs, "two, overlapping"].split(b"\n")
    assert len(two) > len(set(two))                                # a record in both regions comes out once per region


def test_the_gate_and_the_reasons(files, tmp_path):
    path, data = files[700]
    regions = bai_cases.locus_regions()
    text(path, regions)                                            # a small file: read whole
    assert engine.bam_index_last()["why_not"] == "small"
    with engine.test_switches(bai="force"):
        text(path, None)
        assert engine.bam_index_last()["why_not"] == "no regions"
        lone = str(tmp_path / "lone.bam")
        shutil.copy(path, lone)
        text(lone, regions)
        assert engine.bam_index_last()["why_not"] == "none"
        put_index(lone[:-4], data)                                 # <path minus .bam>.bai is found too
        text(lone, regions)
        assert engine.bam_index_last()["used"]
        sam = str(tmp_path / "plain.sam")
        with open(sam, "w") as f:
            f.write("\n".join(bai_cases.sam_lines()) + "\n")
        put_index(sam, data)
        text(sam, regions)
        assert engine.bam_index_last()["why_not"] == "not bgzf"


@pytest.mark.parametrize("bs", bai_cases.BLOCK_SIZES)
def test_parse_gives_the_same_batch(files, bs):
    path, _ = files[bs]
    pl, L = bai_cases.packed(), len(bai_cases.the_locus().backbone)
    left = bai_cases.locus_span()[0]
    grid = bai_cases.region_grid()
    for name in ("locus", "two, one block", "two, overlapping", "nine"):
        regions = grid[name] if name != "nine" else grid[name][:8] + ["A*BACKBONE"]
        with engine.test_switches(bai="off"):
            want = pl.parse_alignment_file(path, regions, base_locus=left)
        with engine.test_switches(bai="force"):
            got = pl.parse_alignment_file(path, regions, base_locus=left)
            rep = engine.bam_index_last()
        assert rep["used"] and rep["file_bytes_read"] < os.path.getsize(path), rep
        assert want.n_reads > 0 or name != "locus"
        same_batch(got, want, L)


def test_index_variants_answer_alike(files, full):
    path, data = files[700]
    try:
        for variant in (bai_ref.with_pseudo_bin(data), bai_ref.without_no_coor(data), bai_ref.with_zero_linear(data)):
            put_index(path, variant)
            for name, regions in bai_cases.region_grid().items():
                with engine.test_switches(bai="force"):
                    assert text(path, regions) == full[700, name], name
                    assert engine.bam_index_last()["used"], name
    finally:
        put_index(path, data)


def test_unusable_indexes_mean_no_index(files, full):
    path, data = files[700]
    regions, want = bai_cases.locus_regions(), full[700, "locus"]
    try:
        for cut in range(0, len(data), 7):                         # every prefix, in steps of 7 bytes
            put_index(path, data[:cut])
            with engine.test_switches(bai="force"):
                assert text(path, regions) == want, cut
                rep = engine.bam_index_last()
            if cut == len(data) - 8:                               # (only n_no_coor is missing: fine)
                assert rep["used"], (cut, rep)
            else:
                assert not rep["used"] and rep["why_not"] == "unusable", (cut, rep)
        ix = bai_ref.parse(data)
        ix["refs"].append({"bins": {}, "ioffset": []})             # another reference count than the header's
        bad_magic = b"BAJ\x01" + data[4:]
        negative = data[:8] + b"\xff\xff\xff\xff" + data[12:]
        for variant in (bai_ref.dump(ix), bad_magic, negative):
            put_index(path, variant)
            with engine.test_switches(bai="force"):
                assert text(path, regions) == want
                assert engine.bam_index_last()["why_not"] == "unusable"
        # the first chunk the query takes begins one byte late: the chain guard finds it
        ix = bai_ref.parse(data)
        left, right = bai_cases.locus_span()
        first = min(bai_ref.query(ix, 0, left, right + 1))
        for chunks in ix["refs"][0]["bins"].values():
            for k, c in enumerate(chunks):
                if c == first:
                    chunks[k] = (c[0] + 1, c[1])
        put_index(path, bai_ref.dump(ix))
        with engine.test_switches(bai="force"):
            assert text(path, regions) == want
            assert engine.bam_index_last()["why_not"] == "chain"
        # an index of the same records in blocks of another size
        put_index(path, files[300][1])
        with engine.test_switches(bai="force"):
            assert text(path, regions) == want
            assert engine.bam_index_last()["why_not"] in ("chain", "inflate")
    finally:
        put_index(path, data)


@pytest.mark.parametrize("bs", bai_cases.BLOCK_SIZES)
def test_writer_writes_the_reference_bytes(files, tmp_path, bs):
    path, data = files[bs]
    out = str(tmp_path / "own.bai")
    assert bamio.index_bam(path, out) == out
    assert open(out, "rb").read() == data
    for piece in (1, 257, 4099):                                   # pieces that cut blocks and records everywhere
        with engine.test_switches(bai_piece=piece):
            bamio.index_bam(path, out)
        assert open(out, "rb").read() == data, piece
    assert sorted(os.listdir(str(tmp_path))) == ["own.bai"]        # no temporary file stays


def test_writer_default_name_and_refusals(tmp_path):
    lines = list(bai_cases.sam_lines())
    path = bai_cases.write_fixture(tmp_path, 700, lines, "ok.bam")
    assert bamio.index_bam(path) == path + ".bai" and open(path + ".bai", "rb").read() == bai_ref.build(path)
    random.Random(5).shuffle(lines)
    grouped = bai_cases.write_fixture(tmp_path, 700, sorted(lines, key=lambda l: l.split("\t")[0]), "grouped.bam")
    with pytest.raises(capi.HgxError) as e:
        bamio.index_bam(grouped)
    assert e.value.code in (-1, -3) and "offset" in str(e.value), str(e.value)
    placed_last = [l for l in bai_cases.sam_lines() if l.split("\t")[2] == "*"] + [l for l in bai_cases.sam_lines() if l.split("\t")[2] != "*"]
    late = bai_cases.write_fixture(tmp_path, 700, placed_last, "late.bam")
    with pytest.raises(capi.HgxError) as e:
        bamio.index_bam(late)
    assert "unplaced" in str(e.value)
    damaged = str(tmp_path / "damaged.bam")
    raw = bytearray(open(path, "rb").read())
    raw[len(raw) // 2] ^= 0x55
    open(damaged, "wb").write(bytes(raw))
    with pytest.raises(capi.HgxError):
        bamio.index_bam(damaged)
    assert sorted(f for f in os.listdir(str(tmp_path)) if not f.endswith(".bam")) == ["ok.bam.bai"]
