"""The BAM index on the device route.  k_bam_splice (hgx_bam_splice) against numpy.concatenate at its alignment, length and table-size
edges; then the fixtures of test_bam_index.py with front=device, bai=force against bai=off: the path call (the blocks the index names
go up, are inflated and spliced on the device), the typing call, many files in one pass, the file opened once, and a stale index that
the device walk declines and the host reader's guard then drops."""
import os
import shutil
import sys

import numpy as np
import pytest

import hisatgenotype_amd as hgx
from hisatgenotype_amd import capi, engine

import bai_cases
import bai_ref
from test_bam_index import put_index, same_batch

htyping = sys.modules["hisatgenotype_amd.typing"]
pytestmark = pytest.mark.gpu
LDS_SEGS = 2048                     # csrc/hgx_inflate.hip SPL_LDS_SEGS: up to this many segments the prefix table lives in LDS
WG_BYTES = 64 << 10                 # ... and a workgroup's share of the destination


def _splice(rng, src, segments, dst_off, tail=37):
    total = sum(n for _, n in segments)
    dst = rng.integers(0, 256, dst_off + total + tail, dtype=np.uint8)
    want = dst.copy()
    if total:
        want[dst_off:dst_off + total] = np.concatenate([src[o:o + n] for o, n in segments])
    got = engine.bam_splice(src, segments, dst.copy(), dst_off)
    assert np.array_equal(got, want), (segments[:4], dst_off)      # (the bytes before and after the range included)


def test_splice_alignments_and_lengths():
    capi.set_device(0)
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, 9000, dtype=np.uint8)
    for n in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097):
        for sm in range(4):
            for dst_off in (0, 1, 2, 3, 13, 14, 15, 16, 17):       # every destination offset mod 4, and on both sides of a 16-byte unit
                _splice(rng, src, [(100 + sm, n)], dst_off)
    _splice(rng, src, [(len(src) - 4097, 4097)], 5)                  # up to the source's last byte


def test_splice_segment_edges():
    capi.set_device(0)
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, 400000, dtype=np.uint8)
    _splice(rng, src, [(7, 3), (1001, 5)], 0)                        # two segments in one destination dword / 16-byte unit
    _splice(rng, src, [(7, 3), (1001, 5), (50, 2), (9, 40)], 2)
    _splice(rng, src, [(10, 100), (500, 0), (2000, 100)], 3)         # an empty segment between two others
    _splice(rng, src, [(0, 0), (10, 17), (0, 0), (0, 0), (33, 1), (90, 0)], 16)
    _splice(rng, src, [], 4)
    _splice(rng, src, [(3, 0)], 4)
    _splice(rng, src, [(5, 3 * WG_BYTES + 11), (1, 30), (200001, WG_BYTES)], 9)     # a segment larger than a workgroup's share
    _splice(rng, src, [(2, WG_BYTES - 16), (70001, 16), (9, 16)], 0)               # segments that end on a workgroup's edge


@pytest.mark.parametrize("n_seg", [1, 2, 65, 1025, LDS_SEGS - 1, LDS_SEGS, LDS_SEGS + 1, 5000])
def test_splice_table_sizes(n_seg):
    """The prefix table in LDS and in global memory: the count on both sides of the switch."""
    capi.set_device(0)
    rng = np.random.default_rng(n_seg)
    src = rng.integers(0, 256, 50000, dtype=np.uint8)
    lens = rng.integers(0, 41, n_seg)
    offs = rng.integers(0, len(src) - 41, n_seg)
    _splice(rng, src, list(zip(offs.tolist(), lens.tolist())), int(rng.integers(0, 32)))


def test_splice_refuses_what_does_not_fit():
    capi.set_device(0)
    src = np.zeros(100, np.uint8)
    for segments, size in (([(90, 11)], 64), ([(0, 50), (101, 0)], 64), ([(0, 60)], 59)):
        with pytest.raises(capi.HgxError):
            engine.bam_splice(src, segments, np.zeros(size, np.uint8), 0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_bam_index")
    out = {}
    for bs in bai_cases.BLOCK_SIZES:
        path = bai_cases.write_fixture(d, bs)
        data = bai_ref.build(path)
        put_index(path, data)
        out[bs] = (path, data)
    return out


@pytest.mark.parametrize("bs", bai_cases.BLOCK_SIZES)
def test_path_call_through_the_index(files, bs):
    capi.set_device(0)
    path, _ = files[bs]
    pl, L = bai_cases.packed(), len(bai_cases.the_locus().backbone)
    left, right = bai_cases.locus_span()
    three = ["6:%d-%d" % (left + 1, left + 1200), "A*BACKBONE", "6:%d-%d" % (left + 900, right + 1)]
    far = ["6:%d-%d" % (left + 1, right + 1), "7:40001-48000"]       # the second region lies far behind the first in the file: two segments
    for regions in (["6:%d-%d" % (left + 1, right + 1)], three, bai_cases.locus_regions(), far):
        with engine.test_switches(front="device", bai="off"):
            want = pl.parse_alignment_file_dev(path, regions, base_locus=left)
            assert engine.front_last() == (2, 0)
            sent_full = engine.front_last_bytes()
        with engine.test_switches(front="device", bai="force"):
            got = pl.parse_alignment_file_dev(path, regions, base_locus=left)
            route, sent, rep = engine.front_last(), engine.front_last_bytes(), engine.bam_index_last()
        print(bs, regions, "sent", sent, "of", sent_full, rep)
        assert want.to_host().n_reads > 0
        same_batch(got.to_host(), want.to_host(), L)
        assert route == (2, 0), route
        assert rep["used"] and rep["file_bytes_read"] < os.path.getsize(path), rep
        assert 0 < sent < sent_full, (sent, sent_full)
        assert rep["n_segments"] >= (2 if regions is far else 1), rep


def test_typing_call_through_the_index(files):
    capi.set_device(0)
    path, _ = files[700]
    pl, left = bai_cases.packed(), bai_cases.locus_span()[0]
    regions = bai_cases.locus_regions()
    with engine.test_switches(front="device", bai="off"):
        want = hgx.type_file(pl, path, regions, base_locus=left)
    with engine.test_switches(front="device", bai="force"):
        got = hgx.type_file(pl, path, regions, base_locus=left)
        assert engine.front_last() == (2, 0) and engine.bam_index_last()["used"]
    assert got.num_reads == want.num_reads > 0 and got.num_pairs == want.num_pairs
    assert got.gene_prob == want.gene_prob and got.em == want.em and got.counts_sorted == want.counts_sorted       # the EM's doubles, bit for bit
    assert hgx.report_lines(got, False, (), True)[0] == hgx.report_lines(want, False, (), True)[0]


def test_many_files_in_one_pass(files, tmp_path):
    """Three files: one with its index, one that lists the references in another order (its own index), one without an index; regions per task."""
    capi.set_device(0)
    pl, (left, right) = bai_cases.packed(), bai_cases.locus_span()
    other = bai_cases.write_fixture(tmp_path, 700, name="other_order.bam", refs=[bai_cases.REFS[1], bai_cases.REFS[0], bai_cases.REFS[2]])
    put_index(other, bai_ref.build(other))
    lone = str(tmp_path / "lone.bam")
    shutil.copy(files[300][0], lone)
    paths = [files[700][0], other, lone]
    regions = ["\n".join(bai_cases.locus_regions()), "6:%d-%d" % (left + 500, right + 1), "6:%d-%d\n6:%d-%d" % (left + 1, left + 1500, left + 1400, right + 1)]
    with engine.test_switches(front="device", bai="off"):
        want = engine.ManyBatch.from_files(pl, paths, regions=regions, base_locus=left)
        assert engine.front_last() == (2, 0)
        sent_full = engine.front_last_bytes()
        assert engine.bam_index_last()["n_used"] == 0
    with engine.test_switches(front="device", bai="force"):
        got = engine.ManyBatch.from_files(pl, paths, regions=regions, base_locus=left)
        assert engine.front_last() == (2, 0)
        sent, rep = engine.front_last_bytes(), engine.bam_index_last()
    print("many: sent", sent, "of", sent_full, rep)
    # the two files with an index went through it (each reader's report, summed); the third was sent whole, deflated, as before
    assert rep["n_used"] == 2 and rep["n_segments"] >= 2 and 0 < rep["file_bytes_read"] < os.path.getsize(paths[0]) + os.path.getsize(paths[1]), rep
    assert os.path.getsize(lone) < sent < sent_full, (sent, sent_full)
    assert got.n_tasks == want.n_tasks == 3 and got.pair_base == want.pair_base and min(want.task_reads) > 0
    assert got.task_reads == want.task_reads and got.task_pieces == want.task_pieces and got.task_refs == want.task_refs
    a, b = got.merged(), want.merged()
    for k in ("pieces", "masks", "pair_off", "pair_ref"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_file_opened_once_is_not_read_at_open(files):
    capi.set_device(0)
    path, _ = files[700]
    pl, L = bai_cases.packed(), len(bai_cases.the_locus().backbone)
    left, right = bai_cases.locus_span()
    with engine.test_switches(front="device", bai="off"):
        with engine.Alignment(path) as al:
            assert al.resident
            want = [al.parse_dev(pl, r, base_locus=left).to_host() for r in (bai_cases.locus_regions(), ["6:%d-%d" % (left + 700, right + 1)])]
    with engine.test_switches(front="device", bai="force"):
        with engine.Alignment(path) as al:
            rep = engine.bam_index_last()
            assert not al.resident and al.bytes_to_device == 0
            assert rep["used"] and rep["n_segments"] == 0 and 0 < rep["file_bytes_read"] <= 16384, rep      # the header's blocks only
            for w, r in zip(want, (bai_cases.locus_regions(), ["6:%d-%d" % (left + 700, right + 1)])):
                got = al.parse_dev(pl, r, base_locus=left)
                assert engine.front_last() == (2, 0) and engine.bam_index_last()["used"]
                same_batch(got.to_host(), w, L)


def test_stale_index_declines_once_and_reads_the_file(files, tmp_path):
    """The first chunk of the locus begins one byte late: the device walk's chain does not link up and declines; the host reader's
    guard finds the same, drops the index and reads the whole file: the same batch, why_not = chain."""
    capi.set_device(0)
    path = str(tmp_path / "stale.bam")
    shutil.copy(files[700][0], path)
    pl, L = bai_cases.packed(), len(bai_cases.the_locus().backbone)
    left, right = bai_cases.locus_span()
    regions = bai_cases.locus_regions()
    ix = bai_ref.parse(files[700][1])
    first = min(bai_ref.query(ix, 0, left, right + 1))
    for chunks in ix["refs"][0]["bins"].values():
        for k, c in enumerate(chunks):
            if c == first:
                chunks[k] = (c[0] + 1, c[1])
    put_index(path, bai_ref.dump(ix))
    with engine.test_switches(front="device", bai="off"):
        want = pl.parse_alignment_file_dev(path, regions, base_locus=left).to_host()
        with engine.Alignment(path) as al:
            inflated = al.stream_bytes
    with engine.test_switches(front="device", bai="force"):
        got = pl.parse_alignment_file_dev(path, regions, base_locus=left)
        rep, sent = engine.bam_index_last(), engine.front_last_bytes()
    same_batch(got.to_host(), want, L)
    assert not rep["used"] and rep["why_not"] == "chain", rep
    # one device attempt, declined: the blocks the index named went up, then the second read's whole inflated stream -- had the host
    # guard met the index first, the file alone would have gone up, deflated
    assert inflated < sent < inflated + os.path.getsize(path), (sent, inflated)
