"""The kernels of the "hgx" aligner on a linear index (csrc/hgx_align_linear.hip) against the plain statement
(tests/align_linear_ref.py), byte for byte, over the case table (tests/align_linear_cases.py).  Every case asserts that the kernels
gave the bytes (route 2) unless the table names the decline code, so that a fallback cannot pass for a kernel."""
import contextlib
import importlib
import io
import os

import pytest

import align_linear_cases as lc
import align_linear_ref as ref
import linear_ref
from hisatgenotype_amd import align, capi, engine, simulate, synth

pytestmark = pytest.mark.gpu


def _device(c, reads=None):
    capi.set_device(0)
    ix = align.LinearAlignIndex(c["Genes"], c["refGenes"])
    try:
        sw = {"align_linear_budget": c["budget"]} if c["budget"] else {}
        with engine.test_switches(**sw):
            got = ix.align(lc.texts(c) if reads is None else reads, max_edits=c["max_edits"], k=c["k"], route="device")
        return got, align.align_linear_last()
    finally:
        ix.close()


@pytest.mark.parametrize("name", lc.NAMES)
def test_kernels_write_the_statements_bytes(name):
    c = lc.BY_NAME[name]
    got, last = _device(c)
    assert (last["route"], last["decline"]) == ((0, c["decline"]) if c["decline"] else (2, 0)), last
    assert got == lc.ref_text(name)
    alleles = ref.index_of(c["Genes"], c["refGenes"])
    n, aligned, records = ref.counters(alleles, c["reads"], c["max_edits"], c["k"])
    assert (last["reads"], last["aligned"], last["records"]) == (n, aligned, records)
    if not name.startswith("reads-"):
        assert last["candidates"] == sum(ref.candidates(alleles, s, c["max_edits"]) for recs in c["reads"] for _, s, _ in recs)


@pytest.mark.parametrize("name", ["pairs", "single-end-fastq", "cut-candidates+0", "mixed-lengths", "mixed-lengths-own-chunks", "mixed-lengths-span-2",
                                  "mixed-pairs", "mixed-pairs-own-chunks", "tandem", "mixed-257-last"])
def test_a_read_table_made_on_the_device(name):
    """engine.Reads.from_text (the table made by the kernels where the text lies) in place of the loader.  Reads of
    mixed lengths: the table's len[] is indexed by the read's place in the CALL, not in its chunk.  mixed-257-last: the table is made
    (257 bases are within the table's limit) and the aligner declines on the table's max_len; text and table are copied down."""
    c = lc.BY_NAME[name]
    capi.set_device(0)
    with engine.test_switches(front="device"):
        reads = engine.Reads.from_text(lc.texts(c))
    try:
        assert reads.route == 2
        got, last = _device(c, reads)
    finally:
        reads.close()
    assert (last["route"], last["decline"]) == ((0, c["decline"]) if c["decline"] else (2, 0)), last
    assert got == lc.ref_text(name)
    n, aligned, records = ref.counters(ref.index_of(c["Genes"], c["refGenes"]), c["reads"], c["max_edits"], c["k"])
    assert (last["reads"], last["aligned"], last["records"]) == (n, aligned, records)


def test_auto_takes_the_kernels_from_the_gate_on():
    """route="auto": the host route while reads x alleles < LINEAR_GATE, the kernels from there on; one read on either side."""
    c = dict(lc.BY_NAME["bucket-64"])
    assert align.LINEAR_GATE == 64 * 256
    capi.set_device(0)
    ix = align.LinearAlignIndex(c["Genes"], c["refGenes"])
    alleles = ref.index_of(c["Genes"], c["refGenes"])
    try:
        for n, route, decline in ((255, 0, align.LINEAR_DECLINE_GATE), (256, 2, 0)):
            recs = [("g%d" % i, c["reads"][0][i % 3][1], None) for i in range(n)]
            got = ix.align([lc.fasta(recs)], max_edits=c["max_edits"], k=c["k"])
            last = align.align_linear_last()
            assert (last["route"], last["decline"]) == (route, decline), last
            assert got == ref.align_text(alleles, [recs], c["max_edits"], c["k"]).encode()
        with engine.test_switches(front="device"):
            ix.align([lc.fasta(recs[:1])], max_edits=c["max_edits"], k=c["k"])
        assert align.align_linear_last()["route"] == 2
        with engine.test_switches(front="host"):
            ix.align([lc.fasta(recs)], max_edits=c["max_edits"], k=c["k"])
        assert (align.align_linear_last()["route"], align.align_linear_last()["decline"]) == (0, align.LINEAR_DECLINE_SWITCH)
    finally:
        ix.close()


def test_typing_end_to_end(tmp_path, monkeypatch):
    """typing() with ["hgx", "linear"] and reads to align, the kernels aligning (front=device): both forms against linear_ref."""
    from test_align_linear_host import typing_call
    capi.set_device(0)
    with engine.test_switches(front="device"):
        out = typing_call(tmp_path, monkeypatch)
    assert out["routes"] == [2, 2]
