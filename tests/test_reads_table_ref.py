"""The plain statement of the aligner's read table (tests/reads_table_ref.py) against the host loader (csrc/hgx_align_host.cpp
through engine.Reads with front=host), on every named case of tests/reads_table_cases.py; device_takes against the expectation
written down per case; and the aligner over an engine.Reads on the host route against the aligner over the texts.  No GPU."""
import gzip

import pytest

import align_cases
import reads_table_cases as rc
import reads_table_ref as ref
from hisatgenotype_amd import align, capi, engine

NAMES = list(rc.cases())


def test_the_constants_are_the_library_s():
    assert (ref.TILE, ref.GATE, ref.MAX_READ, ref.MAX_BYTES) == (align.READS_TILE, align.READS_GATE, align.MAX_READ, align.READS_MAX_BYTES)
    assert (align.READS_DECLINE_GATE, align.READS_DECLINE_SWITCH, align.READS_DECLINE_EMPTY_LINE, align.READS_DECLINE_MARKER,
            align.READS_DECLINE_TRUNCATED, align.READS_DECLINE_QUAL_LEN, align.READS_DECLINE_LOWER, align.READS_DECLINE_COUNT,
            align.READS_DECLINE_READ_LEN, align.READS_DECLINE_SIZE) == (ref.GATE_CODE, ref.SWITCH, ref.EMPTY_LINE, ref.MARKER, ref.TRUNCATED,
                                                                         ref.QUAL_LEN, ref.LOWER, ref.COUNT, ref.READ_LEN, ref.SIZE)
    for name in ("hgx_reads_from_text", "hgx_reads_dims", "hgx_reads_table", "hgx_reads_input_text", "hgx_reads_last", "hgx_reads_free",
                 "hgx_align_reads_dev", "hgx_align_reads_dev_resident"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)


@pytest.mark.parametrize("name", NAMES)
def test_the_host_loader_gives_the_statement(name):
    case = rc.cases()[name]
    with engine.test_switches(front="host"):
        if case.error is not None:
            with pytest.raises(ref.ReadsError) as e:
                ref.records(case.texts, case.fastq)
            assert e.value.kind == case.error
            with pytest.raises(capi.HgxError) as e:
                engine.Reads.from_text(case.texts, fastq=case.fastq)
            assert ref.MESSAGES[case.error] in str(e.value)
            return
        want = ref.records(case.texts, case.fastq)
        r = engine.Reads.from_text(case.texts, fastq=case.fastq)
        try:
            assert (r.route, r.decline, r.n_reads, r.n_inputs) == (0, align.READS_DECLINE_SWITCH, len(want), len(case.texts))
            assert engine.reads_last() == (0, align.READS_DECLINE_SWITCH, len(want), max([len(s) for _, s, _ in want] + [0]))
            assert r.records() == want
            assert [r.input_text(i) for i in range(r.n_inputs)] == [bytes(t) for t in case.texts]
        finally:
            r.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_takes_is_what_the_case_says(name):
    case = rc.cases()[name]
    assert ref.device_takes(case.texts, case.fastq, case.front) == case.takes
    # a text the kernels take is one where the positional view and the loader's agree: the statement then raises nothing
    if case.takes == 0:
        assert case.error is None
    if case.front == "device":
        assert ref.device_takes(case.texts, case.fastq, "host") == ref.SWITCH
        assert ref.device_takes(case.texts, case.fastq, None) == (ref.GATE_CODE if sum(map(len, case.texts)) < ref.GATE else case.takes)


def test_gzip_texts_and_paths_are_inflated_first(tmp_path):
    case = rc.cases()["two-fastq"]
    want = ref.records(case.texts)
    paths = []
    for i, t in enumerate(case.texts):
        paths.append(str(tmp_path / ("m%d.fq.gz" % i)))
        with open(paths[-1], "wb") as f:
            f.write(gzip.compress(t))
    with engine.test_switches(front="host"):
        for src in ([gzip.compress(t) for t in case.texts], paths):
            r = engine.Reads.from_text(src)
            assert r.records() == want and [r.input_text(i) for i in range(2)] == case.texts
            out = [str(tmp_path / ("saved%d.fq.gz" % i)) for i in range(2)]
            r.save(out)
            assert [gzip.open(p).read() for p in out] == case.texts
            r.close()
        with pytest.raises(capi.HgxError):
            engine.Reads.from_text([str(tmp_path / "missing.fq")])


@pytest.mark.parametrize("k", range(7))
def test_the_aligner_over_reads_equals_the_aligner_over_texts(k):
    _, loci, reads, me, _ = align_cases.hand_cases()[k]
    texts = [align_cases.fasta(reads)]
    ix = align.AlignIndex(*align_cases.dicts_of(loci))
    try:
        want = ix.align(texts, max_edits=me, route="host")
        last = align.align_last()
        with engine.test_switches(front="host"):
            r = engine.Reads.from_text(texts)
        for _ in range(2):                       # (the object is not used up)
            assert ix.align(r, max_edits=me, route="host") == want
            assert align.align_last() == last
        assert ix.align(r, max_edits=me, route="host", order="coordinate") == ix.align(texts, max_edits=me, route="host", order="coordinate")
        r.close()
    finally:
        ix.close()


@pytest.mark.parametrize("n_inputs", [1, 2])
def test_the_size_rule_at_its_threshold(n_inputs):
    """HGX_RD_DECLINE_SIZE with the limit lowered by the test switch reads_max_bytes (4 GB of text is no test input): the texts with
    64 bytes of padding one byte below the limit pass the rule (here: on to the gate), at the limit they decline with SIZE -- the
    rule of device_takes; the loader gives the statement's records either way.  The rule is settled before any kernel: no GPU."""
    text = rc.cases()["count-65"].texts[0]
    texts = [text] * n_inputs
    total = len(text) * n_inputs
    want = ref.records(texts)
    for limit, code in ((total + 65, ref.GATE_CODE), (total + 64, ref.SIZE), (total, ref.SIZE)):
        assert ref.device_takes(texts, None, None, max_bytes=limit) == code
        with engine.test_switches(reads_max_bytes=str(limit)):
            r = engine.Reads.from_text(texts)
        assert (r.route, r.decline) == (0, code) and r.records() == want
        r.close()
    assert ref.device_takes([b"x" * 10], None, "device", max_bytes=ref.MAX_BYTES) != ref.SIZE
    assert ref.MAX_BYTES - 64 == (1 << 32) - 128
