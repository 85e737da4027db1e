"""The read table made by kernels where the text lies (csrc/hgx_reads.hip: k_rd_nl, k_rd_records; engine.Reads with front=device)
against the plain statement (tests/reads_table_ref.py) on every named case of tests/reads_table_cases.py -- the same records, the
decline code the statement names -- the gate, and the aligner over such an object against the aligner over the texts: every form
of the call, across a chunk edge, single-end and paired, behind a decline of the aligner's own, and the resident hand-off."""
import pytest

import align_cases
import reads_table_cases as rc
import reads_table_ref as ref
from hisatgenotype_amd import align, capi, engine

pytestmark = pytest.mark.gpu

CHUNK = 8192                         # reads per chunk of the aligner's device route (csrc/hgx_align.hip)
FORMS = {"default": {}, "states_all": dict(search="states_all"), "pair_aware": dict(pair="aware"), "clip": dict(clip=32),
         "gap": dict(gap=16), "rescue": dict(rescue=(16, 32))}      # (tests/test_gpu_align_resident.py FORMS)


@pytest.mark.parametrize("name", list(rc.cases()))
def test_kernels_equal_the_statement(name):
    case = rc.cases()[name]
    takes = ref.device_takes(case.texts, case.fastq, case.front)
    assert takes == case.takes
    with engine.test_switches(front=case.front):
        if case.error is not None:
            with pytest.raises(capi.HgxError) as e:
                engine.Reads.from_text(case.texts, fastq=case.fastq)
            assert ref.MESSAGES[case.error] in str(e.value)
            return
        want = ref.records(case.texts, case.fastq)
        r = engine.Reads.from_text(case.texts, fastq=case.fastq)
    try:
        assert (r.route, r.decline) == ((2, 0) if takes == 0 else (0, takes))
        longest = max([len(s) for _, s, _ in want] + [0])
        assert (r.n_reads, r.max_len) == (len(want), longest)
        assert engine.reads_last() == (r.route, r.decline, len(want), longest)
        assert r.records() == want
        assert [r.input_text(i) for i in range(r.n_inputs)] == [bytes(t) for t in case.texts]
        if r.route == 2:                         # the offsets point into the text as it lies: input 1, then input 2 at a multiple of 64
            text, no, so, qo, nl, ln = r.table()
            at = 0
            for i, t in enumerate(case.texts):
                assert text[at:at + len(t)] == bytes(t)
                at = (at + len(t) + 63) // 64 * 64
    finally:
        r.close()


def test_the_gate():
    for size, route, decline in ((align.READS_GATE + (6 << 10), 2, 0), (align.READS_GATE - (4 << 10), 0, align.READS_DECLINE_GATE)):
        t = align_cases.fastq([("g%04d" % k, "ACGT" * 25, "F" * 100) for k in range(size // 211)])      # (211 bytes per record)
        assert abs(len(t) - size) < 211 and (len(t) >= align.READS_GATE) == (route == 2)
        r = engine.Reads.from_text([t])
        assert (r.route, r.decline) == (route, decline) and r.records() == ref.records([t])
        r.close()


_POOL = []


def _pool():
    """The hand-made loci of align_cases in one index and their reads."""
    if not _POOL:
        loci, reads = [], []
        for _, ls, rs, _, _ in align_cases.hand_cases():
            loci += ls
            reads += rs
        _POOL.append((loci, reads))
    return _POOL[0]


def _both(d, texts, **kw):
    """(text, align_last()) of the aligner over the texts and over an engine.Reads of them, front=device; the table's (route, decline)."""
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="device"):
            want = ix.align(texts, **kw)
            last0 = align.align_last()
            r = engine.Reads.from_text(texts)
            made = (r.route, r.decline)
            got = ix.align(r, **kw)
            last = align.align_last()
            r.close()
        return want, last0, got, last, made
    finally:
        ix.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_the_aligner_over_the_table_single_end(form):
    loci, reads = _pool()
    n = CHUNK + 1
    pick = [(k * 7 + k // len(reads)) % len(reads) for k in range(n)]
    text = align_cases.fasta([("q%d" % k, reads[j][1]) for k, j in enumerate(pick)])
    want, last0, got, last, made = _both(align_cases.dicts_of(loci), [text], **FORMS[form])
    assert made == (2, 0) and got == want and last == last0
    assert (last["route"], last["reads"]) == (2, n) and last["aligned"] > n // 2


@pytest.mark.parametrize("form", list(FORMS))
def test_the_aligner_over_the_table_paired(form):
    m1, m2, _ = align_cases.pair_reads()
    n_pairs = CHUNK // 2 + 1
    pick = [(k * 3 + k // len(m1)) % len(m1) for k in range(n_pairs)]
    f1 = align_cases.fastq([("p%d" % k, m1[j][1], "F" * 100) for k, j in enumerate(pick)])
    f2 = align_cases.fastq([("p%d" % k, m2[j][1], "5" * 100) for k, j in enumerate(pick)])
    want, last0, got, last, made = _both(align_cases.dicts_of(align_cases.pair_loci()), [f1, f2], **FORMS[form])
    assert made == (2, 0) and got == want and last == last0
    assert (last["route"], last["reads"]) == (2, 2 * n_pairs) and last["pairs_concordant"] == sum(j < 2 for j in pick)


def test_an_anchor_decline_behind_a_full_first_chunk():
    loci, reads = _pool()
    rep_loci, rep_reads = align_cases.limit_case("anchors", align_cases.DEV_ANCHORS + 1)
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, rep_reads[0])
    want, last0, got, last, made = _both(align_cases.dicts_of(loci + rep_loci), [align_cases.fasta(recs)])
    assert made == (2, 0)
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS) and last == last0
    assert got == want


def test_a_300_base_read():
    loc = align_cases.length_locus()
    reads = align_cases.length_reads([100, 300, 64])
    want, last0, got, last, made = _both(align_cases.dicts_of([loc]), [align_cases.fasta(reads)])
    assert made == (2, 0)
    assert (last["route"], last["decline"]) == (0, align.DECLINE_READ_LEN) and last == last0
    assert got == want and got.count(b"\n") == 1 + 3


def test_the_resident_hand_off():
    loci, reads = _pool()
    pick = [(k * 7 + k // len(reads)) % len(reads) for k in range(1200)]
    text = align_cases.fasta([("q%d" % k, reads[j][1]) for k, j in enumerate(pick)])
    ix = align.AlignIndex(*align_cases.dicts_of(loci))
    try:
        with engine.test_switches(front="device"):
            al = ix.align_resident([text])
            want, last0 = al.text(), align.align_last()
            al.close()
            r = engine.Reads.from_text([text])
            al = ix.align_resident(r)
            assert r.route == 2 and al.resident and al.text() == want and align.align_last() == last0 and last0["route"] == 2
            al.close()
            r.close()
    finally:
        ix.close()
