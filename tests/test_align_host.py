"""The host route of the "hgx" aligner (csrc/hgx_align_host.cpp through hgx_align_reads, route forced with front=host) gives the
Python statement's text (tests/align_ref.py) byte for byte.  No GPU."""
import gzip

import pytest

import align_cases
import align_ref
from hisatgenotype_amd import align, capi, engine

MAX_READ = 1024                      # HGX_ALN_MAX_READ: the longest read the core takes


def _host(d, texts, max_edits=2, **kw):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="host"):
            out = ix.align(texts, max_edits=max_edits, **kw)
        last = align.align_last()
        assert last["route"] == 0 and last["decline"] == align.DECLINE_SWITCH
        return out, last
    finally:
        ix.close()


@pytest.mark.parametrize("key", align_cases.INPUT_IDS)
def test_host_route_equals_the_statement(key):
    d, texts, me = align_cases.inputs()[key]
    got, last = _host(d, texts, me)
    want = align_cases.ref_text(key)
    assert got == want
    recs = [l for l in want.decode().split("\n") if l and not l.startswith("@")]
    assert last["aligned"] == len(recs)
    assert last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert last["reads"] == sum(len(align_ref.read_records(t)) for t in texts)


def test_files_on_disk(tmp_path):
    """Paths instead of texts: FASTQ .gz mate files and a plain FASTA, the format told or found."""
    d, texts, me = align_cases.inputs()["pairs-fastq"]
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("r-%d.fq.gz" % (m + 1))
        p.write_bytes(gzip.compress(t))
        paths.append(str(p))
    assert _host(d, paths, me)[0] == align_cases.ref_text("pairs-fastq")
    assert _host(d, paths, me, fastq=True)[0] == align_cases.ref_text("pairs-fastq")
    d, texts, me = align_cases.inputs()["hand0"]
    p = tmp_path / "h.fa"
    p.write_bytes(texts[0])
    assert _host(d, [str(p)], me, fastq=False)[0] == align_cases.ref_text("hand0")
    with pytest.raises(capi.HgxError):
        _host(d, [str(tmp_path / "missing.fa")], me)


def test_longest_read_and_one_more():
    loc = align_cases.length_locus()
    d = align_cases.dicts_of([loc])
    reads = align_cases.length_reads([MAX_READ])
    want = align_ref.align_text([loc], [[(n, s, None) for n, s in reads]]).encode()
    assert want.count(b"\n") == 2
    assert _host(d, [align_cases.fasta(reads)])[0] == want
    with pytest.raises(capi.HgxError, match="1025 bases"):
        _host(d, [align_cases.fasta(align_cases.length_reads([MAX_READ + 1]))])


def test_names_keep_what_the_statement_keeps():
    text = align_cases.ref_text("pairs-fasta").decode()
    names = [l.split("\t")[0] for l in text.split("\n") if l and not l.startswith("@")]
    assert names[:4] == ["fr|x/1", "fr|x/2", "rf", "rf"]


def test_lower_case_bases_and_unequal_mate_files():
    d, texts, me = align_cases.inputs()["hand0"]
    assert _host(d, [texts[0].lower().replace(b">A", b">a")], me)[0] == align_cases.ref_text("hand0")
    d, texts, me = align_cases.inputs()["pairs-fasta"]
    with pytest.raises(capi.HgxError):
        _host(d, [texts[0], texts[1][:200]], me)


def test_the_gate_keeps_small_calls_on_the_host_route():
    d, texts, me = align_cases.inputs()["hand0"]
    ix = align.AlignIndex(*d)
    assert ix.align(texts, max_edits=me) == align_cases.ref_text("hand0")
    assert align.align_last()["route"] == 0 and align.align_last()["decline"] == align.DECLINE_GATE
    assert engine.AlignIndex is align.AlignIndex


def test_align_reads_takes_the_new_aligner_name(tmp_path, monkeypatch):
    """simulate.align_reads(aligner="hgx"): a coordinate-sorted BAM of the statement's records; "linear" stays outside."""
    from hisatgenotype_amd import bamio, simulate
    d, texts, me = align_cases.inputs()["single_test_id_and_list-1"]
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    out = str(tmp_path / "out.bam")
    with engine.test_switches(front="host"):
        simulate.align_reads("hgx", True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                             var_list=Var_list, max_edits=me)
    want = str(tmp_path / "want.bam")
    simulate._store_as_the_reference_does(want, align_cases.ref_text("single_test_id_and_list-1").decode())
    assert bamio.read_bam(out) == bamio.read_bam(want) and len(bamio.read_bam(out)) == 344
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx", True, "ix", "linear", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                             var_list=Var_list)


@pytest.mark.parametrize("key", [k for k in align_cases.INPUT_IDS if not k.startswith("empty")])
def test_the_pruned_statement_is_the_exhaustive_one(key):
    """align_ref's prune=True (one entry per state instead of every way through it) gives the exhaustive search's text."""
    d, texts, me = align_cases.inputs()[key]
    loci = align_ref.loci_from_dicts(*d)
    reads = [align_ref.read_records(t) for t in texts]
    assert align_ref.align_text(loci, reads, me, prune=True).encode() == align_cases.ref_text(key)


def test_tandem_repeat_with_many_known_indels():
    """GATA x 40 with 14 known unit deletions and 14 known unit insertions, a 250-base read with one error behind the repeat: the
    number of WAYS through the repeat is exponential in the number of indels, the number of states is not.  The host route
    remembers the best arrival at every state reached through an indel (HostMemo), so this finishes in well under a second per
    read (an enumeration of the ways takes 5 x longer for every two indels more: minutes here); the text is the statement's."""
    loci, reads = align_cases.tandem_case(4)
    plain = [[(q, s, None) for q, s in reads]]
    assert align_ref.align_text(loci, plain, prune=True) == align_ref.align_text(loci, plain)
    for n, mism in ((14, 1), (14, 3), (10, 2)):
        loci, reads = align_cases.tandem_case(n, mismatches=mism)
        want = align_ref.align_text(loci, [[(q, s, None) for q, s in reads]], prune=True).encode()
        assert want.count(b"\n") == (1 if mism > 2 else 2)
        assert _host(align_cases.dicts_of(loci), [align_cases.fasta(reads)])[0] == want
