"""The "hgx" aligner's search over STATES (csrc/hgx_align_states.hpp) on the host route (route="host", search="states_all" /
"states"): the tables of the pruned statement (tests/align_ref.py, prune=True) give the statement's text byte for byte -- on every
input the other two forms are judged on, on tandem repeats whose WAYS the per-anchor search cannot enumerate, and past the
window the kernels would decline (the host route widens it).  The default search is untouched.  No GPU."""
import time

import pytest

import align_cases
import align_ref
from hisatgenotype_amd import align, capi


def _host(d, texts, max_edits=2, **kw):
    ix = align.AlignIndex(*d)
    try:
        out = ix.align(texts, max_edits=max_edits, route="host", **kw)
        last = align.align_last()
        assert (last["route"], last["decline"]) == (0, align.DECLINE_SWITCH)
        return out, last
    finally:
        ix.close()


def _plain(reads):
    return [[(q, s, None) for q, s in reads]]


def _n_with_anchor(loci, records):
    """Reads of which some 16-mer at a seed offset, of either strand, stands in a backbone."""
    n = 0
    for _, seq, _ in records:
        seq = seq.upper()
        n += any(s[o:o + align_ref.K] in loc.kmers for s in (seq, align_ref.revcomp(seq)) for o in align_ref.seed_offsets(len(s))
                 for loc in loci)
    return n


@pytest.mark.parametrize("key", align_cases.INPUT_IDS)
def test_states_all_equals_the_statement_on_every_input(key):
    d, texts, me = align_cases.inputs()[key]
    got, last = _host(d, texts, me, search="states_all")
    assert got == align_cases.ref_text(key)
    loci = align_ref.loci_from_dicts(*d)
    assert last["states_reads"] == sum(_n_with_anchor(loci, align_ref.read_records(t)) for t in texts)
    assert (last["states_anchors"] > 0) == (last["states_reads"] > 0) == (last["states_cells"] > 0)


def test_states_all_on_the_hand_pool():
    """All hand-made loci in one index (a read's anchors spread over loci and strands), every read's line the statement's."""
    loci, reads = [], []
    for _, ls, rs, _, _ in align_cases.hand_cases():
        loci += ls
        reads += rs
    want = align_ref.align_text(loci, _plain(reads), 2).encode()
    for search in ("states", "states_all"):
        got, last = _host(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search=search)
        assert got == want
        assert last["states_reads"] == _n_with_anchor(loci, _plain(reads)[0])      # on the host route "states" takes every read too
    assert want.count(b"\n") - len(loci) == len(reads) - 2           # beyond two edits: "e3", and "lf" whose case allows four


@pytest.mark.parametrize("n", [3, 5])
def test_tandem_repeat_against_the_unpruned_statement(n):
    loci, reads = align_cases.tandem_case(n, read_len=100)
    want = align_ref.align_text(loci, _plain(reads), prune=False)
    assert want == align_ref.align_text(loci, _plain(reads), prune=True) and want.count("\n") == 2
    assert _host(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")[0] == want.encode()


@pytest.mark.parametrize("n,kw,anchors", [(13, dict(units=30, singles=4), 23), (19, dict(units=40, singles=4), 13), (19, {}, 1388)])
def test_tandem_repeat_against_the_pruned_statement(n, kw, anchors):
    """13 + 13 and 19 + 19 known unit indels (the kernels' per-anchor search stops between 12 + 12 and 13 + 13; the host route's
    takes seconds at 19 + 19), and the plain repeat whose read has 1 388 anchors on 73 diagonals: one pair of tables each."""
    loci, reads = align_cases.tandem_case(n, **kw)
    want = align_ref.align_text(loci, _plain(reads), prune=True).encode()
    assert want.count(b"\n") == 2
    t = time.perf_counter()
    got, last = _host(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")
    t = time.perf_counter() - t
    assert got == want
    assert (last["states_reads"], last["states_anchors"]) == (1, anchors), last
    assert t < 5.0, t                                                # (milliseconds; the ways form needs 5 s at 19 + 19)
    if not kw:
        rec = want.decode().split("\n")[1].split("\t")
        assert rec[5] == "250M" and "NH:i:1" in rec


def test_a_deletion_that_leaves_the_window_is_followed_on_the_host_route():
    """A known 300-base deletion (longer than HGX_ALN_STATES_MARGIN = 128) that the read takes: the first window poisons the
    anchors' cells, the host route widens it and answers exactly."""
    bb = align_cases._bb(61, 1200)
    loc = align_ref.Locus("W1*BACKBONE", bb, [("deletion", 400, "300", "hv0")])
    reads = [("del", bb[350:400] + bb[700:750]), ("plain", bb[340:440])]
    want = align_ref.align_text([loc], _plain(reads)).encode()
    assert b"50M300D50M" in want and want.count(b"\n") == 3
    assert _host(align_cases.dicts_of([loc]), [align_cases.fasta(reads)], search="states")[0] == want


@pytest.mark.parametrize("key", ["hand3", "pairs-fastq", "lengths"])
def test_the_default_search_is_untouched(key):
    d, texts, me = align_cases.inputs()[key]
    a, last = _host(d, texts, me)
    assert (last["states_reads"], last["states_anchors"], last["states_cells"]) == (0, 0, 0)
    b, last = _host(d, texts, me, search="ways")
    assert (last["states_reads"], last["states_anchors"], last["states_cells"]) == (0, 0, 0)
    assert a == b == align_cases.ref_text(key)
    with pytest.raises(capi.HgxError):
        _host(d, texts, me, search=3)
    with pytest.raises(KeyError):
        _host(d, texts, me, search="state")


def test_align_reads_takes_the_states_name(tmp_path):
    """simulate.align_reads(aligner="hgx.states"): the same BAM as "hgx"; "linear" stays outside."""
    from hisatgenotype_amd import bamio, engine, simulate
    d, texts, me = align_cases.inputs()["single_test_id_and_list-1"]
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    outs = {}
    for name in ("hgx", "hgx.states"):
        out = str(tmp_path / (name + ".bam"))
        with engine.test_switches(front="host"):
            simulate.align_reads(name, True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                                 var_list=Var_list, max_edits=me)
        outs[name] = bamio.read_bam(out)
        assert (align.align_last()["states_reads"] > 0) == (name == "hgx.states")
    assert outs["hgx"] == outs["hgx.states"] and len(outs["hgx"]) == 344
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.states", True, "ix", "linear", "hla", paths, False, 1, str(tmp_path / "x.bam"), 0,
                             truth=(Genes, Vars, refGenes), var_list=Var_list)
