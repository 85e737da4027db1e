"""Pair-aware placement on the host route of the "hgx" aligner (csrc/hgx_align_host.cpp, hgx_align_opts.pair = 1, route forced with
front=host): the bytes of the plain-Python statement (tests/align_pair_ref.py), the counters of hgx_align_last_pairs, the argument
checks, and the aligner name "hgx.pairs".  No GPU."""
import ctypes as C

import pytest

import align_cases
import align_pair_cases
from hisatgenotype_amd import align, capi, engine

PAIRED = align_pair_cases.PAIRED


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


@pytest.mark.parametrize("key", align_pair_cases.INPUT_IDS)
def test_host_route_equals_the_pair_statement(key):
    d, texts, me, frag = align_pair_cases.inputs()[key]
    got, last = _host(d, texts, me, max_fragment=frag, pair="aware")
    want = align_pair_cases.ref_text(key)
    assert got == want
    recs = [l for l in want.decode().split("\n") if l and not l.startswith("@")]
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert (last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]) == align_pair_cases.ref_counters(key)


@pytest.mark.parametrize("key", align_pair_cases.HAND_IDS)
def test_the_counters_of_the_hand_cases(key):
    d, texts, me, frag = align_pair_cases.inputs()[key]
    _, last = _host(d, texts, me, max_fragment=frag, pair=1)
    assert (last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]) == align_pair_cases.HAND_COUNTERS[key]
    s, p, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert capi.lib().hgx_align_last_pairs(C.byref(s), C.byref(p), C.byref(c)) == 0
    assert (s.value, p.value, c.value) == align_pair_cases.HAND_COUNTERS[key]
    assert capi.lib().hgx_align_last_pairs(None, None, None) == 0
    _, last = _host(d, texts, me, max_fragment=frag)
    assert (last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]) == (0, 0, 0)


@pytest.mark.parametrize("key", PAIRED)
def test_the_independent_suites_paired_inputs(key):
    """pair = 0 gives align_cases.ref_text unchanged; pair = 1 gives the pair statement's text -- the same bytes wherever both
    independent NH are 1 (tests/test_align_pair_ref.py) -- and the independent text on the pair cases."""
    d, texts, me = align_cases.inputs()[key]
    assert len(texts) == 2
    assert _host(d, texts, me, pair="independent")[0] == align_cases.ref_text(key)
    assert _host(d, texts, me, pair=0)[0] == align_cases.ref_text(key)
    got, last = _host(d, texts, me, pair="aware")
    assert got == align_pair_cases.ref_text_paired(key)
    if key.startswith(("pairs-", "empty")):
        assert got == align_cases.ref_text(key) and last["pairs_changed"] == 0
        assert (last["pairs_searched"], last["pairs_placed"]) == ((6, 2) if key.startswith("pairs-") else (0, 0))


def test_single_end_input_with_the_pair_rule():
    for key in ("single-fastq", "hand6", "empty"):
        d, texts, me = align_cases.inputs()[key]
        got, last = _host(d, texts, me, pair="aware")
        assert got == align_cases.ref_text(key)
        assert (last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]) == (0, 0, 0)


def test_invalid_values():
    d, texts, me, frag = align_pair_cases.inputs()["ambiguous"]
    for kw in (dict(pair=2), dict(pair=-1), dict(pair=1, search=1), dict(pair="aware", search="states_all")):
        with pytest.raises(capi.HgxError):
            _host(d, texts, me, **kw)
    with pytest.raises(KeyError):
        _host(d, texts, me, pair="together")


def test_one_mate_pairs_beside_rescued_pairs():
    """A mate without candidates (either one) beside rescued pairs: its pair is not searched and its record is the independent one."""
    d, texts, me, frag = align_pair_cases.inputs()["mixed"]
    got, last = _host(d, texts, me, max_fragment=frag, pair="aware")
    assert [f[0] for f in align_pair_cases.fields(got)] == [99, 147, 153, 99, 147, 73, 99, 147]
    assert (last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]) == (3, 3, 2)


def test_more_pairs_survive_the_typing_filter():
    """The reference's decode loop keeps a record with NH == 1 and FLAG & 2: a plain count over the written text."""
    for key in ("ambiguous", "rescue", "mixed"):
        d, texts, me, frag = align_pair_cases.inputs()[key]
        before = align_pair_cases.survivors(_host(d, texts, me, max_fragment=frag)[0])
        after = align_pair_cases.survivors(_host(d, texts, me, max_fragment=frag, pair="aware")[0])
        assert after > before, (key, before, after)
        assert (before, after) == {"ambiguous": (0, 1), "rescue": (0, 1), "mixed": (1, 3)}[key]


def test_align_reads_takes_the_pairs_name(tmp_path):
    """simulate.align_reads(aligner="hgx.pairs") stores the pair statement's records; more pairs survive the filter than with
    "hgx"; "linear" stays outside."""
    from hisatgenotype_amd import bamio, simulate
    d, texts, me, frag = align_pair_cases.inputs()["mixed"]
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    kept = {}
    for name in ("hgx", "hgx.pairs"):
        out = str(tmp_path / (name + ".bam"))
        with engine.test_switches(front="host"):
            simulate.align_reads(name, True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                                 var_list=Var_list, max_edits=me)
        assert align.align_last()["pairs_searched"] == (3 if name == "hgx.pairs" else 0)
        want = str(tmp_path / (name + ".want.bam"))
        text = align_pair_cases.ref_text("mixed") if name == "hgx.pairs" else _host(d, texts, me)[0]
        simulate._store_as_the_reference_does(want, text.decode())
        assert bamio.read_bam(out) == bamio.read_bam(want)
        kept[name] = align_pair_cases.survivors(text)
    assert kept["hgx.pairs"] > kept["hgx"]
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.pairs", True, "ix", "linear", "hla", paths, False, 1, str(tmp_path / "x.bam"), 0,
                             truth=(Genes, Vars, refGenes), var_list=Var_list)


def test_the_symbol_is_declared_and_bound():
    assert "hgx_align_last_pairs" in capi.SYMBOLS and hasattr(capi.lib(), "hgx_align_last_pairs")
