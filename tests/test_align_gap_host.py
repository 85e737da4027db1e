"""The gap tier on the host route of the "hgx" aligner (csrc/hgx_align_host.cpp, hgx_align_more.gap through hgx_align_reads_x, route
forced with front=host): the bytes of the plain-Python statement (tests/align_gap_ref.py), the counters of hgx_align_last_gap,
gap = 0, the new entry point's argument checks, and the aligner name "hgx.gap".  No read of these inputs reaches the host route's
step limit: every call asserts that the "gave up" line was not written.  No GPU."""
import ctypes as C

import pytest

import align_cases
import align_gap_cases as gc
import align_gap_ref
import align_ref
from hisatgenotype_amd import align, capi, engine


def _host(d, texts, max_edits=2, capfd=None, **kw):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="host"):
            out = ix.align(texts, max_edits=max_edits, **kw)
        last = align.align_last()
        assert last["route"] == 0 and last["decline"] == align.DECLINE_SWITCH
        if capfd is not None:
            assert "passed the host route's limits" not in capfd.readouterr().err      # nothing was left out silently
        return out, last
    finally:
        ix.close()


def _counters(last):
    return dict(searched=last["gap_searched"], gapped=last["gap_gapped"], bases=last["gap_bases"])


def _input(key):
    return gc.inputs()[key] if key in gc.inputs() else align_cases.inputs()[key] + (gc.GAP,)


@pytest.mark.parametrize("key", gc.INPUT_IDS + align_cases.INPUT_IDS)
def test_host_route_equals_the_gap_statement(key, capfd):
    d, texts, me, gap = _input(key)
    got, last = _host(d, texts, me, capfd, gap=gap)
    st = {}
    want = gc.ref_text(key, stats=st)
    assert got == want
    recs = gc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == st
    if key in gc.inputs() and key != "ghand1":
        assert st["gapped"] > 0
    s, g, b = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert capi.lib().hgx_align_last_gap(C.byref(s), C.byref(g), C.byref(b)) == 0
    assert dict(searched=s.value, gapped=g.value, bases=b.value) == st
    assert capi.lib().hgx_align_last_gap(None, None, None) == 0
    assert align.align_last_gap() == (st["searched"], st["gapped"], st["bases"])


@pytest.mark.parametrize("key", gc.INPUT_IDS + align_cases.INPUT_IDS)
def test_gap_0_gives_align_refs_bytes(key, capfd):
    d, texts, me, _ = _input(key)
    got, last = _host(d, texts, me, capfd, gap=0)
    assert got == (align_cases.ref_text(key) if key in align_cases.inputs() else gc.ref_text(key, gap=0))
    assert got == _host(d, texts, me)[0]
    assert _counters(last) == dict(searched=0, gapped=0, bases=0)


def _raw(ix, text, opts, more):
    """hgx_align_reads (more is False) or hgx_align_reads_x (more: None or an AlignMore) on one in-memory text: (rc, bytes)."""
    out_p, n = C.c_void_p(), C.c_size_t(0)
    texts, sizes = (C.c_char_p * 1)(text), (C.c_size_t * 1)(len(text))
    lib = capi.lib()
    with engine.test_switches(front="host"):
        if more is False:
            rc = lib.hgx_align_reads(ix.h, C.c_int32(1), None, texts, sizes, C.byref(opts), C.byref(out_p), C.byref(n))
        else:
            rc = lib.hgx_align_reads_x(ix.h, C.c_int32(1), None, texts, sizes, C.byref(opts), C.byref(more) if more is not None else None,
                                       C.byref(out_p), C.byref(n))
    try:
        return rc, C.string_at(out_p.value, n.value) if rc == 0 else None
    finally:
        if rc == 0:
            lib.hgx_free_text(out_p)


def test_the_entry_points():
    """hgx_align_reads, hgx_align_reads_x(more = NULL) and more.gap = 0 give the same bytes; more.bytes too small is refused; a
    larger more.bytes (a later caller) is read up to the fields this build knows."""
    d, texts, me, gap = gc.inputs()["ghand0"]
    ix = align.AlignIndex(*d)
    try:
        opts = align.AlignOpts(me, 1000, -1, 0, 0, 0, 0)
        rc0, plain = _raw(ix, texts[0], opts, False)
        assert rc0 == 0 and plain == gc.ref_text("ghand0", gap=0)
        assert _raw(ix, texts[0], opts, None) == (0, plain)
        assert _raw(ix, texts[0], opts, align.AlignMore(C.sizeof(align.AlignMore), 0)) == (0, plain)
        assert C.sizeof(align.AlignMore) == 8
        assert _raw(ix, texts[0], opts, align.AlignMore(8, gap)) == (0, gc.ref_text("ghand0"))
        assert align.align_last_gap()[1] > 0
        assert _raw(ix, texts[0], opts, False) == (0, plain) and align.align_last_gap() == (0, 0, 0)
        for small in (0, 4, 7, -1):
            rc, _ = _raw(ix, texts[0], opts, align.AlignMore(small, gap))
            assert rc == -1 and b"more.bytes" in capi.lib().hgx_last_error()      # HGX_EINVAL

        class Later(C.Structure):
            _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("later", C.c_int32 * 6)]
        assert _raw(ix, texts[0], opts, Later(C.sizeof(Later), gap)) == (0, gc.ref_text("ghand0"))
    finally:
        ix.close()


@pytest.mark.parametrize("gap", [1, 2, 16])
@pytest.mark.parametrize("me", [1, 2, 4])
def test_other_budgets(gap, me, capfd):
    for key in ("ghand0", "ghand4", "ghand7", "novel-err1"):
        d, texts, _, _ = gc.inputs()[key]
        st = {}
        want = gc.ref_text(key, gap=gap, stats=st, max_edits=me)
        got, last = _host(d, texts, me, capfd, gap=gap)
        assert got == want and _counters(last) == st


def test_max_edits_0_writes_no_gap(capfd):
    d, texts, _, _ = gc.inputs()["ghand0"]
    got, last = _host(d, texts, 0, capfd, gap=16)
    assert got == gc.ref_text("ghand0", max_edits=0) and got.count(b"\n") == 1 and _counters(last) == dict(searched=6, gapped=0, bases=0)


def test_random_loci_with_dense_variants(capfd):
    """The 60 seeds of align_gap_cases.RANDOM_SEEDS: small alphabets, known indels at and near the gaps, repeats and ties.  Every
    seed is compared, and every seed has a gapped record."""
    gapped = 0
    assert len(gc.random_cases()) == len(gc.RANDOM_SEEDS) == 60
    for seed, loci, reads, me, gap, want, st in gc.random_cases():
        got, last = _host(align_cases.dicts_of(loci), [gc.fasta(reads)], me, capfd, gap=gap)
        assert got == want and _counters(last) == st, seed
        assert st["gapped"] > 0, seed
        gapped += st["gapped"]
    assert gapped > 100


def test_files_on_disk(tmp_path, capfd):
    d, texts, me, gap = gc.inputs()["gpair-fastq-gz"]
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("r-%d.fq.gz" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    assert _host(d, paths, me, capfd, gap=gap)[0] == gc.ref_text("gpair-fastq-gz")
    assert b"50M1D50M" in gc.ref_text("gpair-fastq-gz")


def test_the_lengths():
    """Reads of 17 (no whole seed beside the gap: unaligned), 33, 100 and 1 024 bases with one novel deletion."""
    cig = [l.split("\t")[5] for l in gc.records(gc.ref_text("glengths"))]
    assert cig == ["17M1D16M", "50M1D50M", "100M1D924M"]


def test_invalid_values():
    d, texts, me, _ = gc.inputs()["ghand0"]
    for kw in (dict(gap=-1), dict(gap=17), dict(gap=16, search=1), dict(gap=1, search="states_all"), dict(gap=1, pair="aware"),
               dict(gap=16, clip=32), dict(gap=1, clip=1)):
        with pytest.raises(capi.HgxError):
            _host(d, texts, **kw)
    assert align.GAP_MAX == align.NAMED_GAP == align_gap_ref.GAP_MAX == 16
    _host(d, texts, max_edits=5, gap=16)                                    # (no limit on max_edits of the tier's own)
    _host(d, texts, gap=0, clip=32)
    _host(d, texts, gap=0, pair="aware")


def test_more_records_survive_the_front_ends_filters():
    """The synth pairs with novel indels through hgx_parse_sam: gap = 16 keeps pairs gap = 0 loses (a pair with an unaligned mate is
    dropped)."""
    from hisatgenotype_amd import locus as hl, synth
    d, texts, me, gap = gc.inputs()["novel-err1"]
    pl = hl.PackedLocus.from_synth(synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11))
    kept = {}
    for g in (0, gap):
        with engine.test_switches(front="host"):
            b = pl.parse_sam(_host(d, texts, me, gap=g)[0], num_editdist=2, simulation=False)
        assert engine.front_last() == (0, 0)
        kept[g] = b.n_pairs
        b.close()
    assert kept[gap] > kept[0] > 0


def test_align_reads_takes_the_gap_name(tmp_path):
    """simulate.align_reads(aligner="hgx.gap") stores the gap statement's records (gap = 16): more than "hgx"; "linear" stays
    outside."""
    from hisatgenotype_amd import bamio, simulate
    d, texts, me, gap = gc.inputs()["novel-err1"]
    assert gap == align.NAMED_GAP == 16
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    n = {}
    for name in ("hgx", "hgx.gap"):
        out = str(tmp_path / (name + ".bam"))
        with engine.test_switches(front="host"):
            simulate.align_reads(name, True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                                 var_list=Var_list, max_edits=me)
        assert (align.align_last()["gap_gapped"] > 0) == (name == "hgx.gap")
        want = str(tmp_path / (name + ".want.bam"))
        simulate._store_as_the_reference_does(want, gc.ref_text("novel-err1", gap=gap if name == "hgx.gap" else 0).decode())
        assert bamio.read_bam(out) == bamio.read_bam(want)
        n[name] = len(bamio.read_bam(out))
    assert n["hgx.gap"] > n["hgx"]
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.gap", True, "ix", "linear", "hla", paths, False, 1, str(tmp_path / "x.bam"), 0,
                             truth=(Genes, Vars, refGenes), var_list=Var_list)


def test_the_tier_counters_do_not_leak_between_calls(capfd):
    """The two tiers share one counter triple in the library: in calls that follow each other on one thread, each of
    hgx_align_last_clip and hgx_align_last_gap reports its own tier's call and zeros after the other tier's or a default call."""
    import align_clip_cases as cc
    cst, gst = {}, {}
    cc.ref_text("chand0", stats=cst)
    gc.ref_text("ghand0", stats=gst)
    assert cst["clipped"] > 0 and gst["gapped"] > 0
    want_clip, want_gap = (cst["searched"], cst["clipped"], cst["bases"]), (gst["searched"], gst["gapped"], gst["bases"])

    def six(which):
        d, texts, me, n = cc.inputs()["chand0"] if which != "gap" else gc.inputs()["ghand0"]
        last = _host(d, texts, me, capfd, **({} if which == "default" else {which: n}))[1]
        return ((last["clip_searched"], last["clip_clipped"], last["clip_bases"]), (last["gap_searched"], last["gap_gapped"], last["gap_bases"]))

    assert six("clip") == (want_clip, (0, 0, 0))
    assert six("gap") == ((0, 0, 0), want_gap)
    assert six("clip") == (want_clip, (0, 0, 0))
    assert six("default") == ((0, 0, 0), (0, 0, 0))
    assert six("gap") == ((0, 0, 0), want_gap)
    assert six("default") == ((0, 0, 0), (0, 0, 0))


def test_the_symbols_are_declared_and_bound():
    for name in ("hgx_align_reads_x", "hgx_align_last_gap"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert [f[0] for f in align.AlignOpts._fields_] == ["max_edits", "max_fragment", "fastq", "route", "search", "pair", "clip"]
    assert C.sizeof(align.AlignOpts) == 28
