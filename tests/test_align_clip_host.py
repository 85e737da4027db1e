"""The clip tier on the host route of the "hgx" aligner (csrc/hgx_align_host.cpp, hgx_align_opts.clip, route forced with front=host):
the bytes of the plain-Python statement (tests/align_clip_ref.py), the counters of hgx_align_last_clip, clip = 0, the argument
checks, and the aligner name "hgx.clip".  No read of these inputs reaches the host route's step limit: every call asserts that the
"gave up" line was not written.  No GPU."""
import ctypes as C

import pytest

import align_cases
import align_clip_cases as cc
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
    return dict(searched=last["clip_searched"], clipped=last["clip_clipped"], bases=last["clip_bases"])


def _input(key):
    return cc.inputs()[key] if key in cc.inputs() else align_cases.inputs()[key] + (cc.CLIP,)


@pytest.mark.parametrize("key", cc.INPUT_IDS + align_cases.INPUT_IDS)
def test_host_route_equals_the_clip_statement(key, capfd):
    d, texts, me, clip = _input(key)
    got, last = _host(d, texts, me, capfd, clip=clip)
    st = {}
    want = cc.ref_text(key, stats=st)
    assert got == want
    recs = cc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == st
    if key in cc.inputs():
        assert st["clipped"] > 0
    s, c, b = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert capi.lib().hgx_align_last_clip(C.byref(s), C.byref(c), C.byref(b)) == 0
    assert dict(searched=s.value, clipped=c.value, bases=b.value) == st
    assert capi.lib().hgx_align_last_clip(None, None, None) == 0
    assert align.align_last_clip() == (st["searched"], st["clipped"], st["bases"])


@pytest.mark.parametrize("key", cc.INPUT_IDS + align_cases.INPUT_IDS)
def test_clip_0_gives_align_refs_bytes(key, capfd):
    d, texts, me, _ = _input(key)
    got, last = _host(d, texts, me, capfd, clip=0)
    assert got == (align_cases.ref_text(key) if key in align_cases.inputs() else cc.ref_text(key, clip=0))
    assert got == _host(d, texts, me)[0]
    assert _counters(last) == dict(searched=0, clipped=0, bases=0)


@pytest.mark.parametrize("clip", [1, 5, 21, 22, 255])
def test_other_budgets(clip, capfd):
    for key in ("chand0", "chand1", "chand3", "clengths"):
        d, texts, me, _ = cc.inputs()[key]
        st = {}
        want = cc.ref_text(key, clip=clip, stats=st)
        got, last = _host(d, texts, me, capfd, clip=clip)
        assert got == want and _counters(last) == st


@pytest.mark.parametrize("me", [0, 1, 3, 4])
def test_other_edit_budgets(me, capfd):
    import align_clip_ref
    import align_ref
    for key in ("chand2", "chand3", "overhang-err1"):
        d, texts, _, clip = cc.inputs()[key]
        loci = align_ref.loci_from_dicts(*d)
        want = align_clip_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me, clip=clip).encode()
        assert _host(d, texts, me, capfd, clip=clip)[0] == want


def test_random_loci_with_dense_variants(capfd):
    """60 seeded cases of align_clip_cases.random_case: small alphabets, known indels at and near the clip boundaries, ties."""
    clipped = 0
    for loci, reads, me, clip, want, st in cc.random_cases():
        got, last = _host(align_cases.dicts_of(loci), [cc.fasta(reads)], me, capfd, clip=clip)
        assert got == want and _counters(last) == st
        clipped += st["clipped"]
    assert clipped > 100


def test_files_on_disk(tmp_path, capfd):
    d, texts, me, clip = cc.inputs()["cpair-fastq-gz"]
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("r-%d.fq.gz" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    assert _host(d, paths, me, capfd, clip=clip)[0] == cc.ref_text("cpair-fastq-gz")
    assert b"80M20S" in cc.ref_text("cpair-fastq-gz")


def test_invalid_values():
    d, texts, me, _ = cc.inputs()["chand0"]
    for kw in (dict(clip=-1), dict(clip=256), dict(clip=32, search=1), dict(clip=32, search="states_all"), dict(clip=1, pair="aware"),
               dict(clip=32, max_edits=5)):
        with pytest.raises(capi.HgxError):
            _host(d, texts, **kw)
    _host(d, texts, max_edits=5, clip=0)                                    # the limit on max_edits is the tier's alone
    _host(d, texts, max_edits=4, clip=255)


def test_more_records_survive_the_front_ends_filters():
    """The overhang pairs through hgx_parse_sam: "hgx.clip" keeps pairs "hgx" loses (a pair with an unaligned mate is dropped)."""
    from hisatgenotype_amd import locus as hl
    loc, d, m1, m2 = cc.overhang_pairs(0.0)
    texts = [cc.fasta(m1), cc.fasta(m2)]
    pl = hl.PackedLocus.from_synth(loc)
    kept = {}
    for clip in (0, cc.CLIP):
        with engine.test_switches(front="host"):
            b = pl.parse_sam(_host(d, texts, 2, clip=clip)[0], num_editdist=2, simulation=False)
        assert engine.front_last() == (0, 0)
        kept[clip] = b.n_pairs
        b.close()
    assert kept[cc.CLIP] > kept[0] > 0


def test_align_reads_takes_the_clip_name(tmp_path):
    """simulate.align_reads(aligner="hgx.clip") stores the clip statement's records (clip = 32); "linear" stays outside."""
    from hisatgenotype_amd import bamio, simulate
    d, texts, me, clip = cc.inputs()["overhang-err1"]
    assert clip == align.NAMED_CLIP == 32
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    n = {}
    for name in ("hgx", "hgx.clip"):
        out = str(tmp_path / (name + ".bam"))
        with engine.test_switches(front="host"):
            simulate.align_reads(name, True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                                 var_list=Var_list, max_edits=me)
        assert (align.align_last()["clip_clipped"] > 0) == (name == "hgx.clip")
        want = str(tmp_path / (name + ".want.bam"))
        simulate._store_as_the_reference_does(want, cc.ref_text("overhang-err1", clip=clip if name == "hgx.clip" else 0).decode())
        assert bamio.read_bam(out) == bamio.read_bam(want)
        n[name] = len(bamio.read_bam(out))
    assert n["hgx.clip"] > n["hgx"]
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.clip", True, "ix", "linear", "hla", paths, False, 1, str(tmp_path / "x.bam"), 0,
                             truth=(Genes, Vars, refGenes), var_list=Var_list)


def test_the_symbol_is_declared_and_bound():
    assert "hgx_align_last_clip" in capi.SYMBOLS and hasattr(capi.lib(), "hgx_align_last_clip")
    assert [f[0] for f in align.AlignOpts._fields_][-1] == "clip"
