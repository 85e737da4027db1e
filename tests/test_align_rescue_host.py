"""Both fallback tiers in one call on the host route of the "hgx" aligner (csrc/hgx_align_host.cpp: host_route<RescueTier>,
hgx_align_more.rescue_clip through hgx_align_reads_x, route forced with front=host): the bytes of the plain-Python statement
(tests/align_rescue_ref.py), both counter triples, the field's versions (bytes = 8 / 12), the HGX_EINVAL cases, the aligner name
"hgx.rescue", and the stand-alone host program (tools/align_host_main.cpp, rescue=G,C) on this file's inputs.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import align_cases
import align_rescue_cases as rc
from hisatgenotype_amd import align, capi, engine
from test_align_gap_host import _raw

ZERO = dict(searched=0, clipped=0, bases=0), dict(searched=0, gapped=0, bases=0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return (dict(searched=last["clip_searched"], clipped=last["clip_clipped"], bases=last["clip_bases"]),
            dict(searched=last["gap_searched"], gapped=last["gap_gapped"], bases=last["gap_bases"]))


@pytest.mark.parametrize("key", rc.INPUT_IDS + align_cases.INPUT_IDS)
def test_host_route_equals_the_statement(key, capfd):
    d, texts, me, gap, clip = rc._input(key)
    got, last = _host(d, texts, me, capfd, rescue=(gap, clip))
    st = {}
    want = rc.ref_text(key, stats=st)
    assert got == want
    recs = rc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == (st["clip"], st["gap"])
    assert align.align_last_clip() == tuple(st["clip"][c] for c in ("searched", "clipped", "bases"))
    assert align.align_last_gap() == tuple(st["gap"][c] for c in ("searched", "gapped", "bases"))
    # a following default call: every counter is zero again
    assert _counters(_host(d, texts, me)[1]) == ZERO


def test_random_loci_with_dense_variants(capfd):
    """The 40 seeds of align_rescue_cases.RANDOM_SEEDS: every seed is compared and has a clipped and a gapped record."""
    for seed, loci, reads, me, gap, clip, want, st in rc.random_cases():
        got, last = _host(align_cases.dicts_of(loci), [rc.fasta(reads)], me, capfd, rescue=(gap, clip))
        assert got == want and _counters(last) == (st["clip"], st["gap"]), seed
        assert st["clip"]["clipped"] > 0 and st["gap"]["gapped"] > 0, seed


@pytest.mark.parametrize("gap", [1, 16])
@pytest.mark.parametrize("clip", [1, 32, 255])
@pytest.mark.parametrize("me", [1, 2, 4])
def test_other_budgets(gap, clip, me, capfd):
    for key in ("rhand1", "rhand2", "rhand4", "mixed-err1"):
        d, texts, _, _, _ = rc.inputs()[key]
        st = {}
        want = rc.ref_text(key, gap=gap, clip=clip, stats=st, max_edits=me)
        got, last = _host(d, texts, me, capfd, rescue=(gap, clip))
        assert got == want and _counters(last) == (st["clip"], st["gap"]), key


class More12(C.Structure):
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("rescue_clip", C.c_int32)]


def test_the_versions_of_the_field():
    """bytes = 12 with rescue_clip = 0 gives the gap-only bytes; bytes = 8 with the 12-byte struct ignores the field; bytes < 8 stays
    HGX_EINVAL; a later, larger struct is read up to the fields this build knows."""
    d, texts, me, gap, clip = rc.inputs()["rhand1"]
    assert C.sizeof(align.AlignMore) == 8 and C.sizeof(align.AlignMoreRescue) == C.sizeof(More12) == 12
    assert [f[0] for f in align.AlignMoreRescue._fields_] == ["bytes", "gap", "rescue_clip"]
    ix = align.AlignIndex(*d)
    try:
        opts = align.AlignOpts(me, 1000, -1, 0, 0, 0, 0)
        gap_only = _raw(ix, texts[0], opts, align.AlignMore(8, gap))
        assert gap_only[0] == 0 and gap_only[1] != rc.ref_text("rhand1") and b"2I" in gap_only[1]
        only_counters = _counters(align.align_last())
        assert only_counters[0] == ZERO[0] and only_counters[1]["gapped"] > 0
        assert _raw(ix, texts[0], opts, More12(12, gap, 0)) == gap_only and _counters(align.align_last()) == only_counters
        assert _raw(ix, texts[0], opts, More12(8, gap, clip)) == gap_only and _counters(align.align_last()) == only_counters
        assert _raw(ix, texts[0], opts, More12(11, gap, clip)) == gap_only
        assert _raw(ix, texts[0], opts, More12(12, gap, clip)) == (0, rc.ref_text("rhand1"))
        assert _counters(align.align_last())[0]["clipped"] == 3
        for small in (0, 4, 7, -1):
            rc_, _ = _raw(ix, texts[0], opts, More12(small, gap, clip))
            assert rc_ == -1 and b"more.bytes" in capi.lib().hgx_last_error()

        class Later(C.Structure):
            _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("rescue_clip", C.c_int32), ("later", C.c_int32 * 5)]
        assert _raw(ix, texts[0], opts, Later(C.sizeof(Later), gap, clip)) == (0, rc.ref_text("rhand1"))
    finally:
        ix.close()


def test_invalid_values():
    d, texts, me, gap, clip = rc.inputs()["rhand1"]
    ix = align.AlignIndex(*d)
    try:
        def refused(opts, more, field):
            r, _ = _raw(ix, texts[0], opts, more)
            assert r == -1 and field in capi.lib().hgx_last_error(), (field, capi.lib().hgx_last_error())
        ok = align.AlignOpts(2, 1000, -1, 0, 0, 0, 0)
        refused(ok, More12(12, 0, 32), b"rescue_clip")                       # needs gap > 0
        refused(ok, More12(12, 16, -1), b"rescue_clip")
        refused(ok, More12(12, 16, 256), b"rescue_clip")
        refused(align.AlignOpts(5, 1000, -1, 0, 0, 0, 0), More12(12, 16, 32), b"rescue_clip")      # max_edits <= 4
        refused(align.AlignOpts(2, 1000, -1, 0, 1, 0, 0), More12(12, 16, 32), b"gap")              # search = ways
        refused(align.AlignOpts(2, 1000, -1, 0, 0, 1, 0), More12(12, 16, 32), b"gap")              # pair = independent
        refused(align.AlignOpts(2, 1000, -1, 0, 0, 0, 32), More12(12, 16, 32), b"gap")             # opts.clip = 0
        refused(align.AlignOpts(2, 1000, -1, 0, 0, 0, 32), More12(12, 16, 0), b"gap")              # (as before: one of clip= and gap=)
        refused(ok, More12(12, 17, 32), b"gap")
        assert _raw(ix, texts[0], align.AlignOpts(4, 1000, -1, 0, 0, 0, 0), More12(12, 16, 255))[0] == 0
    finally:
        ix.close()
    for kw in (dict(rescue=(16, 32), clip=32), dict(rescue=(16, 32), search="states"), dict(rescue=(16, 32), pair="aware"),
               dict(rescue=(0, 32)), dict(rescue=(16, 256)), dict(rescue=(16, 32), max_edits=5), dict(gap=16, clip=32), dict(gap=1, clip=1)):
        with pytest.raises(capi.HgxError):
            _host(d, texts, **kw)
    with pytest.raises(ValueError):
        _host(d, texts, rescue=(16, 32), gap=16)
    assert align.NAMED_RESCUE == (align.NAMED_GAP, align.NAMED_CLIP) == (rc.GAP, rc.CLIP)
    _host(d, texts, rescue=(16, 0))                                           # (rescue_clip = 0: the gap tier alone)
    assert _counters(align.align_last())[0] == ZERO[0]


def test_files_on_disk(tmp_path, capfd):
    d, texts, me, gap, clip = rc.inputs()["rpair-fastq-gz"]
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("r-%d.fq.gz" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    want = rc.ref_text("rpair-fastq-gz")
    assert _host(d, paths, me, capfd, rescue=(gap, clip))[0] == want
    assert b"3S97M" in want and b"50M1D50M" in want and want.count(b"YT:Z:CP") == 4


def test_the_lengths():
    cig = [l.split("\t")[5] for l in rc.records(rc.ref_text("glengths"))]
    assert cig == ["17M1D16M", "50M1D50M", "100M1D924M"]
    cig = [l.split("\t")[5] for l in rc.records(rc.ref_text("clengths"))]
    assert cig == ["16M", "16M1S", "97M3S", "1021M3S"]


def test_more_pairs_survive_the_front_end_than_under_either_tier():
    """The mixed synth pairs through hgx_parse_sam: "hgx.rescue" keeps pairs that "hgx.clip" and "hgx.gap" each lose."""
    from hisatgenotype_amd import locus as hl, synth
    d, texts, me, gap, clip = rc.inputs()["mixed-err1"]
    pl = hl.PackedLocus.from_synth(synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11))
    kept = {}
    for name, kw in (("rescue", dict(rescue=(gap, clip))), ("clip", dict(clip=clip)), ("gap", dict(gap=gap))):
        with engine.test_switches(front="host"):
            b = pl.parse_sam(_host(d, texts, me, **kw)[0], num_editdist=2, simulation=False)
        assert engine.front_last() == (0, 0)
        kept[name] = b.n_pairs
        b.close()
    assert kept["rescue"] > kept["clip"] > 0 and kept["rescue"] > kept["gap"] > 0


def test_align_reads_takes_the_rescue_name(tmp_path):
    """simulate.align_reads(aligner="hgx.rescue") stores the statement's records (rescue = (16, 32)); "linear" stays outside."""
    from hisatgenotype_amd import bamio, simulate
    d, texts, me, gap, clip = rc.inputs()["mixed-err1"]
    Genes, Vars, Var_list, refGenes = d
    paths = []
    for m, t in enumerate(texts):
        p = tmp_path / ("in_%d.fa" % (m + 1))
        p.write_bytes(t)
        paths.append(str(p))
    out = str(tmp_path / "rescue.bam")
    with engine.test_switches(front="host"):
        simulate.align_reads("hgx.rescue", True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(Genes, Vars, refGenes),
                             var_list=Var_list, max_edits=me)
    last = align.align_last()
    assert last["gap_gapped"] > 0 and last["clip_clipped"] > 0
    want = str(tmp_path / "want.bam")
    simulate._store_as_the_reference_does(want, rc.ref_text("mixed-err1").decode())
    assert bamio.read_bam(out) == bamio.read_bam(want)
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.rescue", True, "ix", "linear", "hla", paths, False, 1, str(tmp_path / "x.bam"), 0,
                             truth=(Genes, Vars, refGenes), var_list=Var_list)


def test_genotyping_locus_takes_the_rescue_name(tmp_path, monkeypatch):
    """genotyping_locus with aligners=[["hgx.rescue", "graph"]] hands the name to every typing() call of the self-test loop (typing
    itself needs a GPU: tests/test_gpu_align_rescue.py runs the loop), and align_reads under that name, on the reads and dicts of
    such a call, stores the statement's records."""
    from hisatgenotype_amd import bamio, driver, simulate
    import align_ref
    import align_rescue_ref
    calls = align_cases.selftest_calls("pairs_two_genes", str(tmp_path / "plain"))
    seen = []
    monkeypatch.setattr(driver, "typing", lambda *a, **k: seen.append(a) or {})
    import contextlib
    import gzip
    import io
    import json
    import hisatgenotype_amd as hgx
    with gzip.open(os.path.join(ROOT, "tests", "golden", "selftest_loop.json.gz"), "rb") as f:
        spec = json.loads(f.read().decode())["pairs_two_genes"]
    ix_dir, out_dir = tmp_path / "ix", tmp_path / "out"
    ix_dir.mkdir()
    out_dir.mkdir()
    for name, text in spec["index_files"].items():
        (ix_dir / name).write_text(text)
    p = spec["params"]
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stderr(io.StringIO()):
        hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx.rescue", "graph"]], [], False, "", 1,
                             p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"], 0.0, [], False,
                             "assembly_graph", True, False, False, False, True, [], 0, False, str(out_dir), False, dict(p["debug"]))
    assert len(seen) == len(calls) > 0 and all(a[14] == [["hgx.rescue", "graph"]] for a in seen)
    c = calls[0]
    paths = []                                                            # (the loop writes every test's reads to the same two files)
    for m, recs in enumerate(c["reads"]):
        paths.append(str(tmp_path / ("call0_%d.fa" % (m + 1))))
        with open(paths[-1], "wb") as f:
            f.write(align_cases.fasta([(n, q) for n, q, _ in recs]))
    out = str(tmp_path / "rescue.bam")
    with engine.test_switches(front="host"):
        simulate.align_reads("hgx.rescue", True, "ix", "graph", "hla", paths, False, 1, out, 0, truth=(c["Genes"], c["Vars"], c["refGenes"]),
                             var_list=c["Var_list"], max_edits=c["num_editdist"])
    loci = align_ref.loci_from_dicts(c["Genes"], c["Vars"], c["Var_list"], c["refGenes"])
    want = str(tmp_path / "want.bam")
    simulate._store_as_the_reference_does(want, align_rescue_ref.align_text(loci, c["reads"], c["num_editdist"], gap=rc.GAP, clip=rc.CLIP))
    assert bamio.read_bam(out) == bamio.read_bam(want)


def _write_index(path, d):
    Genes, Vars, Var_list, refGenes = d
    types = {"insertion": 0, "single": 1, "deletion": 2}
    with open(path, "w") as f:
        f.write("%d\n" % len(Genes))
        for g in Genes:
            vl = Var_list.get(g, [])
            f.write("%s %s %d\n" % (refGenes[g], Genes[g][refGenes[g]], len(vl)))
            for _, v in vl:
                t, p, data = Vars[g][v][:3]
                f.write("%d %d %s %s\n" % (types[t], p, data, v))


def test_the_stand_alone_host_program_under_asan_and_ubsan(tmp_path):
    """tools/align_host_main.cpp with rescue=16,32, built with -fsanitize=address,undefined (a program with its own main; nothing of
    the GPU library, nothing loaded into Python): the statement's bytes and no sanitizer report on every input of this file."""
    exe = str(tmp_path / "align_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DHGX_ALIGN_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hisat-genotype_amd", "csrc"),
                           os.path.join(ROOT, "hisat-genotype_amd", "csrc", "hgx_align_host.cpp"), os.path.join(ROOT, "tools", "align_host_main.cpp"),
                           "-lz", "-o", exe])

    def run(d, texts, me, gap, clip, tag):
        ix = str(tmp_path / (tag + ".ix"))
        _write_index(ix, d)
        paths = []
        for m, t in enumerate(texts):
            p = str(tmp_path / ("%s_%d.in" % (tag, m)))
            with open(p, "wb") as f:
                f.write(t)
            paths.append(p)
        r = subprocess.run([exe, ix, str(me)] + paths + ["rescue=%d,%d" % (gap, clip)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stderr == b"", (tag, r.stderr[-2000:])
        return r.stdout

    for key in rc.INPUT_IDS + align_cases.INPUT_IDS:
        d, texts, me, gap, clip = rc._input(key)
        assert run(d, texts, me, gap, clip, key) == rc.ref_text(key), key
    for seed, loci, reads, me, gap, clip, want, st in rc.random_cases():
        assert run(align_cases.dicts_of(loci), [rc.fasta(reads)], me, gap, clip, "seed%d" % seed) == want, seed
