"""The host route of the "hgx" aligner on a linear index (csrc/hgx_align_linear_host.cpp) against the plain statement
(tests/align_linear_ref.py) over the case table, in FASTA, FASTQ and gzip; its counters and refused options; simulate.align_reads
and typing() with ["hgx", "linear"] and reads to align.  No GPU: route="host" (typing(): the test switch front=host)."""
import contextlib
import gzip
import importlib
import io
import os
import random
import threading

import pytest

import align_linear_cases as lc
import align_linear_ref as ref
import linear_ref
from hisatgenotype_amd import align, bamio, capi, engine, simulate, synth


def _host(c, reads=None, fastq=None):
    ix = align.LinearAlignIndex(c["Genes"], c["refGenes"])
    try:
        got = ix.align(lc.texts(c) if reads is None else reads, max_edits=c["max_edits"], k=c["k"], fastq=fastq, route="host")
        return got, align.align_linear_last()
    finally:
        ix.close()


@pytest.mark.parametrize("name", lc.NAMES)
def test_host_route_writes_the_statements_bytes(name):
    c = lc.BY_NAME[name]
    got, last = _host(c)
    assert got == lc.ref_text(name)
    alleles = ref.index_of(c["Genes"], c["refGenes"])
    n, aligned, records = ref.counters(alleles, c["reads"], c["max_edits"], c["k"])
    assert (last["route"], last["decline"]) == (0, align.LINEAR_DECLINE_SWITCH)
    assert (last["reads"], last["aligned"], last["records"]) == (n, aligned, records)
    if not name.startswith("reads-"):
        assert last["candidates"] == sum(ref.candidates(alleles, s, c["max_edits"]) for recs in c["reads"] for _, s, _ in recs)


@pytest.mark.parametrize("name", ["pairs", "n-bases", "length-257"])
def test_input_forms(name, tmp_path):
    """FASTA and FASTQ, as texts, gzip texts, files and gzip files: the loader is the graph aligner's.  Qualities are kept."""
    c = lc.BY_NAME[name]
    want = lc.ref_text(name)
    fq = [lc.fastq(r) for r in c["reads"]]
    want_fq = ref.align_text(ref.index_of(c["Genes"], c["refGenes"]), [ref.read_records(t) for t in fq], c["max_edits"], c["k"]).encode()
    assert _host(c, lc.texts(c))[0] == want
    assert _host(c, [gzip.compress(t) for t in lc.texts(c)])[0] == want
    assert _host(c, fq)[0] == want_fq and _host(c, fq, fastq=True)[0] == want_fq
    paths = []
    for m, t in enumerate(fq):
        paths.append(str(tmp_path / ("r%d.fq.gz" % m)))
        with open(paths[-1], "wb") as f:
            f.write(gzip.compress(t))
    assert _host(c, paths)[0] == want_fq
    plain = []
    for m, t in enumerate(lc.texts(c)):
        plain.append(str(tmp_path / ("r%d.txt" % m)))
        with open(plain[-1], "wb") as f:
            f.write(t)
    assert _host(c, plain)[0] == want
    if not lc.texts(c)[0].startswith(b"@"):                    # lower-case bases are upper-cased by the loader
        lower = [b"".join((l if l.startswith(b">") else l.lower()) + b"\n" for l in t.split(b"\n") if l) for t in lc.texts(c)]
        assert lower != lc.texts(c) and _host(c, lower)[0] == want


def test_refused_options():
    c = lc.BY_NAME["pairs"]
    ix = align.LinearAlignIndex(c["Genes"], c["refGenes"])
    try:
        for kw in (dict(max_edits=-1), dict(max_edits=5), dict(k=0), dict(k=1025)):
            with pytest.raises(capi.HgxError) as e:
                ix.align(lc.texts(c), route="host", **kw)
            assert e.value.code == -1 and ("max_edits" if "max_edits" in kw else "k is") in str(e.value)
        assert ix.align(lc.texts(c), route="host", max_edits=4, k=1024)
        opts = align.AlignLinearOpts(8, 2, 10, -1, 1)                # bytes below the struct's size
        import ctypes as C
        out_p, n = C.c_void_p(), C.c_size_t(0)
        bufs = lc.texts(c)
        rc = capi.lib().hgx_align_linear_reads(ix.h, C.c_int32(2), None, (C.c_char_p * 2)(*bufs), (C.c_size_t * 2)(*[len(b) for b in bufs]),
                                               C.byref(opts), C.byref(out_p), C.byref(n))
        assert rc == -1
    finally:
        ix.close()
    with pytest.raises(capi.HgxError):
        align.LinearAlignIndex({"G": {"G*BACKBONE": "ACGT"}}, {"G": "G*BACKBONE"})        # nothing but the backbone: no sequence to index


def test_limits_of_the_index():
    """The key has 20 bits for the allele and 20 for the position: the index build takes a sequence of 2^20 - 1 bases and refuses one
    of 2^20; it refuses 2^20 sequences (the table's cases stop at 66 000: 2^20 - 1 sequences would be a header of 20 MB).  An empty
    sequence is accepted (the case short-and-lower-alleles aligns to such an index)."""
    import ctypes as C

    def create(names, seqs):
        h = C.c_void_p()
        try:
            capi.check(capi.lib().hgx_align_linear_index_create(C.byref(h), C.c_int32(len(names)), (C.c_char_p * len(names))(*names),
                                                                (C.c_char_p * len(seqs))(*seqs)))
        finally:
            if h:
                capi.lib().hgx_align_linear_index_free(h)
    longest = lc.rnd_long(7, (1 << 20) - 1).encode()
    create([b"short", b"longest"], [b"ACGT" * 5, longest])
    with pytest.raises(capi.HgxError) as e:
        create([b"short", b"longer"], [b"ACGT" * 5, longest + b"A"])
    assert e.value.code == -1 and "sequence 1 has 1048576 bases" in str(e.value) and "2^20 - 1" in str(e.value)
    create([b"a", b"empty"], [b"ACGT" * 5, b""])
    n = 1 << 20
    with pytest.raises(capi.HgxError) as e:
        create([b"s"] * n, [b"ACGTACGTACGTACGTACGT"] * n)
    assert e.value.code == -1 and "1048576 sequences" in str(e.value) and "2^20 - 1" in str(e.value)


def test_index_order_and_cache():
    Genes = {"B": {"B*BACKBONE": "AC", "B*02": "ACGT", "B*01": "AAAA"}, "A": {"A*01": "CC", "A*BACKBONE": "GG"}}
    refGenes = {"B": "B*BACKBONE", "A": "A*BACKBONE"}
    assert [n for n, _ in align.linear_alleles(Genes, refGenes)] == ["B*02", "B*01", "A*01"] == [n for n, _ in ref.index_of(Genes, refGenes)]
    ix = align.cached_linear_index(Genes, refGenes)
    assert align.cached_linear_index(Genes, refGenes) is ix and ix.names == ["B*02", "B*01", "A*01"]
    assert align.cached_linear_index(dict(Genes), refGenes) is not ix


def test_align_reads_writes_a_coordinate_sorted_bam(tmp_path):
    c = lc.BY_NAME["pairs"]
    paths = []
    for m, t in enumerate(lc.texts(c)):
        paths.append(str(tmp_path / ("r%d.fq" % m)))
        with open(paths[-1], "wb") as f:
            f.write(t)
    out = str(tmp_path / "o.bam")
    with engine.test_switches(front="host"):
        simulate.align_reads("hgx", False, "ix", "linear", "codis", paths, True, 1, out, 0, truth=(c["Genes"], {}, c["refGenes"]), var_list={})
    want = str(tmp_path / "want.bam")
    simulate._store_as_the_reference_does(want, lc.ref_text("pairs").decode())
    got = bamio.read_bam(out)
    assert got == bamio.read_bam(want) and len(got) == 60
    names = [n for n, _ in ref.index_of(c["Genes"], c["refGenes"])]
    keys = [(names.index(l.split("\t")[2]), int(l.split("\t")[3])) for l in got]
    assert keys == sorted(keys)
    for name in ("hgx.states", "hgx.pairs", "hgx.clip", "hgx.gap", "hgx.rescue"):
        with pytest.raises(NotImplementedError, match="linear index"):
            simulate.align_reads(name, False, "ix", "linear", "codis", paths, True, 1, out, 0, truth=(c["Genes"], {}, c["refGenes"]), var_list={})
    with pytest.raises(NotImplementedError, match="simulation"):
        simulate.align_reads("hgx", True, "ix", "linear", "codis", paths, True, 1, out, 0, truth=(c["Genes"], {}, c["refGenes"]), var_list={})


# ---- typing() ----------------------------------------------------------------------------------------------------------------------
def _section(report_path, aligner="hgx"):
    text = open(report_path).read()
    return text[text.index("\n\t\t%s linear" % aligner):]


def typing_call(tmp_path, monkeypatch, em_on_gpu=True):
    """typing() on a small non-HLA synth locus with reads of simulate.simulate_reads passed as read_fname, aligners = [["hgx", "linear"]],
    in both forms; asserts each against linear_ref.run and returns dict(reports, routes).  em_on_gpu=False: the abundance step, the
    one part of this chain that has no host form (the existing EM kernels), is replaced by the oracle's EM -- aligner, stored file,
    record pass, groups, classes, counts and report are the library's."""
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")      # (the package's attribute `typing` is the function)
    if not em_on_gpu:
        import pyref

        def oracle_em(classes):
            st = {}
            return pyref.single_abundance(classes, False, None, st), st.get("n_iter")
        monkeypatch.setattr(typing_mod, "_single_abundance", oracle_em)
    loc = synth.make_str_like_locus(seed=3)
    d = loc.reference_dicts()
    monkeypatch.chdir(tmp_path)
    state = random.getstate()
    try:
        random.seed(11)
        simulate.simulate_reads(d["Genes"], "lin", [[loc.allele_names[3], loc.allele_names[7]]], d["Vars"], d["Links"], simulate_interval=3,
                                perbase_errorrate=0.5, out_dir=str(tmp_path))
    finally:
        random.setstate(state)
    reads = [str(tmp_path / ("lin_input_%d.fa" % m)) for m in (1, 2)]
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    stored = []
    real_store = simulate._store_as_the_reference_does
    monkeypatch.setattr(simulate, "_store_as_the_reference_does", lambda path, text: stored.append((path, text)) or real_store(path, text))

    def run(read_order, keep=False):
        monkeypatch.setattr(typing_mod.typing_options, "linear_read_order", read_order)
        del stored[:]
        # On a thread of its own.  The library's last-call records are per thread, and the linear typing sets engine.front_last
        # (here to (0, 2): front=host).  tests/test_align_rescue_host.py::test_more_pairs_survive_the_front_end_than_under_either_tier
        # asserts engine.front_last() == (0, 0) behind pl.parse_sam under front=host, a call that does not set the record: it reads
        # what the last setter on ITS thread left, and this file runs in front of it.  That order dependence is the older test's;
        # keeping these calls off the main thread leaves it as it was.  The route asserted below is align_linear_last() of this
        # worker thread, read on the worker itself (box["route"])
        box = {}

        def call():
            try:
                typing_mod.typing(False, str(tmp_path / loc.base_fname), [loc.gene], "", True, set(), d["refGenes"], d["Genes"], d["Gene_names"],
                                  d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"], [["hgx", "linear"]], 2, False,
                                  "assembly_graph", True, keep, False, False, True, [], False, reads, "", [], 100, 250, 1, False, 0, False,
                                  str(out_dir), "NONE", False, 0)
                box["route"] = align.align_linear_last()["route"]
            except BaseException as e:
                box["error"] = e
        with contextlib.redirect_stderr(io.StringIO()):
            t = threading.Thread(target=call)
            t.start()
            t.join()
        if "error" in box:
            raise box["error"]
        rep = [f for f in os.listdir(str(out_dir)) if f.endswith(".report")]
        assert len(rep) == 1
        return _section(str(out_dir / rep[0])), box["route"]

    alleles = ref.index_of(d["Genes"], d["refGenes"])
    text = ref.align_text(alleles, [ref.read_records(p) for p in reads], 2, 10)
    assert text.count("\n") > 400

    def expected(records_text):
        exp = linear_ref.run(records_text, loc.gene, "hisat2", False)
        assert exp["error"] is None and len(exp["gene_prob"]) > 1
        return "\n\t\thgx linear\n" + "\n".join(linear_ref.report_lines(exp["counts_sorted"], exp["gene_prob"])) + "\n"

    # the default form: the stored, coordinate-sorted file typed in file order; the file is removed afterwards
    default, route_a = run(False)
    assert len(stored) == 1 and stored[0][1] == text and not os.path.exists(stored[0][0])
    bam = str(tmp_path / "again.bam")
    real_store(bam, text)
    assert default == expected("\n".join(bamio.read_bam(bam)) + "\n")
    # read order: the aligner's text typed from memory, nothing stored
    ordered, route_b = run(True)
    assert stored == [] and [f for f in os.listdir(str(tmp_path)) if f.endswith(".bam")] == ["again.bam"]
    assert ordered == expected("".join(l + "\n" for l in text.split("\n") if l and not l.startswith("@")))
    assert ordered != default
    # keep_alignment leaves the stored file in either form
    run(True, keep=True)
    assert len(stored) == 1 and os.path.exists(stored[0][0]) and bamio.read_bam(stored[0][0]) == bamio.read_bam(bam)
    return dict(reports=[default, ordered], routes=[route_a, route_b])


def test_typing_aligns_the_reads_first(tmp_path, monkeypatch):
    with engine.test_switches(front="host"):
        out = typing_call(tmp_path, monkeypatch, em_on_gpu=False)
    assert out["routes"] == [0, 0]


def test_typing_linear_keeps_raising_where_it_is_not_built(tmp_path, monkeypatch):
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")
    loc = synth.make_str_like_locus(seed=3)
    d = loc.reference_dicts()
    monkeypatch.chdir(tmp_path)

    def call(simulation, aligner, locus_list):
        with contextlib.redirect_stderr(io.StringIO()):
            typing_mod.typing(simulation, str(tmp_path / loc.base_fname), locus_list, "", True, set(), d["refGenes"], d["Genes"], d["Gene_names"],
                              d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"], [[aligner, "linear"]], 2, False,
                              "assembly_graph", True, False, False, False, True, [], False, ["r.fa"], "", [], 100, 250, 1, False, 0, False,
                              str(tmp_path), "NONE", False, 0)
    with pytest.raises(NotImplementedError, match="simulation"):
        call(True, "hgx", [[loc.allele_names[1]]])
    for aligner in ("hisat2", "hgx.gap"):
        with pytest.raises(NotImplementedError, match="linear index"):
            call(False, aligner, [loc.gene])
    monkeypatch.setattr(typing_mod.typing_options, "align_resident", True)
    with pytest.raises(NotImplementedError, match="align_resident"):
        call(False, "hgx", [loc.gene])
