"""The kernels of the "hgx" aligner (csrc/hgx_align.hip, front=device) give the Python statement's text (tests/align_ref.py) byte
for byte: on the host test's inputs, at the lane / wavefront / workgroup / scan-tile edges of the read count, with mixed read
lengths, one short of and one past every limit of their fixed scratch (past it the host route finishes the call), and under
genotyping_locus / typing() with the aligner name "hgx"."""
import contextlib
import gzip
import io
import json
import os

import pytest

import align_cases
import align_ref
from hisatgenotype_amd import align, bamio, engine, simulate

pytestmark = pytest.mark.gpu


def _device(d, texts, max_edits=2):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="device"):
            out = ix.align(texts, max_edits=max_edits)
        return out, align.align_last()
    finally:
        ix.close()


@pytest.mark.parametrize("key", align_cases.INPUT_IDS)
def test_device_route_equals_the_statement(key):
    d, texts, me = align_cases.inputs()[key]
    got, last = _device(d, texts, me)
    want = align_cases.ref_text(key)
    assert got == want
    if not key.startswith("empty"):
        assert (last["route"], last["decline"]) == (2, 0), last
    recs = [l for l in want.decode().split("\n") if l and not l.startswith("@")]
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2


def _hand_pool():
    """All hand-made loci in one index, their reads, and the statement's line (or None) per read."""
    loci, reads = [], []
    for _, ls, rs, _, _ in align_cases.hand_cases():
        loci += ls
        reads += rs
    lines = []
    for n, s in reads:
        body = [l for l in align_ref.align_text(loci, [[(n, s, None)]], 2).split("\n") if l and not l.startswith("@")]
        lines.append(body[0] if body else None)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)
    return loci, reads, lines, header


_POOL = []


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_read_counts_at_the_grid_edges(n):
    """Reads cycle through the hand-made cases; records stay in input order."""
    if not _POOL:
        _POOL.append(_hand_pool())
    loci, reads, lines, header = _POOL[0]
    assert sum(l is None for l in lines) == 2              # beyond two edits: "e3", and "lf" whose case allows four
    pick = [k % len(reads) for k in range(n)]
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta([reads[k] for k in pick])])
    want = header + "".join(lines[k] + "\n" for k in pick if lines[k] is not None)
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, n)


def test_mixed_read_lengths_in_one_call():
    lengths = list(range(16, align_cases.DEV_MAX_READ + 1, 7)) + [align_cases.DEV_MAX_READ, 15]
    loc = align_cases.length_locus()
    reads = align_cases.length_reads(lengths)
    got, last = _device(align_cases.dicts_of([loc]), [align_cases.fasta(reads)])
    assert got == align_ref.align_text([loc], [[(n, s, None) for n, s in reads]]).encode()
    assert (last["route"], last["decline"], last["aligned"]) == (2, 0, len(lengths) - 1)


@pytest.mark.parametrize("kind,limit,code", [("anchors", align_cases.DEV_ANCHORS, align.DECLINE_ANCHORS),
                                             ("stack", align_cases.DEV_STK, align.DECLINE_STACK),
                                             ("vars", align_cases.DEV_VARS, align.DECLINE_VARS),
                                             ("length", align_cases.DEV_MAX_READ, align.DECLINE_READ_LEN)])
def test_every_decline_limit(kind, limit, code):
    """At the limit the call stays on the device; one past it the kernels decline (nothing is written past their scratch) and the
    host route gives the bytes.  Either way the text is the statement's."""
    for n, route, dec in ((limit, 2, 0), (limit + 1, 0, code)):
        loci, reads = align_cases.limit_case(kind, n)
        want = align_ref.align_text(loci, [[(q, s, None) for q, s in reads]]).encode()
        assert want.count(b"\n") == 2                           # the read is aligned
        got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)])
        assert (last["route"], last["decline"]) == (route, dec), (n, last)
        assert got == want
        ix = align.AlignIndex(*align_cases.dicts_of(loci))
        assert ix.align([align_cases.fasta(reads)], route="host") == got
    if kind == "anchors":
        assert b"NH:i:%d\t" % (limit + 1) in got


def test_the_step_limit_declines():
    """HGX_ALN_DEV_STEPS (200 000 read bases walked per side of an anchor) is not a count an input can hit exactly: the two
    nearest inputs are used.  GATA x 30 whose every unit carries a known single that the read has too (so no 16-mer of the
    repeat seeds: 23 anchors, 30 variants, within the slots): with 12 + 12 known unit indels the read stays on the device (the
    kernels enumerate the ways through the repeat, without the host route's memo); with 13 + 13 they stop at the limit, nothing
    is written, and the host route gives the bytes."""
    for n, route, dec in ((12, 2, 0), (13, 0, align.DECLINE_STEPS)):
        loci, reads = align_cases.tandem_case(n, units=30, singles=4)
        want = align_ref.align_text(loci, [[(q, s, None) for q, s in reads]], prune=True).encode()
        assert want.count(b"\n") == 2
        got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)])
        assert (last["route"], last["decline"]) == (route, dec), (n, last)
        assert got == want


CHUNK = 8192                         # reads per chunk of the device route (csrc/hgx_align.hip)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_single_reads_across_chunks(n):
    """Everything that exists for a second chunk: the offsets into the read table, the per-chunk reset of the anchor counts and
    the decline word, each chunk's text appended in order, the counts summed."""
    if not _POOL:
        _POOL.append(_hand_pool())
    loci, reads, lines, header = _POOL[0]
    pick = [(k * 7 + k // len(reads)) % len(reads) for k in range(n)]          # (not the same read at the same place in every chunk)
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta([("q%d" % k, reads[j][1]) for k, j in enumerate(pick)])])
    want = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, n)
    assert last["aligned"] == sum(lines[j] is not None for j in pick)


@pytest.mark.parametrize("n_pairs", [CHUNK // 2 - 1, CHUNK // 2, CHUNK // 2 + 1, CHUNK + 1])
def test_pairs_across_chunks(n_pairs):
    """Mates stay together at the chunk edge (the chunk-local mate index), FLAG / PNEXT / YT are the mate's, concordant pairs are
    counted over all chunks.  Pairs cycle through the pair cases, FASTQ with qualities."""
    m1, m2, _ = align_cases.pair_reads()
    loci = align_cases.pair_loci()
    per = []
    for k in range(len(m1)):
        text = align_ref.align_text(loci, [[("x", m1[k][1], "F" * 100)], [("x", m2[k][1], "5" * 100)]])
        per.append([l for l in text.split("\n") if l and not l.startswith("@")])
    pick = [(k * 3 + k // len(m1)) % len(m1) for k in range(n_pairs)]
    f1 = align_cases.fastq([("p%d" % k, m1[j][1], "F" * 100) for k, j in enumerate(pick)])
    f2 = align_cases.fastq([("p%d" % k, m2[j][1], "5" * 100) for k, j in enumerate(pick)])
    got, last = _device(align_cases.dicts_of(loci), [f1, f2])
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)
    want = header + "".join("p%d\t%s\n" % (k, l.split("\t", 1)[1]) for k, j in enumerate(pick) for l in per[j])
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, 2 * n_pairs)
    assert last["pairs_concordant"] == sum(j < 2 for j in pick) and last["aligned"] == sum(len(per[j]) for j in pick)


def test_a_decline_in_the_second_chunk():
    """A read past the anchor slots behind a full first chunk: the first chunk's text and counts are taken back, the host route
    writes the whole call."""
    if not _POOL:
        _POOL.append(_hand_pool())
    loci, reads, lines, header = _POOL[0]
    rep_loci, rep_reads = align_cases.limit_case("anchors", align_cases.DEV_ANCHORS + 1)
    all_loci = loci + rep_loci
    rep_line = [l for l in align_ref.align_text(all_loci, [[("rep", rep_reads[0][1], None)]]).split("\n") if l and not l.startswith("@")][0]
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, rep_reads[0])
    body = ["q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) if lines[j] is not None else "" for k, j in enumerate(pick)]
    body.insert(CHUNK + 8, rep_line + "\n")
    want = (header + "@SQ\tSN:%s\tLN:%d\n" % (rep_loci[0].name, len(rep_loci[0].bb)) + "".join(body)).encode()
    got, last = _device(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)])
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == want
    assert last["aligned"] == want.count(b"\n") - len(all_loci)


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


@pytest.mark.parametrize("case,last_call", [("pairs_two_genes", 2), ("single_test_id_and_list", 1)])
def test_selftest_loop_with_the_aligner(case, last_call, tmp_path, monkeypatch):
    """genotyping_locus on the error-free golden cases with aligners=[["hgx", "graph"]]: the alignment file holds the records of
    the statement's text, and as many tests pass as in the recorded run (whose alignments were read off the read names)."""
    import hisatgenotype_amd as hgx
    spec = CASES[case]
    ix_dir, out_dir = tmp_path / "ix", tmp_path / "out"
    ix_dir.mkdir()
    out_dir.mkdir()
    for name, text in spec["index_files"].items():
        (ix_dir / name).write_text(text)
    p = spec["params"]
    monkeypatch.chdir(tmp_path)
    want_text = align_cases.ref_text("%s-%d" % (case, last_call)).decode()
    with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
        passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx", "graph"]], [], False, "",
                                      1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                      0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                      False, dict(p["debug"]))
    last = align.align_last()
    assert (last["route"], last["decline"]) == (2, 0), last
    simulate._store_as_the_reference_does(str(tmp_path / "want.bam"), want_text)
    got = bamio.read_bam(str(tmp_path / "hla_output.bam"))              # keep_alignment=True: the last test's file is still there
    assert got == bamio.read_bam(str(tmp_path / "want.bam")) and len(got) == last["aligned"] > 300
    total = [l for l in spec["stderr"].split("\n") if "passed (" in l][-1]
    assert passed == {"hgx graph": int(total.split("\t")[1].split("/")[0])}


def _body(path):
    with open(path) as f:
        lines = f.read().split("\n")
    out, k = [], 0
    while k < len(lines):
        if lines[k].startswith("# COMMAND"):
            k += 2
            continue
        if not lines[k].startswith("#"):
            out.append(lines[k])
        k += 1
    return out


def test_real_reads_mode(tmp_path, monkeypatch):
    """typing(simulation=False, read_fname=[-1.fq.gz, -2.fq.gz], alignment_fname=""): the reads of pairs_two_genes under names
    that spell nothing are aligned by the kernels and typed; the report is that of typing() on a BAM of the same records, and
    the alignment file is removed afterwards."""
    from hisatgenotype_amd.typing import typing
    call = align_cases.selftest_calls("pairs_two_genes", str(tmp_path / "loop"))[-1]
    monkeypatch.chdir(tmp_path)
    paths, texts = [], []
    for m, recs in enumerate(call["reads"]):
        texts.append(align_cases.fastq([("frag%d" % k, s, "F" * len(s)) for k, (_, s, _) in enumerate(recs)]))
        paths.append(str(tmp_path / ("reads-%d.fq.gz" % (m + 1))))
        with open(paths[-1], "wb") as f:
            f.write(gzip.compress(texts[-1]))
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    a = list(call["args"])
    a[0], a[2], a[14], a[19], a[24], a[25], a[26], a[27], a[34] = False, ["A", "B"], [["hgx", "graph"]], False, True, paths, "", [], str(out_dir)
    report = str(out_dir / "assembly_graph-hla.reads-1_fq.report")
    with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
        typing(*a)
    last = align.align_last()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, 832), last
    assert not os.path.exists("reads-1_fq.bam")
    first = _body(report)
    loci = align_ref.loci_from_dicts(call["Genes"], call["Vars"], call["Var_list"], call["refGenes"])
    want = align_ref.align_text(loci, [align_ref.read_records(t) for t in texts], call["num_editdist"])
    simulate._store_as_the_reference_does(str(tmp_path / "given.bam"), want)
    a[26] = str(tmp_path / "given.bam")
    with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
        typing(*a)
    second = _body(report)
    assert first == second and any("ranked" in l or "abundance" in l for l in first), first[:20]
    assert os.path.exists(a[26])


def test_the_old_aligner_name_still_goes_through_truth_align(tmp_path, monkeypatch):
    """["hisat2", "graph"] in simulation mode: truth_align, not the new aligner."""
    called = []
    monkeypatch.setattr(simulate, "truth_align", lambda *a, **k: called.append(a) or (_ for _ in ()).throw(KeyboardInterrupt()))
    with pytest.raises(KeyboardInterrupt):
        simulate.align_reads("hisat2", True, "ix", "graph", "hla", ["a.fa", "b.fa"], False, 1, str(tmp_path / "o.bam"), 0,
                             truth=({}, {}, {}), var_list={}, max_edits=2)
    assert len(called) == 1
