"""Coordinate order on the kernels' route of the "hgx" aligner (csrc/hgx_align.hip: k_aln_rec_keys, the stable radix sort,
k_aln_gather_lines; front=device) and the resident hand-off (hgx_align_reads_resident -> engine.Alignment): the kernels' text is
the statement (tests/align_resident_ref.py) applied to the read-order text and the host route's, at the lane / wavefront / chunk
edges of the read count, across a chunk edge, with lines of every length residue, with keys beyond 16 bits, where everything ties,
behind a decline and with nothing aligned; the resident object gives every locus the batch that the stored BAM gives it, with and
without its temporary-file fallback; typing() with typing_options.align_resident types as without it and leaves no file."""
import contextlib
import glob
import gzip
import importlib
import io
import os
import random
import threading

import numpy as np
import pytest

import align_cases
import align_ref
import align_rescue_cases as rc
from align_resident_ref import coordinate_order
from hisatgenotype_amd import align, engine, simulate
from hisatgenotype_amd.locus import PackedLocus

pytestmark = pytest.mark.gpu

CHUNK = 8192                         # reads per chunk of the device route (csrc/hgx_align.hip)
KEYS = rc.INPUT_IDS + align_cases.INPUT_IDS
FORMS = {"default": {}, "states_all": dict(search="states_all"), "pair_aware": dict(pair="aware"), "clip": dict(clip=32),
         "gap": dict(gap=16), "rescue": dict(rescue=(16, 32))}


def _run(d, texts, me=2, front="device", **kw):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front=front):
            out = ix.align(texts, max_edits=me, **kw)
        return out, align.align_last()
    finally:
        ix.close()


def _header(loci):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)


@pytest.mark.parametrize("form", list(FORMS))
def test_kernels_equal_the_statement_and_the_host_route(form):
    for key in KEYS:
        d, texts, me, _, _ = rc._input(key)
        plain, last0 = _run(d, texts, me, "host", **FORMS[form])
        want = coordinate_order(plain)
        assert _run(d, texts, me, "host", order="coordinate", **FORMS[form])[0] == want, key
        got, last = _run(d, texts, me, "device", order="coordinate", **FORMS[form])
        assert got == want, key
        # what a call reports whichever route gave the bytes (the states_* words count per route): as in read order
        same = [c for c in last if c not in ("route", "decline") and not c.startswith("states_")]
        assert [last[c] for c in same] == [last0[c] for c in same], key
        if last["reads"]:
            assert last["route"] == 2 or last["decline"] not in (0, align.DECLINE_SWITCH, align.DECLINE_GATE), (key, last)


_POOL = []


def _pool():
    """The hand-made loci of align_cases in one index, their reads, the statement's line (or None) per read, the header."""
    if not _POOL:
        loci, reads = [], []
        for _, ls, rs, _, _ in align_cases.hand_cases():
            loci += ls
            reads += rs
        lines = []
        for n, s in reads:
            body = [l for l in align_ref.align_text(loci, [[(n, s, None)]], 2).split("\n") if l and not l.startswith("@")]
            lines.append(body[0] if body else None)
        _POOL.append((loci, reads, lines, _header(loci)))
    return _POOL[0]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_read_counts_at_the_grid_and_chunk_edges(n):
    loci, reads, lines, header = _pool()
    pick = [(k * 7 + k // len(reads)) % len(reads) for k in range(n)]
    plain = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    got, last = _run(align_cases.dicts_of(loci), [align_cases.fasta([("q%d" % k, reads[j][1]) for k, j in enumerate(pick)])],
                     order="coordinate")
    assert got == coordinate_order(plain.encode())
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, n)
    assert last["aligned"] == sum(lines[j] is not None for j in pick)


def _lines_of(loci, named_reads):
    return [l for l in align_ref.align_text(loci, [[(n, s, None) for n, s in named_reads]]).split("\n") if l and not l.startswith("@")]


def test_the_last_read_of_the_second_chunk_sorts_first():
    """2 x CHUNK reads: all at one place but the last one, which lies left of them -- the only record that moves, over the chunk edge."""
    loc = align_cases.length_locus()
    at, left = _lines_of([loc], [("x", loc.bb[500:600]), ("x", loc.bb[100:200])])
    n = 2 * CHUNK
    recs = [("q%d" % k, loc.bb[500:600]) for k in range(n - 1)] + [("q%d" % (n - 1), loc.bb[100:200])]
    body = ["q%d\t%s\n" % (k, at.split("\t", 1)[1]) for k in range(n - 1)]
    last_line = "q%d\t%s\n" % (n - 1, left.split("\t", 1)[1])
    got, last = _run(align_cases.dicts_of([loc]), [align_cases.fasta(recs)], order="coordinate")
    want = (_header([loc]) + last_line + "".join(body)).encode()
    assert want == coordinate_order((_header([loc]) + "".join(body) + last_line).encode())
    assert got == want and (last["route"], last["decline"], last["aligned"]) == (2, 0, n)


def test_pairs_whose_mates_swap_across_chunks():
    """CHUNK / 2 + 1 pairs cycling through the pair cases ("rf", "out": mate 2 left of mate 1; "loci": on two loci), FASTQ."""
    m1, m2, _ = align_cases.pair_reads()
    loci = align_cases.pair_loci()
    per = []
    for k in range(len(m1)):
        text = align_ref.align_text(loci, [[("x", m1[k][1], "F" * 100)], [("x", m2[k][1], "5" * 100)]])
        per.append([l for l in text.split("\n") if l and not l.startswith("@")])
    n_pairs = CHUNK // 2 + 1
    pick = [(k * 3 + k // len(m1)) % len(m1) for k in range(n_pairs)]
    f1 = align_cases.fastq([("p%d" % k, m1[j][1], "F" * 100) for k, j in enumerate(pick)])
    f2 = align_cases.fastq([("p%d" % k, m2[j][1], "5" * 100) for k, j in enumerate(pick)])
    plain = (_header(loci) + "".join("p%d\t%s\n" % (k, l.split("\t", 1)[1]) for k, j in enumerate(pick) for l in per[j])).encode()
    for form in ({}, dict(pair="aware")):
        got, last = _run(align_cases.dicts_of(loci), [f1, f2], order="coordinate", **form)
        if not form:
            assert got == coordinate_order(plain)
        assert got == coordinate_order(_run(align_cases.dicts_of(loci), [f1, f2], **form)[0])
        assert (last["route"], last["decline"], last["reads"]) == (2, 0, 2 * n_pairs)
        assert last["pairs_concordant"] == sum(j < 2 for j in pick)


def test_lines_of_every_length_residue_are_gathered():
    """Read lengths 16 .. 256 in one call, the longer the further left: the order is reversed, and lines (SEQ and QUAL grow by one
    base each) and their offsets on both sides take every residue mod 4 and mod 16."""
    loc = align_cases.length_locus()
    reads = [("len%d" % n, loc.bb[320 + (256 - n) * 4:320 + (256 - n) * 4 + n]) for n in range(16, 257)]
    d = align_cases.dicts_of([loc])
    text = align_cases.fasta(reads)
    plain, _ = _run(d, [text], 2, "host")
    body = plain.split(b"\n")[1:-1]
    assert len(body) == 241
    assert {len(l) % 16 for l in body} == set(range(16))
    offs = np.cumsum([0] + [len(l) + 1 for l in body])
    assert {int(o) % 16 for o in offs} == set(range(16))
    want = coordinate_order(plain)
    assert want == plain.split(b"\n")[0] + b"\n" + b"".join(l + b"\n" for l in reversed(body))
    got, last = _run(d, [text], order="coordinate")
    assert got == want and (last["route"], last["decline"], last["aligned"]) == (2, 0, 241)


def test_keys_wider_than_sixteen_bits():
    """Three loci, the reads' loci descending; the middle locus has a 70 000-base backbone and reads beyond position 65 536."""
    loci = [align_ref.Locus("K0*BACKBONE", align_cases._bb(41, 900), []), align_ref.Locus("K1*BACKBONE", align_cases._bb(42, 70000), []),
            align_ref.Locus("K2*BACKBONE", align_cases._bb(43, 900), [])]
    reads = [("r2b", loci[2].bb[700:800]), ("r2a", loci[2].bb[5:105]), ("r1d", loci[1].bb[69000:69100]), ("r1c", loci[1].bb[65537:65637]),
             ("r1b", loci[1].bb[65535:65635]), ("r1a", loci[1].bb[1000:1100]), ("r1z", loci[1].bb[3464:3564]), ("r0b", loci[0].bb[300:400]),
             ("r0a", loci[0].bb[0:100])]
    d = align_cases.dicts_of(loci)
    text = align_cases.fasta(reads)
    plain, _ = _run(d, [text], 2, "host")
    assert [l.split(b"\t")[0] for l in plain.split(b"\n")[3:-1]] == [n.encode() for n, _ in reads]
    got, last = _run(d, [text], order="coordinate")
    assert got == coordinate_order(plain) and (last["route"], last["decline"]) == (2, 0)
    assert [l.split(b"\t")[0] for l in got.split(b"\n")[3:-1]] == [b"r0a", b"r0b", b"r1a", b"r1z", b"r1b", b"r1c", b"r1d", b"r2a", b"r2b"]
    assert [int(l.split(b"\t")[3]) for l in got.split(b"\n")[3:-1]][4:7] == [65536, 65538, 69001]


def test_hundreds_of_reads_at_one_position():
    loc = align_cases.length_locus()
    line = _lines_of([loc], [("x", loc.bb[700:800])])[0]
    recs = [("t%d" % ((k * 37) % 500), loc.bb[700:800]) for k in range(500)]
    got, last = _run(align_cases.dicts_of([loc]), [align_cases.fasta(recs)], order="coordinate")
    assert got == (_header([loc]) + "".join("%s\t%s\n" % (n, line.split("\t", 1)[1]) for n, _ in recs)).encode()
    assert (last["route"], last["decline"], last["aligned"]) == (2, 0, 500)


def test_a_decline_behind_a_full_first_chunk():
    """A read past the anchor slots (the 129-anchor input) in the second chunk: nothing of chunk one's text or table is kept, the
    host route writes the whole call in coordinate order."""
    loci, reads, lines, header = _pool()
    rep_loci, rep_reads = align_cases.limit_case("anchors", align_cases.DEV_ANCHORS + 1)
    all_loci = loci + rep_loci
    rep_line = _lines_of(all_loci, [("rep", rep_reads[0][1])])[0]
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, rep_reads[0])
    body = ["q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) if lines[j] is not None else "" for k, j in enumerate(pick)]
    body.insert(CHUNK + 8, rep_line + "\n")
    plain = (_header(all_loci) + "".join(body)).encode()
    got, last = _run(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)], order="coordinate")
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == coordinate_order(plain)
    assert last["aligned"] == plain.count(b"\n") - len(all_loci)


def test_no_aligned_read():
    loc = align_cases.length_locus()
    junk = align_cases.fasta([("j%d" % k, align_cases.rand_seq(random.Random(1000 + k), 90)) for k in range(70)])      # (seeds no backbone has)
    got, last = _run(align_cases.dicts_of([loc]), [junk], order="coordinate")
    assert got == _header([loc]).encode() and (last["route"], last["decline"], last["aligned"], last["reads"]) == (2, 0, 0, 70)


# ---- the resident object ---------------------------------------------------------------------------------------------------------
def test_resident_text_above_and_below_the_gate():
    """No switch: 65 reads stay below the aligner's 1 000-read gate (the host route's ordered text is uploaded), CHUNK + 1 take the
    kernels; both objects are resident and hold the statement's text."""
    loci, reads, lines, header = _pool()
    for n, route in ((65, 0), (CHUNK + 1, 2)):
        pick = [(k * 7 + k // len(reads)) % len(reads) for k in range(n)]
        plain = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
        ix = align.AlignIndex(*align_cases.dicts_of(loci))
        try:
            al = ix.align_resident([align_cases.fasta([("q%d" % k, reads[j][1]) for k, j in enumerate(pick)])])
            last = align.align_last()
            assert (last["route"], last["reads"]) == (route, n) and last["decline"] == (0 if route else align.DECLINE_GATE)
            assert al.resident and al.is_text and al.path is None
            want = coordinate_order(plain.encode())
            assert al.text() == want and al.stream_bytes == len(want)
            al.close()
        finally:
            ix.close()


_CALL = []


def _call():
    """The last typing() call of the golden self-test loop "pairs_two_genes" (loci A and B): its dicts, reads and arguments."""
    if not _CALL:
        import tempfile
        _CALL.append(align_cases.selftest_calls("pairs_two_genes", os.path.join(tempfile.mkdtemp(), "loop"))[-1])
    return _CALL[0]


def _batch_arrays(db):
    b = db.to_host()
    try:
        return (b.n_reads, b.n_pairs, b.pieces.tobytes(), b.masks.tobytes(), b.pair_off.tobytes(), b.pair_ref.tobytes())
    finally:
        b.close()


def _locus(call, gene):
    a = call["args"]
    return PackedLocus.cached_from_reference_dicts(gene, "hla", a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13])


def _read_texts(call):
    return [align_cases.fasta([(q, s) for q, s, _ in m]) for m in call["reads"]]


@pytest.mark.parametrize("aligner", ["hgx", "hgx.rescue"])
def test_every_locus_gets_the_batch_of_the_stored_file(aligner, tmp_path, monkeypatch):
    call = _call()
    monkeypatch.setenv("TMPDIR", str(tmp_path / "tmp"))
    (tmp_path / "tmp").mkdir()
    texts = _read_texts(call)
    ix = align.AlignIndex(call["Genes"], call["Vars"], call["Var_list"], call["refGenes"])
    form = simulate._hgx_form(aligner)
    stored, saved = str(tmp_path / "stored.bam"), str(tmp_path / "saved.bam")
    try:
        with engine.test_switches(front="device"):
            plain = ix.align(texts, max_edits=call["num_editdist"], **form)
            simulate._store_as_the_reference_does(stored, plain.decode())
            al = ix.align_resident(texts, max_edits=call["num_editdist"], **form)
            assert align.align_last()["route"] == 2 and al.resident
            assert al.text() == coordinate_order(plain)
            al.save(saved)
            want = {}
            with engine.Alignment(stored) as f_stored, engine.Alignment(saved) as f_saved:
                for gene in ("A", "B"):
                    pl = _locus(call, gene)
                    region = [call["refGenes"][gene]]
                    want[gene] = _batch_arrays(f_stored.parse_dev(pl, region, simulation=True))
                    assert want[gene][0] > 100
                    assert _batch_arrays(f_saved.parse_dev(pl, region, simulation=True)) == want[gene]
                    assert _batch_arrays(al.parse_dev(pl, region, simulation=True)) == want[gene]
            assert glob.glob(str(tmp_path / "tmp" / "*")) == []              # the kernels took every locus: no temporary file
        # front=host: every locus takes the per-path fallback, two loci on two threads at once, over ONE temporary BAM
        got, errs = {}, []

        def worker(gene):
            try:
                got[gene] = _batch_arrays(al.parse_dev(_locus(call, gene), [call["refGenes"][gene]], simulation=True))
            except BaseException as e:
                errs.append(e)
        with engine.test_switches(front="host"):
            ths = [threading.Thread(target=worker, args=(g,)) for g in ("A", "B")]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
        assert not errs and got == want
        tmp = glob.glob(str(tmp_path / "tmp" / "*"))
        assert len(tmp) == 1 and tmp[0].endswith(".bam")
        al.close()
        assert glob.glob(str(tmp_path / "tmp" / "*")) == []
    finally:
        ix.close()


# ---- typing() ----------------------------------------------------------------------------------------------------------------------
def _report_body(path):
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


def _result_numbers(res):
    return (res.num_reads, res.num_pairs, res.n_pieces, res.n_refs, None if res.counts is None else np.asarray(res.counts).tobytes(),
            [(e["n_classes"], e["n_iter"], [(n, float(p)) for n, p in e["result"]]) for e in res.em], [(n, float(p)) for n, p in res.gene_prob])


@pytest.mark.parametrize("aligner", ["hgx", "hgx.rescue"])
@pytest.mark.parametrize("locus_list", [["A"], ["A", "B"]])
def test_typing_types_the_same_without_the_file(aligner, locus_list, tmp_path, monkeypatch):
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")      # (the package's attribute `typing` is the function)
    call = _call()
    monkeypatch.chdir(tmp_path)
    paths = []
    for m, recs in enumerate(call["reads"]):
        paths.append(str(tmp_path / ("reads-%d.fq.gz" % (m + 1))))
        with open(paths[-1], "wb") as f:
            f.write(gzip.compress(align_cases.fastq([("frag%d" % k, s, "F" * len(s)) for k, (_, s, _) in enumerate(recs)])))
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    a = list(call["args"])
    a[0], a[2], a[14], a[19], a[24], a[25], a[26], a[27], a[34] = False, locus_list, [[aligner, "graph"]], False, True, paths, "", [], str(out_dir)
    report = str(out_dir / "assembly_graph-hla.reads-1_fq.report")
    seen = []
    real_lines = typing_mod.report_lines
    monkeypatch.setattr(typing_mod, "report_lines", lambda res, *r, **k: seen.append(_result_numbers(res)) or real_lines(res, *r, **k))
    real_store, stored = simulate._store_as_the_reference_does, []
    monkeypatch.setattr(simulate, "_store_as_the_reference_does", lambda *r, **k: stored.append(r[0]) or real_store(*r, **k))
    runs = {}
    for name, resident, keep in (("file", False, False), ("resident", True, False), ("resident-keep", True, True)):
        a[19] = keep
        del seen[:], stored[:]
        monkeypatch.setattr(typing_mod.typing_options, "align_resident", resident)
        with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
            typing_mod.typing(*a)
        assert align.align_last()["route"] == 2
        runs[name] = (_report_body(report), list(seen))
        assert len(seen) == len(locus_list) and all(s[0] > 100 for s in seen)
        assert bool(stored) == (not resident)                                   # with the option on, no file is ever written ...
        assert (glob.glob("*.bam") == ["reads-1_fq.bam"]) == keep and (keep or glob.glob("*.bam") == [])      # ... or left
    assert runs["resident"] == runs["file"] and runs["resident-keep"] == runs["file"]
    assert any("ranked" in l or "abundance" in l for l in runs["file"][0])
    # the kept file types the same when it is given
    a[19], a[26] = True, str(tmp_path / "reads-1_fq.bam")
    del seen[:]
    monkeypatch.setattr(typing_mod.typing_options, "align_resident", False)
    with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
        typing_mod.typing(*a)
    assert (_report_body(report), list(seen)) == runs["file"]


def test_a_linear_index_stays_outside(tmp_path, monkeypatch):
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")      # (the package's attribute `typing` is the function)
    call = _call()
    monkeypatch.chdir(tmp_path)
    a = list(call["args"])
    a[0], a[2], a[14], a[25], a[26], a[34] = False, ["A"], [["hgx", "linear"]], ["r.fq"], "", str(tmp_path)
    monkeypatch.setattr(typing_mod.typing_options, "align_resident", True)
    with pytest.raises(NotImplementedError), contextlib.redirect_stderr(io.StringIO()):
        typing_mod.typing(*a)
