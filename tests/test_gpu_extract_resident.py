"""The extractor that keeps its text for the aligner (hgx_extract_keep / hgx_extract_take_reads: Extractor(keep=True).take_reads):
for every family the object's records are the plain statement's (tests/reads_table_ref.py) over the FASTA / FASTQ text that a
second handle WITHOUT keep hands out -- one device chunk, a device chunk followed by a host chunk (the segments mix), a BAM in
three chunks; paired FASTQ, single-end, FASTA; a record with SEQ '*'; Reads.save; the stats of both handles; take() on a keep
handle.  End to end: a genome-wide stream typed through extract_reads_resident -> typing_options.reads -> typing() gives the report
of the file route."""
import contextlib
import glob
import gzip
import importlib
import io
import os
import random

import numpy as np
import pytest

import extract_bam_cases as X
import extract_ref
import reads_table_ref as ref
from hisatgenotype_amd import align, capi, engine, extract

pytestmark = pytest.mark.gpu

REFS = [(str(i + 1), 200000000) for i in range(22)] + [("X", 200000000)]
_STREAM = {}


def _stream(n_pairs, seed=11):
    """(fixture arguments, regions, families, SAM text) of a seeded stream with a twentieth of its pairs inside a region."""
    if (n_pairs, seed) not in _STREAM:
        fx = extract_ref.load("big_random")
        dbl = []
        regions = extract_ref.region_table(fx["locus"], dbl)
        big = [(f, c, l * 1000, r * 1000) for f, c, l, r in regions]
        dbl.append("nofamily")                   # a family without a region: no read, an object of 0 reads
        _STREAM[(n_pairs, seed)] = (fx["args"], big, dbl, extract.synth_stream(n_pairs, big, seed=seed, hit_fraction=0.05, read_len=50))
    return _STREAM[(n_pairs, seed)]


def _fed(a, regions, fams, feeds, bam, keep, paired, fastq):
    ex = extract.Extractor(regions, fams, a["aligner"], paired, a["simulation"], fastq, keep=keep)
    for i, block in enumerate(feeds):
        (ex.feed_bam if bam else ex.feed)(block, last=i == len(feeds) - 1)
    return ex


def _check(a, regions, fams, feeds, bam, paired, fastq, tmp_path=None):
    """Both handles over the same feeds; -> (stats, the statement's records of every family)."""
    kept = _fed(a, regions, fams, feeds, bam, True, paired, fastq)
    plain = _fed(a, regions, fams, feeds, bam, False, paired, fastq)
    try:
        assert kept.stats() == plain.stats()
        with pytest.raises(capi.HgxError):
            kept.take(0, 0)
        all_recs = []
        for f in range(len(fams)):
            texts = [plain.take(f, m) for m in range(2 if paired else 1)]
            want = ref.records(texts, fastq)
            r = kept.take_reads(f)
            try:
                assert (r.route, r.decline, r.n_reads, r.n_inputs) == (2, 0, len(want), len(texts)), fams[f]
                assert r.records() == want, fams[f]
                assert [r.input_text(i) for i in range(len(texts))] == texts
                if tmp_path is not None:
                    paths = [str(tmp_path / ("%s-%d.gz" % (fams[f], m))) for m in range(len(texts))]
                    r.save(paths)
                    assert [gzip.open(p).read() for p in paths] == texts
            finally:
                r.close()
            r = kept.take_reads(f)               # the lists were emptied
            assert (r.n_reads, r.route) == (0, 2)
            r.close()
            all_recs.append(want)
        return kept.stats(), all_recs
    finally:
        kept.close()
        plain.close()


FORMS = {"paired-fastq": (True, True), "single-end": (False, True), "paired-fasta": (True, False)}


@pytest.mark.parametrize("form", list(FORMS))
def test_one_device_chunk(form, tmp_path):
    a, regions, fams, sam = _stream(3000)
    paired, fastq = FORMS[form]
    st, recs = _check(a, regions, fams, [sam], False, paired, fastq, tmp_path)
    assert (st["chunks_device"], st["chunks_host"]) == (1, 0) and sum(st["written"].values()) > 50 and recs[-1] == []
    assert sum(len(r) for r in recs) == sum(st["written"].values()) * (2 if paired else 1)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_device_chunk_then_a_host_chunk(form):
    """3 000 pairs, then 300 more as a second feed: below the extractor's record gate, so that chunk's text is a host segment."""
    a, regions, fams, sam = _stream(3300, seed=12)
    lines = sam.split(b"\n")
    names = [l.split(b"\t", 1)[0] for l in lines]
    cut = names.index(b"read%09d" % 3000)
    first = b"\n".join(lines[:cut]) + b"\n"
    paired, fastq = FORMS[form]
    st, recs = _check(a, regions, fams, [first, sam[len(first):]], False, paired, fastq)
    assert st["chunks_device"] >= 1 and st["chunks_host"] >= 1, st
    assert sum(len(r) for r in recs) == sum(st["written"].values()) * (2 if paired else 1)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_bam_in_three_chunks(form):
    a, regions, fams, sam = _stream(3000)
    data = X.sam_to_bam(sam.decode(), refs=REFS)
    paired, fastq = FORMS[form]
    with engine.test_switches(extract_bam_piece=str(len(data) // 3 + 1), front="device"):      # (a third of the stream is near the record gate)
        st, recs = _check(a, regions, fams, [data], True, paired, fastq)
    assert (st["chunks_device"], st["chunks_host"]) == (3, 0), st
    text_st, text_recs = _check(a, regions, fams, [sam], False, paired, fastq)
    assert recs == text_recs and st["written"] == text_st["written"]


def test_a_record_without_bases():
    """SEQ and QUAL '*' on every 7th record: the text holds "@name\\n*\\n+\\n*\\n" and the table a read of one base."""
    a, regions, fams, sam = _stream(3000)
    out = []
    for k, l in enumerate(sam.split(b"\n")):
        f = l.split(b"\t")
        if k % 7 == 0 and len(f) > 10:
            f[9] = f[10] = b"*"
        out.append(b"\t".join(f))
    st, recs = _check(a, regions, fams, [b"\n".join(out)], False, True, True)
    assert any(s == b"*" and q == b"*" for r in recs for _, s, q in r)


# ---- end to end: a genome-wide stream in, the report out ---------------------------------------------------------------------------
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


def test_stream_to_report_without_a_file_in_between(tmp_path, monkeypatch):
    """The reads of the golden self-test call "pairs_two_genes" as a genome-wide SAM stream: every pair of them inside the hla
    family's regions (a .locus table over two chromosomes), as many pairs of random bases outside.  Route A -- extract_reads_resident
    -> typing_options.reads -> typing() -- against route B -- extract_reads -> the .fq.gz pair -> typing() with align_resident."""
    import align_cases
    typing_mod = importlib.import_module("hisatgenotype_amd.typing")      # (the package's attribute `typing` is the function)
    call = align_cases.selftest_calls("pairs_two_genes", str(tmp_path / "loop"))[-1]
    m1, m2 = call["reads"]
    assert len(m1) == len(m2) > 100
    ix_dir = tmp_path / "genome"
    ix_dir.mkdir()
    (ix_dir / "genotype_genome.locus").write_text("HLA\tA*BACKBONE\t6\t1000000\t2000000\t3000\t+\nHLA\tB*BACKBONE\t7\t5000000\t6000000\t3000\t+\n")
    rng = random.Random(5)
    lines = []
    for k in range(len(m1)):
        chrom, pos = ("6", 1000100 + 3 * k) if k % 2 == 0 else ("7", 5000100 + 3 * k)
        for (_, s, _), flag, p in ((m1[k], 0x43, pos), (m2[k], 0x83, pos + 300)):
            lines.append("frag%06d\t%d\t%s\t%d\t60\t%dM\t=\t%d\t300\t%s\t%s\tNH:i:1\n" % (k, flag, chrom, p, len(s), pos, s, "F" * len(s)))
        for flag, p in ((0x43, 40000000 + 7 * k), (0x83, 40000300 + 7 * k)):
            s = align_cases.rand_seq(rng, 100)
            lines.append("out%06d\t%d\t1\t%d\t60\t100M\t=\t%d\t300\t%s\t%s\tNH:i:1\n" % (k, flag, p, p, s, "5" * 100))
    stream = tmp_path / "genome.sam"
    stream.write_text("".join(lines))
    seen = []
    real_lines = typing_mod.report_lines
    monkeypatch.setattr(typing_mod, "report_lines", lambda res, *r, **k: seen.append(_result_numbers(res)) or real_lines(res, *r, **k))
    monkeypatch.setenv("TMPDIR", str(tmp_path / "tmp"))
    (tmp_path / "tmp").mkdir()
    names = ["sample-hla-extracted-1.fq.gz", "sample-hla-extracted-2.fq.gz"]
    runs = {}
    for route in ("B", "A"):
        work = tmp_path / route
        (work / "out").mkdir(parents=True)
        monkeypatch.chdir(work)
        a = list(call["args"])
        a[0], a[2], a[14], a[19], a[24], a[26], a[27], a[34] = False, ["A", "B"], [["hgx", "graph"]], False, True, "", [], str(work / "out")
        a[25] = [str(work / n) for n in names]
        del seen[:]
        monkeypatch.setattr(typing_mod.typing_options, "align_resident", True)
        with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
            if route == "B":
                got = extract.extract_reads("genotype_genome", str(ix_dir), ["hla"], "", str(work), "fq.gz", ["sample", "sample"], True, True, False,
                                            1, 1, 1, [0, 1], "hisat2", 0, False, alignment_fname=str(stream))
                assert got == {"hla": ["sample-hla"]} and all(os.path.exists(p) for p in a[25])
                typing_mod.typing(*a)
            else:
                reads = extract.extract_reads_resident("genotype_genome", str(ix_dir), ["hla"], str(stream), True, True, False, "hisat2")
                assert list(reads) == ["hla"] and (reads["hla"].route, reads["hla"].n_reads) == (2, 2 * len(m1))
                monkeypatch.setattr(typing_mod.typing_options, "reads", reads["hla"])
                try:
                    typing_mod.typing(*a)
                finally:
                    monkeypatch.setattr(typing_mod.typing_options, "reads", None)
                    reads["hla"].close()
        assert align.align_last()["route"] == 2 and align.align_last()["reads"] == 2 * len(m1)
        assert extract.last_stats["route"] == 2 and extract.last_stats["written"] == {"hla": len(m1)}
        runs[route] = (_report_body(str(work / "out" / "assembly_graph-hla.sample-hla-extracted-1_fq.report")), list(seen))
        assert len(seen) == 2 and all(s[0] > 100 for s in seen)
    assert runs["A"] == runs["B"]
    assert any("ranked" in l or "abundance" in l for l in runs["B"][0])
    left = [p for pat in ("*.fq.gz", "*.bam", "out/*.bam", "out/*.fq.gz") for p in glob.glob(str(tmp_path / "A" / pat))]
    assert left == [] and glob.glob(str(tmp_path / "tmp" / "*")) == []
