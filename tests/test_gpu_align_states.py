"""The second tier of the "hgx" aligner's kernels, the search over STATES (csrc/hgx_align.hip: k_aln_states over
csrc/hgx_align_states.hpp; search="states" / "states_all", front=device), gives the Python statement's text (tests/align_ref.py) byte
for byte: on the reads the per-anchor search declines today (anchor slots, stack, step limit), on every input of the other forms,
with the marked read alone in a second chunk, as one mate of a pair, at the window's limits, and under genotyping_locus with the
aligner name "hgx.states".  The limits that stay (variants, read length) still decline with their codes."""
import contextlib
import gzip
import io
import json
import os
import random
import re

import pytest

import align_cases
import align_ref
from hisatgenotype_amd import align, bamio, engine, simulate

pytestmark = pytest.mark.gpu

CHUNK = 8192                         # reads per chunk of the device route (csrc/hgx_align.hip)


def _device(d, texts, max_edits=2, **kw):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="device"):
            out = ix.align(texts, max_edits=max_edits, **kw)
        return out, align.align_last()
    finally:
        ix.close()


def _plain(reads):
    return [[(q, s, None) for q, s in reads]]


def _body(text):
    return [l for l in text.split("\n") if l and not l.startswith("@")]


def _n_with_anchor(loci, records):
    n = 0
    for _, seq, _ in records:
        seq = seq.upper()
        n += any(s[o:o + align_ref.K] in loc.kmers for s in (seq, align_ref.revcomp(seq)) for o in align_ref.seed_offsets(len(s))
                 for loc in loci)
    return n


def test_the_constants_are_the_header_s():
    with open(os.path.join(os.path.dirname(align.__file__), "csrc", "hgx_align_states.hpp")) as f:
        h = f.read()
    assert int(re.search(r"#define HGX_ALN_STATES_MAX_WINDOW (\d+)", h).group(1)) == align.STATES_MAX_WINDOW
    assert int(re.search(r"#define HGX_ALN_STATES_MARGIN (\d+)", h).group(1)) == align.STATES_MARGIN
    assert int(re.search(r"#define HGX_ALN_DECLINE_WINDOW (\d+)", h).group(1)) == align.DECLINE_WINDOW


def test_past_the_step_limit():
    """13 + 13 known unit indels: the per-anchor search stops at HGX_ALN_DEV_STEPS and today's call goes to the host route; with
    search="states" the read is marked and the call stays on the device."""
    loci, reads = align_cases.tandem_case(13, units=30, singles=4)
    want = align_ref.align_text(loci, _plain(reads), prune=True).encode()
    assert want.count(b"\n") == 2
    d, text = align_cases.dicts_of(loci), [align_cases.fasta(reads)]
    got, last = _device(d, text, search="states")
    assert (last["route"], last["decline"], last["states_reads"], last["states_anchors"]) == (2, 0, 1, 23), last
    assert got == want
    got, last = _device(d, text)
    assert (last["route"], last["decline"], last["states_reads"]) == (0, align.DECLINE_STEPS, 0), last
    assert got == want


def test_past_the_anchor_slots_in_a_plain_repeat():
    loci, reads = align_cases.tandem_case(19)
    want = align_ref.align_text(loci, _plain(reads), prune=True).encode()
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")
    assert (last["route"], last["decline"], last["states_reads"], last["states_anchors"]) == (2, 0, 1, 1388), last
    assert got == want
    rec = _body(want.decode())[0].split("\t")
    assert rec[5] == "250M" and "NH:i:1" in rec


@pytest.mark.parametrize("kind,n", [("anchors", align_cases.DEV_ANCHORS + 1), ("stack", align_cases.DEV_STK + 1)])
def test_one_past_the_limits_that_the_states_form_lifts(kind, n):
    loci, reads = align_cases.limit_case(kind, n)
    want = align_ref.align_text(loci, _plain(reads)).encode()
    assert want.count(b"\n") == 2
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")
    assert (last["route"], last["decline"], last["states_reads"]) == (2, 0, 1), last
    assert got == want
    if kind == "anchors":
        assert last["states_anchors"] == n and b"NH:i:%d\t" % n in got


@pytest.mark.parametrize("kind,n,code", [("vars", align_cases.DEV_VARS + 1, align.DECLINE_VARS),
                                         ("length", align_cases.DEV_MAX_READ + 1, align.DECLINE_READ_LEN)])
def test_one_past_the_limits_that_stay(kind, n, code):
    loci, reads = align_cases.limit_case(kind, n)
    want = align_ref.align_text(loci, _plain(reads)).encode()
    assert want.count(b"\n") == 2
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")
    assert (last["route"], last["decline"]) == (0, code), last
    assert got == want


@pytest.mark.parametrize("key", align_cases.INPUT_IDS)
def test_states_all_equals_the_statement_on_every_input(key):
    d, texts, me = align_cases.inputs()[key]
    got, last = _device(d, texts, me, search="states_all")
    want = align_cases.ref_text(key)
    assert got == want
    if not key.startswith("empty"):
        assert (last["route"], last["decline"]) == (2, 0), last
    loci = align_ref.loci_from_dicts(*d)
    assert last["states_reads"] == sum(_n_with_anchor(loci, align_ref.read_records(t)) for t in texts)
    recs = _body(want.decode())
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2


def test_a_marked_read_alone_in_the_second_chunk():
    """The hand-made reads cycled to CHUNK + 1 reads with the tandem read as read CHUNK: the second tier runs in the second chunk
    only, on chunk-local indices."""
    loci, reads = [], []
    for _, ls, rs, _, _ in align_cases.hand_cases():
        loci += ls
        reads += rs
    t_loci, t_reads = align_cases.tandem_case(13, units=30, singles=4)
    all_loci = loci + t_loci
    lines = []
    for n, s in reads + t_reads:
        body = _body(align_ref.align_text(all_loci, [[(n, s, None)]], 2, prune=True))
        lines.append(body[0] if body else None)
    pick = [k % len(reads) for k in range(CHUNK)] + [len(reads)]
    recs = [("q%d" % k, (reads + t_reads)[j][1]) for k, j in enumerate(pick)]
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in all_loci)
    want = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    assert lines[-1] is not None
    got, last = _device(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)], search="states")
    assert (last["route"], last["decline"], last["reads"], last["states_reads"]) == (2, 0, CHUNK + 1, 1), last
    assert got == want.encode()


def test_a_pair_with_one_hard_mate():
    """Mate 1 is the tandem read (second tier), mate 2 a plain read of the same locus on the other strand (first tier): they meet
    in k_aln_emit, FLAG / YT / RNEXT as the statement writes them."""
    loci, reads = align_cases.tandem_case(13, units=30, singles=4)
    bb = loci[0].bb
    m1 = [(reads[0][0], reads[0][1], None)]
    m2 = [(reads[0][0], align_ref.revcomp(bb[len(bb) - 98:len(bb) - 2]), None)]
    want = align_ref.align_text(loci, [m1, m2], prune=True)
    recs = _body(want)
    assert len(recs) == 2 and all(l.endswith("YT:Z:CP") for l in recs) and [l.split("\t")[1] for l in recs] == ["99", "147"]
    texts = [align_cases.fasta([(q, s) for q, s, _ in m]) for m in (m1, m2)]
    got, last = _device(align_cases.dicts_of(loci), texts, search="states")
    assert (last["route"], last["decline"], last["states_reads"], last["pairs_concordant"]) == (2, 0, 1, 1), last
    assert got == want.encode()


def _spread_case(span, n=align_cases.DEV_ANCHORS + 2):
    """A 16-base read whose bases stand `n` times in the locus, the first and the last copy `span` apart, 200 bases of the locus
    beyond either: the hull of the anchors' diagonals is `span` wide, the window span + 16 + 2 margins."""
    rng = random.Random(71)
    w = align_cases.rand_seq(rng, 16)
    gaps = [span // (n - 1)] * (n - 1)
    gaps[-1] += span - sum(gaps)
    bb = align_cases.rand_seq(rng, 200) + "".join(w + align_cases.rand_seq(rng, g - 16) for g in gaps) + w + align_cases.rand_seq(rng, 200)
    loc = align_ref.Locus("X1*BACKBONE", bb, [])
    assert len(loc.kmers[w]) == n
    return [loc], [("rep", w)], n


@pytest.mark.parametrize("width,route,code", [(align.STATES_MAX_WINDOW - 1, 2, 0), (align.STATES_MAX_WINDOW, 2, 0),
                                              (align.STATES_MAX_WINDOW + 1, 0, align.DECLINE_WINDOW)])
def test_the_widest_window(width, route, code):
    loci, reads, n = _spread_case(width - 16 - 2 * align.STATES_MARGIN)
    want = align_ref.align_text(loci, _plain(reads)).encode()
    assert b"NH:i:%d\t" % n in want
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], search="states")
    assert (last["route"], last["decline"]) == (route, code), last
    assert got == want
    assert (last["states_reads"], last["states_anchors"]) == (1, n)            # (on the host route too: it widens the window)


def test_an_option_that_leaves_the_window():
    """A known 300-base deletion (longer than the margin) that starts inside the windows of both reads: cells with an option the
    tables cannot cost are poisoned, the anchors read them, the kernels decline and the host route answers exactly."""
    bb = align_cases._bb(61, 1200)
    loc = align_ref.Locus("W1*BACKBONE", bb, [("deletion", 400, "300", "hv0")])
    reads = [("del", bb[350:400] + bb[700:750]), ("plain", bb[340:440])]
    want = align_ref.align_text([loc], _plain(reads)).encode()
    assert b"50M300D50M" in want and want.count(b"\n") == 3
    got, last = _device(align_cases.dicts_of([loc]), [align_cases.fasta(reads)], search="states_all")
    assert (last["route"], last["decline"]) == (0, align.DECLINE_WINDOW), last
    assert got == want
    far = [("far", bb[800:900])]                        # the deletion is not in this read's window: nothing to decline
    got, last = _device(align_cases.dicts_of([loc]), [align_cases.fasta(far)], search="states_all")
    assert (last["route"], last["decline"], last["states_reads"]) == (2, 0, 1), last
    assert got == align_ref.align_text([loc], _plain(far)).encode()


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


def test_selftest_loop_with_the_states_name(tmp_path, monkeypatch):
    """genotyping_locus on an error-free golden case with aligners=[["hgx.states", "graph"]] and with [["hgx", "graph"]]: the same
    alignment file and as many tests passed."""
    import hisatgenotype_amd as hgx
    case = "single_test_id_and_list"
    spec = CASES[case]
    p = spec["params"]
    runs = {}
    for name in ("hgx", "hgx.states"):
        work = tmp_path / name.replace(".", "_")
        ix_dir, out_dir = work / "ix", work / "out"
        ix_dir.mkdir(parents=True)
        out_dir.mkdir()
        for fname, text in spec["index_files"].items():
            (ix_dir / fname).write_text(text)
        monkeypatch.chdir(work)
        with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
            passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [[name, "graph"]], [], False, "",
                                          1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                          0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                          False, dict(p["debug"]))
        last = align.align_last()
        assert (last["route"], last["decline"]) == (2, 0), last
        runs[name] = (list(passed.values()), bamio.read_bam(str(work / "hla_output.bam")))
        assert list(passed) == ["%s graph" % name]
    assert runs["hgx"] == runs["hgx.states"] and len(runs["hgx"][1]) > 300
    simulate._store_as_the_reference_does(str(tmp_path / "want.bam"), align_cases.ref_text("%s-1" % case).decode())
    assert runs["hgx.states"][1] == bamio.read_bam(str(tmp_path / "want.bam"))
    with pytest.raises(NotImplementedError):
        simulate.align_reads("hgx.states", True, "ix", "linear", "hla", ["a.fa"], False, 1, str(tmp_path / "o.bam"), 0,
                             truth=({}, {}, {}), var_list={})
