"""k_aln_pair_pick (csrc/hgx_align.hip; hgx_align_opts.pair = 1, the kernels forced with front=device) gives the bytes of the
plain-Python statement (tests/align_pair_ref.py): on the host test's inputs, at the grid and chunk edges of the pair count, at the
slot-count edges of a mate's candidates (one past them the call declines and the host route gives the same bytes), with a mate
without candidates beside a rescued pair, on single-end input, and under genotyping_locus with the aligner name "hgx.pairs"."""
import contextlib
import gzip
import io
import json
import os

import pytest

import align_cases
import align_pair_cases
import align_pair_ref
import align_ref
from hisatgenotype_amd import align, engine

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


def _counters(last):
    return last["pairs_searched"], last["pairs_placed"], last["pairs_changed"]


@pytest.mark.parametrize("key", align_pair_cases.INPUT_IDS)
def test_device_route_equals_the_pair_statement(key):
    d, texts, me, frag = align_pair_cases.inputs()[key]
    got, last = _device(d, texts, me, max_fragment=frag, pair="aware")
    want = align_pair_cases.ref_text(key)
    assert got == want
    assert (last["route"], last["decline"]) == (2, 0), last
    recs = [l for l in want.decode().split("\n") if l and not l.startswith("@")]
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == align_pair_cases.ref_counters(key)
    # route="device" forces the kernels as the switch does
    ix = align.AlignIndex(*d)
    assert ix.align(texts, max_edits=me, max_fragment=frag, pair=1, route="device") == want and align.align_last()["route"] == 2
    ix.close()


@pytest.mark.parametrize("key", align_pair_cases.PAIRED)
def test_the_independent_suites_paired_inputs(key):
    d, texts, me = align_cases.inputs()[key]
    got, last = _device(d, texts, me, pair="aware")
    assert got == align_pair_cases.ref_text_paired(key)
    if key != "empty-pair":
        assert (last["route"], last["decline"]) == (2, 0), last
    if key.startswith("pairs-"):
        assert got == align_cases.ref_text(key) and _counters(last) == (6, 2, 0)


def test_the_default_is_the_old_behaviour():
    d, texts, me = align_cases.inputs()["pairs-fasta"]
    for kw in ({}, dict(pair=0), dict(pair="independent")):
        got, last = _device(d, texts, me, **kw)
        assert got == align_cases.ref_text("pairs-fasta") and _counters(last) == (0, 0, 0) and last["route"] == 2


_POOL = []


def _pair_pool():
    """The pairs of the hand family (one index: P, Q with one changed base), each with its two statement lines and its counters."""
    if not _POOL:
        d, texts, me, frag = align_pair_cases.inputs()["mixed"]
        loci = align_ref.loci_from_dicts(*d)
        m1, m2 = [align_ref.read_records(t) for t in texts]
        per, cnt = [], []
        for k in range(len(m1)):
            reads = [[("x", m1[k][1], "F" * 100)], [("x", m2[k][1], "5" * 100)]]
            text = align_pair_ref.align_text(loci, reads, me, frag)
            per.append([l for l in text.split("\n") if l and not l.startswith("@")])
            cnt.append(align_pair_ref.counters(loci, reads, me, frag))
        _POOL.append((d, loci, m1, m2, per, cnt))
    return _POOL[0]


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, CHUNK // 2 - 1, CHUNK // 2, CHUNK // 2 + 1])
def test_pair_counts_at_the_grid_and_chunk_edges(n_pairs):
    """A workgroup per pair; mates stay together at the chunk edge; the counters are summed over the chunks."""
    d, loci, m1, m2, per, cnt = _pair_pool()
    pick = [(k * 5 + k // len(m1)) % len(m1) for k in range(n_pairs)]
    f1 = align_cases.fastq([("p%d" % k, m1[j][1], "F" * 100) for k, j in enumerate(pick)])
    f2 = align_cases.fastq([("p%d" % k, m2[j][1], "5" * 100) for k, j in enumerate(pick)])
    got, last = _device(d, [f1, f2], pair="aware")
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)
    want = header + "".join("p%d\t%s\n" % (k, l.split("\t", 1)[1]) for k, j in enumerate(pick) for l in per[j])
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, 2 * n_pairs)
    assert _counters(last) == tuple(sum(cnt[j][c] for j in pick) for c in range(3))
    assert last["pairs_changed"] > 0 or n_pairs == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128])
def test_candidate_counts_at_the_slot_edges(n):
    """Mate 1 with n candidates (the word that stands n times), mate 2 unique behind the last copy, then mate 2 the word itself
    (n x n slots, the triangle of placement pairs); the fragment limit takes every copy in."""
    frag = align_pair_cases.PERIOD * n + 100
    for both in (False, True):
        loci, w, m2 = align_pair_cases.many(n, both=both)
        reads = [[("m", w, None)], [("m", m2, None)]]
        want = align_pair_ref.align_text(loci, reads, 2, frag)
        nh = n * (n + 1) // 2 if both else n
        assert [f[4:] for f in align_pair_cases.fields(want)] == [(nh, "CP"), (nh, "CP")]
        got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta([("m", w)]), align_cases.fasta([("m", m2)])],
                            max_fragment=frag, pair="aware")
        assert (last["route"], last["decline"]) == (2, 0), last
        assert got == want.encode()
        assert _counters(last) == (1, 1, int(n > 1))


def test_one_candidate_more_declines_to_the_host_route():
    n = align_cases.DEV_ANCHORS + 1
    frag = align_pair_cases.PERIOD * n + 100
    loci, w, m2 = align_pair_cases.many(n)
    want = align_pair_ref.align_text(loci, [[("m", w, None)], [("m", m2, None)]], 2, frag).encode()
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta([("m", w)]), align_cases.fasta([("m", m2)])],
                        max_fragment=frag, pair="aware")
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == want and b"NH:i:%d\t" % n in got
    assert _counters(last) == (1, 1, 1)


def test_a_decline_behind_a_full_chunk():
    """A mate past the anchor slots behind a full first chunk: the first chunk's text and counters are taken back, the host route
    writes the whole call with the same rule."""
    d, loci, m1, m2, per, cnt = _pair_pool()
    n = align_cases.DEV_ANCHORS + 1
    rep_loci, w, w2 = align_pair_cases.many(n)
    all_loci = loci + rep_loci
    frag = 1000
    rep = [l for l in align_pair_ref.align_text(all_loci, [[("rep", w, "F" * len(w))], [("rep", w2, "5" * len(w2))]], 2, frag).split("\n")
           if l and not l.startswith("@")]
    n_pairs = CHUNK // 2 + 6
    pick = [k % len(m1) for k in range(n_pairs)]
    r1 = [("q%d" % k, m1[j][1], "F" * 100) for k, j in enumerate(pick)]
    r2 = [("q%d" % k, m2[j][1], "5" * 100) for k, j in enumerate(pick)]
    at = CHUNK // 2 + 3
    r1.insert(at, ("rep", w, "F" * len(w)))
    r2.insert(at, ("rep", w2, "5" * len(w2)))
    # the statement's lines of the pool's pairs do not change when a locus is added behind them (the word is not in P or Q)
    body = ["".join("q%d\t%s\n" % (k, l.split("\t", 1)[1]) for l in per[j]) for k, j in enumerate(pick)]
    body.insert(at, "".join(l + "\n" for l in rep))
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in all_loci)
    got, last = _device(align_cases.dicts_of(all_loci), [align_cases.fastq(r1), align_cases.fastq(r2)], max_fragment=frag, pair="aware")
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == (header + "".join(body)).encode()
    assert _counters(last) == tuple(sum(cnt[j][c] for j in pick) + 1 for c in range(3))


def test_single_end_input_with_the_pair_rule():
    d, texts, me, frag = align_pair_cases.inputs()["mixed-single"]
    got, last = _device(d, texts, me, pair="aware")
    assert got == _device(d, texts, me)[0] == align_pair_cases.ref_text("mixed-single")
    assert _counters(last) == (0, 0, 0) and last["route"] == 2


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


def test_selftest_loop_with_the_pairs_name(tmp_path, monkeypatch):
    """genotyping_locus on pairs_two_genes with aligners=[["hgx.pairs", "graph"]]: the kernels run with the pair rule and as many
    tests pass as in the recorded run."""
    import hisatgenotype_amd as hgx
    spec = CASES["pairs_two_genes"]
    ix_dir, out_dir = tmp_path / "ix", tmp_path / "out"
    ix_dir.mkdir()
    out_dir.mkdir()
    for name, text in spec["index_files"].items():
        (ix_dir / name).write_text(text)
    p = spec["params"]
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stderr(io.StringIO()), engine.test_switches(front="device"):
        passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx.pairs", "graph"]], [], False, "",
                                      1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                      0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                      False, dict(p["debug"]))
    last = align.align_last()
    assert (last["route"], last["decline"]) == (2, 0), last
    assert last["pairs_searched"] > 100 and last["pairs_placed"] > 100
    total = [l for l in spec["stderr"].split("\n") if "passed (" in l][-1]
    assert passed == {"hgx.pairs graph": int(total.split("\t")[1].split("/")[0])}
