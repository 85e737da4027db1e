"""Both fallback tiers in one call on the kernels (csrc/hgx_align.hip: the clip pass, k_aln_tier_keep, the gap pass over the reads the
cost rule leaves to it, k_aln_tier_choose, k_aln_emit<true, true>; route = 2, rescue=(gap, clip)) give the plain-Python statement's
text (tests/align_rescue_ref.py) and the host route's byte for byte: on the host test's inputs and random loci; with no, one, all
clipped, all gapped and mixed reads rescued among 1 .. 65; with the only rescued read first in, last in and alone in the second
chunk; with a chunk whose gap pass is empty and one whose clip pass aligns nothing; over the budgets; at the anchor and variant
limits; with a decline in the gap pass behind a clip pass that aligned reads, and behind a full first chunk; with both counter
triples; under genotyping_locus with the aligner name "hgx.rescue"; and through the device front end."""
import contextlib
import gzip
import io
import json
import os

import pytest

import align_cases
import align_rescue_cases as rc
import align_rescue_ref
import align_ref
from hisatgenotype_amd import align, engine

pytestmark = pytest.mark.gpu

CHUNK = 8192                         # reads per chunk of the device route (csrc/hgx_align.hip)
ZERO = dict(searched=0, clipped=0, bases=0), dict(searched=0, gapped=0, bases=0)


def _run(d, texts, max_edits=2, route="device", **kw):
    ix = align.AlignIndex(*d)
    try:
        with engine.test_switches(front="host") if route == "host" else contextlib.nullcontext():
            out = ix.align(texts, max_edits=max_edits, route="auto" if route == "host" else route, **kw)
        return out, align.align_last()
    finally:
        ix.close()


def _counters(last):
    return (dict(searched=last["clip_searched"], clipped=last["clip_clipped"], bases=last["clip_bases"]),
            dict(searched=last["gap_searched"], gapped=last["gap_gapped"], bases=last["gap_bases"]))


@pytest.mark.parametrize("key", rc.INPUT_IDS + align_cases.INPUT_IDS)
def test_kernels_equal_the_statement_and_the_host_route(key):
    d, texts, me, gap, clip = rc._input(key)
    got, last = _run(d, texts, me, rescue=(gap, clip))
    st = {}
    want = rc.ref_text(key, stats=st)
    assert got == want
    if key in ("glengths", "clengths"):                    # their 1 024-base reads are past the kernels' read length
        assert (last["route"], last["decline"]) == (0, align.DECLINE_READ_LEN), last
    elif not key.startswith("empty"):
        assert (last["route"], last["decline"]) == (2, 0), last
    recs = rc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == (st["clip"], st["gap"])
    host, hlast = _run(d, texts, me, route="host", rescue=(gap, clip))
    assert host == got and _counters(hlast) == _counters(last) and hlast["route"] == 0


def test_random_loci_with_dense_variants():
    for seed, loci, reads, me, gap, clip, want, st in rc.random_cases():
        got, last = _run(align_cases.dicts_of(loci), [rc.fasta(reads)], me, rescue=(gap, clip))
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == (st["clip"], st["gap"]), seed


def _pool():
    """The hand cases' reads on their first locus; per read the statement's line (or None) and its counters, at max_edits 2."""
    loc = rc.locus()
    reads = []
    for _, loci, rs, _, _, _, _, _ in rc.hand_cases()[:4]:
        reads += rs
    plain = reads.pop([n for n, _ in reads].index("e2e"))
    reads = [plain] + reads
    lines, stats = [], []
    for n, s in reads:
        st = {}
        body = rc.records(align_rescue_ref.align_text([loc], [[(n, s, None)]], 2, gap=rc.GAP, clip=rc.CLIP, stats=st).encode())
        lines.append(body[0] if body else None)
        stats.append(st)
    header = "@SQ\tSN:%s\tLN:%d\n" % (loc.name, len(loc.bb))
    clipped = [j for j, l in enumerate(lines) if l is not None and rc.is_clipped(l)]
    gapped = [j for j, l in enumerate(lines) if l is not None and rc.is_gapped(l)]
    return [loc], reads, lines, stats, header, clipped, gapped


_POOL = []


def _pool_once():
    if not _POOL:
        _POOL.append(_pool())
    return _POOL[0]


def _index_of(name):
    return [n for n, _ in _pool_once()[1]].index(name)


def _run_pick(pick):
    loci, reads, lines, stats, header, _, _ = _pool_once()
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    got, last = _run(align_cases.dicts_of(loci), [align_cases.fasta(recs)], 2, rescue=(rc.GAP, rc.CLIP))
    want = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, len(pick)), last
    assert _counters(last) == tuple({c: sum(stats[j][t][c] for j in pick) for c in stats[0][t]} for t in ("clip", "gap"))
    return last


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("mode", ["none", "one", "clipped", "gapped", "mixed"])
def test_few_reads_of_which_none_one_or_all_are_rescued(n, mode):
    _, reads, _, _, _, clipped, gapped = _pool_once()
    assert len(clipped) >= 6 and len(gapped) >= 4
    pick = ([0] * n if mode == "none" else [0] * (n - 1) + [gapped[1]] if mode == "one" else
            [clipped[k % len(clipped)] for k in range(n)] if mode == "clipped" else [gapped[k % len(gapped)] for k in range(n)] if mode == "gapped"
            else [k % len(reads) for k in range(n)])
    last = _run_pick(pick)
    if mode != "mixed":
        assert (last["clip_clipped"], last["gap_gapped"]) == dict(none=(0, 0), one=(0, 1), clipped=(n, 0), gapped=(0, n))[mode]


@pytest.mark.parametrize("n,at", [(CHUNK - 1, 0), (CHUNK, CHUNK - 1), (CHUNK + 1, CHUNK), (CHUNK + 1, CHUNK - 1)])
@pytest.mark.parametrize("which", ["r2", "d20"])
def test_the_only_rescued_read_at_the_chunk_edges(n, at, which):
    """First in, last in its chunk, alone in the second chunk (8 193 reads), and last of the first chunk with a second chunk behind
    it: a clipped read that the gap pass searches too (cost 2), and a gapped one."""
    pick = [0] * n
    pick[at] = _index_of(which)
    last = _run_pick(pick)
    assert (last["clip_searched"], last["gap_searched"]) == (1, 1)
    assert (last["clip_clipped"], last["gap_gapped"]) == ((1, 0) if which == "r2" else (0, 1))


def test_a_chunk_whose_gap_pass_is_empty_and_one_whose_clip_pass_aligns_nothing():
    cheap = [_index_of(n) for n in ("r1", "l1", "r1rc")]               # cost(C) = 1: the gap pass's mark is empty
    last = _run_pick([0, cheap[0], cheap[1], 0, cheap[2]] * 5)
    assert (last["clip_searched"], last["clip_clipped"], last["gap_searched"]) == (15, 15, 0)
    hard = [_index_of(n) for n in ("d40", "none")]                     # the clip tier aligns neither
    last = _run_pick([hard[0], 0, hard[1]] * 7)
    assert (last["clip_searched"], last["clip_clipped"], last["gap_searched"], last["gap_gapped"]) == (14, 0, 14, 7)


@pytest.mark.parametrize("gap", [1, 16])
@pytest.mark.parametrize("clip", [1, 32, 255])
@pytest.mark.parametrize("me", [1, 2, 4])
def test_budgets(gap, clip, me):
    for key in ("rhand1", "rhand2", "rhand4", "mixed-err1"):
        d, texts, _, _, _ = rc.inputs()[key]
        st = {}
        want = rc.ref_text(key, gap=gap, clip=clip, stats=st, max_edits=me)
        got, last = _run(d, texts, me, rescue=(gap, clip))
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == (st["clip"], st["gap"]), key


def _statement(loci, reads, **kw):
    st = {}
    text = align_rescue_ref.align_text(loci, [[(q, s, None) for q, s in reads]], 2, gap=rc.GAP, clip=rc.CLIP, stats=st, **kw).encode()
    return text, st


@pytest.mark.parametrize("kind,n,route,dec", [
    ("anchors", align_cases.DEV_ANCHORS, 2, 0), ("anchors", align_cases.DEV_ANCHORS + 1, 0, align.DECLINE_ANCHORS),
    ("vars", align_cases.DEV_VARS, 2, 0), ("vars", align_cases.DEV_VARS + 1, 0, align.DECLINE_VARS)])
def test_a_rescued_read_at_a_limit_and_past_it(kind, n, route, dec):
    """128 and 129 anchors, 32 and 33 variants of one read (the gap test's reads: each needs the gap tier)."""
    import test_gpu_align_gap as tg
    loci, reads = dict(anchors=tg._anchors_case, vars=tg._vars_case)[kind](n)
    want, st = _statement(loci, reads)
    assert want.count(b"\n") == 2 and st["gap"]["gapped"] == 1
    got, last = _run(align_cases.dicts_of(loci), [align_cases.fasta(reads)], 2, rescue=(rc.GAP, rc.CLIP))
    assert (last["route"], last["decline"]) == (route, dec), (n, last)
    assert got == want and _counters(last) == (st["clip"], st["gap"])


def _gap_pass_case(n_left):
    """A locus and two reads.  `ov` hangs one base over the right end (the clip pass aligns it).  `gp` lacks backbone base 150 and
    carries n_left known singles left of it and 13 right of it; its only whole seed is its last 16 bases.  Through that anchor the
    plain search and the clip pass die a few bases left of the missing base with 13 variants on their lists; the gap pass goes on
    and needs n_left + 13."""
    bb = align_cases._bb(42, 400)
    at = [144 - 2 * j for j in range(n_left)] + [160 + 2 * j for j in range(13)]
    loc = align_ref.Locus("V2*BACKBONE", bb, sorted(("single", p, align_cases._other(bb[p]), "hv%d" % p) for p in at))
    read = list(bb)
    for p in at:
        read[p] = align_cases._other(bb[p])
    read = "".join(read)
    return [loc], [("ov", bb[301:400] + rc._not(bb[399])), ("gp", read[100:150] + read[151:201])]


@pytest.mark.parametrize("n_left,route,dec", [(19, 2, 0), (20, 0, align.DECLINE_VARS)])
def test_a_decline_in_the_gap_pass_behind_a_clip_pass_that_aligned_a_read(n_left, route, dec):
    """33 variants only on the gapped way: the clip pass runs through (and aligns `ov`), the gap pass reaches the variant limit, the
    call's text and counts are taken back and the host route's bytes are returned."""
    loci, reads = _gap_pass_case(n_left)
    want, st = _statement(loci, reads)
    # (the missing base stands in a run of two: the leftmost placement is the record)
    assert [l.split("\t")[5] for l in rc.records(want)] == ["99M1S", "49M1D51M"] and want.count(b"|S|hv") == n_left + 13
    assert (st["clip"]["clipped"], st["gap"]["searched"], st["gap"]["gapped"]) == (1, 1, 1)
    got, last = _run(align_cases.dicts_of(loci), [align_cases.fasta(reads)], 2, rescue=(rc.GAP, rc.CLIP))
    assert (last["route"], last["decline"]) == (route, dec), last
    assert got == want and _counters(last) == (st["clip"], st["gap"]) and last["aligned"] == 2
    # the clip tier alone takes the same reads without a decline: the limit is the gap pass's
    _, clast = _run(align_cases.dicts_of(loci), [align_cases.fasta(reads)], 2, clip=rc.CLIP)
    assert (clast["route"], clast["decline"], clast["clip_clipped"]) == (2, 0, 1)


def test_a_decline_behind_a_full_first_chunk():
    """The read that stops the gap pass in the second chunk, behind a full first chunk of rescued reads: the first chunk's text and
    both counter triples are taken back and the host route writes the whole call."""
    loci, reads, lines, stats, header, _, _ = _pool_once()
    v_loci, v_reads = _gap_pass_case(20)
    all_loci = loci + v_loci
    v_want, v_st = _statement(all_loci, v_reads[1:])
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, v_reads[1])
    body = ["q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) if lines[j] is not None else "" for k, j in enumerate(pick)]
    body.insert(CHUNK + 8, rc.records(v_want)[0] + "\n")
    want = (header + "@SQ\tSN:%s\tLN:%d\n" % (v_loci[0].name, len(v_loci[0].bb)) + "".join(body)).encode()
    got, last = _run(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)], 2, rescue=(rc.GAP, rc.CLIP))
    assert (last["route"], last["decline"]) == (0, align.DECLINE_VARS), last
    assert got == want
    assert _counters(last) == tuple({c: sum(stats[j][t][c] for j in pick) + v_st[t][c] for c in stats[0][t]} for t in ("clip", "gap"))


def test_the_counters_do_not_leak_between_calls():
    """Both triples after a rescue call, one after a single tier's call, none after a default call, in any order on one thread."""
    d, texts, me, gap, clip = rc.inputs()["rhand3"]
    st = {}
    rc.ref_text("rhand3", stats=st)
    assert st["clip"]["clipped"] > 0 and st["gap"]["gapped"] > 0
    both = lambda: _counters(_run(d, texts, me, rescue=(gap, clip))[1])
    assert both() == (st["clip"], st["gap"])
    assert _counters(_run(d, texts, me)[1]) == ZERO
    assert both() == (st["clip"], st["gap"])
    c_only = _counters(_run(d, texts, me, clip=clip)[1])
    assert c_only[0]["clipped"] > 0 and c_only[1] == ZERO[1]
    g_only = _counters(_run(d, texts, me, gap=gap)[1])
    assert g_only[1]["gapped"] > 0 and g_only[0] == ZERO[0]
    assert both() == (st["clip"], st["gap"])


def test_the_device_front_end_equals_the_host_front_end_on_the_rescued_text():
    """The kernels' text of the mixed synth pairs through both front ends: the same batch, and more pairs than from either tier's
    text alone."""
    from hisatgenotype_amd import locus as hl, synth
    from test_gpu_front import same_batch
    d, texts, me, gap, clip = rc.inputs()["mixed-err1"]
    loc = synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11)
    pl = hl.PackedLocus.from_synth(loc)
    text, last = _run(d, texts, me, rescue=(gap, clip))
    assert (last["route"], last["decline"]) == (2, 0) and last["gap_gapped"] > 0 and last["clip_clipped"] > 0
    host = pl.parse_sam(text, num_editdist=2, simulation=False)
    with engine.test_switches(front="device"):
        dev = pl.parse_sam_dev(text, num_editdist=2, simulation=False)
        assert engine.front_last() == (2, 0), engine.front_last()
    same_batch(host, dev.to_host(), len(loc.backbone))
    for kw in (dict(gap=gap), dict(clip=clip)):
        fewer = pl.parse_sam(_run(d, texts, me, **kw)[0], num_editdist=2, simulation=False)
        assert host.n_pairs > fewer.n_pairs > 0


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


def test_selftest_loop_with_the_rescue_name(tmp_path, monkeypatch):
    """genotyping_locus on pairs_two_genes with aligners=[["hgx.rescue", "graph"]]: the kernels run with rescue = (16, 32) and as many
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
        passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx.rescue", "graph"]], [], False, "",
                                      1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                      0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                      False, dict(p["debug"]))
    last = align.align_last()
    assert (last["route"], last["decline"]) == (2, 0), last
    total = [l for l in spec["stderr"].split("\n") if "passed (" in l][-1]
    assert passed == {"hgx.rescue graph": int(total.split("\t")[1].split("/")[0])}
