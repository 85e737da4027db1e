"""The gap tier's kernels (csrc/hgx_align.hip: k_aln_tier_mark / _fill / _extend<GapTier> / _pick<GapTier>, k_aln_emit<false, true>;
route = 2) give the plain-Python statement's text (tests/align_gap_ref.py) byte for byte: on the host test's inputs and random loci,
with 0, 1 and all reads of a call gapped, with the only gapped read first in, last in and alone in the second chunk, at the anchor,
variant and stack limits of the fixed scratch (past them the host route finishes the call), with gap = 0 (align_ref's bytes,
counters zero: the tier's launches stand behind `gap > 0`), under genotyping_locus with the aligner name "hgx.gap", and through the
device front end."""
import contextlib
import gzip
import io
import json
import os

import pytest

import align_cases
import align_gap_cases as gc
import align_gap_ref
import align_ref
from hisatgenotype_amd import align, engine

pytestmark = pytest.mark.gpu

CHUNK = 8192                         # reads per chunk of the device route (csrc/hgx_align.hip)


def _device(d, texts, max_edits=2, **kw):
    ix = align.AlignIndex(*d)
    try:
        out = ix.align(texts, max_edits=max_edits, route="device", **kw)
        return out, align.align_last()
    finally:
        ix.close()


def _counters(last):
    return dict(searched=last["gap_searched"], gapped=last["gap_gapped"], bases=last["gap_bases"])


def _input(key):
    return gc.inputs()[key] if key in gc.inputs() else align_cases.inputs()[key] + (gc.GAP,)


@pytest.mark.parametrize("key", gc.INPUT_IDS + align_cases.INPUT_IDS)
def test_kernels_equal_the_gap_statement(key):
    d, texts, me, gap = _input(key)
    got, last = _device(d, texts, me, gap=gap)
    st = {}
    want = gc.ref_text(key, stats=st)
    assert got == want
    if key == "glengths":                                  # its 1 024-base read is past the kernels' read length
        assert (last["route"], last["decline"]) == (0, align.DECLINE_READ_LEN), last
    elif not key.startswith("empty"):
        assert (last["route"], last["decline"]) == (2, 0), last
    recs = gc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == st


@pytest.mark.parametrize("key", gc.INPUT_IDS + align_cases.INPUT_IDS)
def test_gap_0_is_the_default(key):
    d, texts, me, _ = _input(key)
    got, last = _device(d, texts, me, gap=0)
    assert got == (align_cases.ref_text(key) if key in align_cases.inputs() else gc.ref_text(key, gap=0))
    assert _counters(last) == dict(searched=0, gapped=0, bases=0)
    assert align.align_last_gap() == (0, 0, 0)


def _pool():
    """All hand-made gap loci in one index; per read of the pool the statement's line (or None) and its counters, at max_edits 2."""
    loci, reads, seen = [], [], set()
    for _, ls, rs, _, _, _ in gc.hand_cases():
        for l in ls:
            if l.name not in seen:
                seen.add(l.name)
                loci.append(l)
        reads += [r for r in rs if r[0] not in ("two", "twor")]      # (their shared part stands in the pool once more: other NH)
    plain = ("plain", loci[1].bb[100:200])                 # aligns end to end
    reads = [plain] + reads
    lines, stats = [], []
    for n, s in reads:
        st = {}
        body = gc.records(align_gap_ref.align_text(loci, [[(n, s, None)]], 2, gap=gc.GAP, stats=st).encode())
        lines.append(body[0] if body else None)
        stats.append(st)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)
    gapped = [j for j, l in enumerate(lines) if l is not None and gc.is_gapped(l)]
    return loci, reads, lines, stats, header, gapped


_POOL = []


def _pool_once():
    if not _POOL:
        _POOL.append(_pool())
    return _POOL[0]


def _run_pick(pick, **kw):
    loci, reads, lines, stats, header, _ = _pool_once()
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(recs)], 2, gap=gc.GAP, **kw)
    want = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, len(pick)), last
    assert _counters(last) == {c: sum(stats[j][c] for j in pick) for c in ("searched", "gapped", "bases")}
    return last


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("mode", ["none", "one", "all"])
def test_few_reads_of_which_none_one_or_all_are_gapped(n, mode):
    gapped = _pool_once()[5]
    assert len(gapped) >= 10
    pick = [0] * n if mode == "none" else [0] * (n - 1) + [gapped[3]] if mode == "one" else [gapped[k % len(gapped)] for k in range(n)]
    last = _run_pick(pick)
    assert last["gap_gapped"] == (0 if mode == "none" else 1 if mode == "one" else n)


@pytest.mark.parametrize("n,at", [(CHUNK - 1, 0), (CHUNK, CHUNK - 1), (CHUNK + 1, CHUNK), (CHUNK + 1, CHUNK - 1)])
def test_the_only_gapped_read_at_the_chunk_edges(n, at):
    """First in, last in its chunk, alone in the second chunk (8 193 reads), and last of the first chunk with a second chunk behind it."""
    pick = [0] * n
    pick[at] = _pool_once()[5][0]
    last = _run_pick(pick)
    assert (last["gap_searched"], last["gap_gapped"]) == (1, 1)


@pytest.mark.parametrize("gap", [1, 2, 16])
@pytest.mark.parametrize("me", [1, 2, 4])
def test_budgets(gap, me):
    for key in ("ghand0", "ghand4", "ghand7", "novel-err1"):
        d, texts, _, _ = gc.inputs()[key]
        st = {}
        want = gc.ref_text(key, gap=gap, stats=st, max_edits=me)
        got, last = _device(d, texts, me, gap=gap)
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == st


def test_random_loci_with_dense_variants():
    """The host test's 60 seeds on the kernels: small alphabets, known indels at and near the gaps, repeats and ties."""
    for seed, loci, reads, me, gap, want, st in gc.random_cases():
        got, last = _device(align_cases.dicts_of(loci), [gc.fasta(reads)], me, gap=gap)
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == st, seed


def _anchors_case(n):
    """A 29-base read whose first 16 bases stand n times in the locus; behind one copy a backbone base is missing.  The copy is the
    first at which the read's other seeds (they span the gap) hit nothing by chance: the read has exactly n anchors."""
    loci, reads = align_cases.limit_case("anchors", n)
    bb, w = loci[0].bb, reads[0][1]
    p = -1
    while True:
        p = bb.index(w, p + 1)
        s = w + bb[p + 17:p + 30]
        hits = sum(len(loci[0].kmers.get(x[o:o + 16], [])) for x in (s, align_ref.revcomp(s)) for o in align_ref.seed_offsets(len(x)))
        if hits == n:
            return loci, [("rep", s)]


def _vars_case(n):
    """A 100-base read with n known singles and a one-base novel deletion behind them."""
    loci, reads = align_cases.limit_case("vars", n)
    return loci, [("va", reads[0][1][:90] + loci[0].bb[191:201])]


def _stack_case(n):
    """A 100-base read that passes n known one-base deletions without taking them (each a pending choice) and has a one-base novel
    deletion behind them."""
    loci, reads = align_cases.limit_case("stack", n)
    return loci, [("st", reads[0][1][:90] + loci[0].bb[191:201])]


@pytest.mark.parametrize("kind,n,route,dec", [
    ("anchors", align_cases.DEV_ANCHORS, 2, 0), ("anchors", align_cases.DEV_ANCHORS + 1, 0, align.DECLINE_ANCHORS),
    ("vars", align_cases.DEV_VARS, 2, 0), ("vars", align_cases.DEV_VARS + 1, 0, align.DECLINE_VARS),
    ("stack", align_cases.DEV_STK - 1, 2, 0), ("stack", align_cases.DEV_STK, 2, 0), ("stack", align_cases.DEV_STK + 1, 0, align.DECLINE_STACK)])
def test_a_gapped_read_at_a_limit_and_past_it(kind, n, route, dec):
    loci, reads = dict(anchors=_anchors_case, vars=_vars_case, stack=_stack_case)[kind](n)
    st = {}
    want = align_gap_ref.align_text(loci, [[(q, s, None) for q, s in reads]], 2, gap=gc.GAP, stats=st).encode()
    assert want.count(b"\n") == 2 and st["gapped"] == 1 and gc.is_gapped(gc.records(want)[0])
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], 2, gap=gc.GAP)
    assert (last["route"], last["decline"]) == (route, dec), (n, last)
    assert got == want and _counters(last) == st
    ix = align.AlignIndex(*align_cases.dicts_of(loci))
    assert ix.align([align_cases.fasta(reads)], max_edits=2, route="host", gap=gc.GAP) == got


def test_a_decline_behind_a_full_first_chunk():
    """A gapped read past the anchor slots behind a full first chunk: the first chunk's text and counters are taken back and the
    host route writes the whole call."""
    loci, reads, lines, stats, header, _ = _pool_once()
    rep_loci, rep_reads = _anchors_case(align_cases.DEV_ANCHORS + 1)
    all_loci = loci + rep_loci
    st = {}
    rep_line = gc.records(align_gap_ref.align_text(all_loci, [[("rep", rep_reads[0][1], None)]], 2, gap=gc.GAP, stats=st).encode())[0]
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, rep_reads[0])
    body = ["q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) if lines[j] is not None else "" for k, j in enumerate(pick)]
    body.insert(CHUNK + 8, rep_line + "\n")
    want = (header + "@SQ\tSN:%s\tLN:%d\n" % (rep_loci[0].name, len(rep_loci[0].bb)) + "".join(body)).encode()
    got, last = _device(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)], 2, gap=gc.GAP)
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == want
    assert _counters(last) == {c: sum(stats[j][c] for j in pick) + st[c] for c in ("searched", "gapped", "bases")}


def test_the_tier_counters_do_not_leak_between_calls():
    """The two tiers share one counter triple in the library: in kernel-route calls that follow each other on one thread, each of
    hgx_align_last_clip and hgx_align_last_gap reports its own tier's call and zeros after the other tier's or a default call."""
    import align_clip_cases as cc
    cst, gst = {}, {}
    cc.ref_text("chand0", stats=cst)
    gc.ref_text("ghand0", stats=gst)
    assert cst["clipped"] > 0 and gst["gapped"] > 0
    want_clip, want_gap = (cst["searched"], cst["clipped"], cst["bases"]), (gst["searched"], gst["gapped"], gst["bases"])

    def six(which):
        d, texts, me, n = cc.inputs()["chand0"] if which != "gap" else gc.inputs()["ghand0"]
        last = _device(d, texts, me, **({} if which == "default" else {which: n}))[1]
        assert (last["route"], last["decline"]) == (2, 0), last
        return ((last["clip_searched"], last["clip_clipped"], last["clip_bases"]), (last["gap_searched"], last["gap_gapped"], last["gap_bases"]))

    assert six("clip") == (want_clip, (0, 0, 0))
    assert six("gap") == ((0, 0, 0), want_gap)
    assert six("clip") == (want_clip, (0, 0, 0))
    assert six("default") == ((0, 0, 0), (0, 0, 0))
    assert six("gap") == ((0, 0, 0), want_gap)
    assert six("default") == ((0, 0, 0), (0, 0, 0))


def test_the_device_front_end_equals_the_host_front_end_on_the_gapped_text():
    """The kernels' gapped text of the synth pairs through both front ends: the same batch, and more pairs than from the gap = 0 text."""
    from hisatgenotype_amd import locus as hl, synth
    from test_gpu_front import same_batch
    d, texts, me, gap = gc.inputs()["novel-err1"]
    loc = synth.make_hla_like_locus(n_alleles=20, n_vars=120, seed=11)
    pl = hl.PackedLocus.from_synth(loc)
    text, last = _device(d, texts, me, gap=gap)
    assert (last["route"], last["decline"]) == (2, 0) and last["gap_gapped"] > 0
    plain, _ = _device(d, texts, me, gap=0)
    host = pl.parse_sam(text, num_editdist=2, simulation=False)
    with engine.test_switches(front="device"):
        dev = pl.parse_sam_dev(text, num_editdist=2, simulation=False)
        assert engine.front_last() == (2, 0), engine.front_last()
    same_batch(host, dev.to_host(), len(loc.backbone))
    fewer = pl.parse_sam(plain, num_editdist=2, simulation=False)
    assert host.n_pairs > fewer.n_pairs > 0


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


def test_selftest_loop_with_the_gap_name(tmp_path, monkeypatch):
    """genotyping_locus on pairs_two_genes with aligners=[["hgx.gap", "graph"]]: the kernels run with gap = 16 and as many tests pass
    as in the recorded run."""
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
        passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx.gap", "graph"]], [], False, "",
                                      1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                      0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                      False, dict(p["debug"]))
    last = align.align_last()
    assert (last["route"], last["decline"]) == (2, 0), last
    total = [l for l in spec["stderr"].split("\n") if "passed (" in l][-1]
    assert passed == {"hgx.gap graph": int(total.split("\t")[1].split("/")[0])}
