"""The clip tier's kernels (csrc/hgx_align.hip: k_aln_tier_mark / _fill / _extend<ClipTier> / _pick<ClipTier>, k_aln_emit<true>; route = 2) give the
plain-Python statement's text (tests/align_clip_ref.py) byte for byte: on the host test's inputs, with 0, 1 and all reads of a call
clipped, with the only clipped read first in, last in and alone in the second chunk, at the anchor and variant limits of the fixed
scratch (past them the host route finishes the call), with clip = 0 (align_ref's bytes, counters zero: the tier's launches stand
behind `clip > 0`), and under genotyping_locus with the aligner name "hgx.clip"."""
import contextlib
import gzip
import io
import json
import os

import pytest

import align_cases
import align_clip_cases as cc
import align_clip_ref
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
    return dict(searched=last["clip_searched"], clipped=last["clip_clipped"], bases=last["clip_bases"])


def _input(key):
    return cc.inputs()[key] if key in cc.inputs() else align_cases.inputs()[key] + (cc.CLIP,)


@pytest.mark.parametrize("key", cc.INPUT_IDS + align_cases.INPUT_IDS)
def test_kernels_equal_the_clip_statement(key):
    d, texts, me, clip = _input(key)
    got, last = _device(d, texts, me, clip=clip)
    st = {}
    want = cc.ref_text(key, stats=st)
    assert got == want
    if key == "clengths":                                  # its 1 024-base read is past the kernels' read length
        assert (last["route"], last["decline"]) == (0, align.DECLINE_READ_LEN), last
    elif not key.startswith("empty"):
        assert (last["route"], last["decline"]) == (2, 0), last
    recs = cc.records(want)
    assert last["aligned"] == len(recs) and last["pairs_concordant"] == sum(l.endswith("YT:Z:CP") for l in recs) // 2
    assert _counters(last) == st


@pytest.mark.parametrize("key", cc.INPUT_IDS + align_cases.INPUT_IDS)
def test_clip_0_is_the_default(key):
    d, texts, me, _ = _input(key)
    got, last = _device(d, texts, me, clip=0)
    assert got == (align_cases.ref_text(key) if key in align_cases.inputs() else cc.ref_text(key, clip=0))
    assert _counters(last) == dict(searched=0, clipped=0, bases=0)
    assert align.align_last_clip() == (0, 0, 0)


def _pool():
    """All hand-made clip loci in one index; per read of the pool the statement's line (or None) and its counters, at max_edits 0."""
    loci, reads = [], []
    for _, ls, rs, _, _, _ in cc.hand_cases():
        loci += ls
        reads += rs
    plain = ("plain", loci[2].bb[100:200])                 # aligns end to end
    reads = [plain] + reads
    lines, stats = [], []
    for n, s in reads:
        st = {}
        body = cc.records(align_clip_ref.align_text(loci, [[(n, s, None)]], 0, clip=cc.CLIP, stats=st).encode())
        lines.append(body[0] if body else None)
        stats.append(st)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (l.name, len(l.bb)) for l in loci)
    return loci, reads, lines, stats, header


_POOL = []


def _run_pick(pick, **kw):
    if not _POOL:
        _POOL.append(_pool())
    loci, reads, lines, stats, header = _POOL[0]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(recs)], 0, clip=cc.CLIP, **kw)
    want = header + "".join("q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) for k, j in enumerate(pick) if lines[j] is not None)
    assert got == want.encode()
    assert (last["route"], last["decline"], last["reads"]) == (2, 0, len(pick)), last
    assert _counters(last) == {c: sum(stats[j][c] for j in pick) for c in ("searched", "clipped", "bases")}
    return last


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("mode", ["none", "one", "all"])
def test_few_reads_of_which_none_one_or_all_are_clipped(n, mode):
    if not _POOL:
        _POOL.append(_pool())
    n_reads = len(_POOL[0][1])
    pick = [0] * n if mode == "none" else [0] * (n - 1) + [4] if mode == "one" else [1 + k % (n_reads - 1) for k in range(n)]
    last = _run_pick(pick)
    assert (last["clip_clipped"] > 0) == (mode != "none")


@pytest.mark.parametrize("n,at", [(CHUNK - 1, 0), (CHUNK, CHUNK - 1), (CHUNK + 1, CHUNK), (CHUNK + 1, CHUNK - 1)])
def test_the_only_clipped_read_at_the_chunk_edges(n, at):
    """First in, last in its chunk, alone in the second chunk, and last of the first chunk with a second chunk behind it."""
    pick = [0] * n
    pick[at] = 8                                           # "t3": a tail with three mismatches
    last = _run_pick(pick)
    assert (last["clip_searched"], last["clip_clipped"]) == (1, 1)


@pytest.mark.parametrize("clip", [1, 32, 255])
@pytest.mark.parametrize("me", [0, 2, 4])
def test_budgets(clip, me):
    for key in ("chand0", "chand3", "chand4", "overhang-err1"):
        d, texts, _, _ = cc.inputs()[key]
        loci = align_ref.loci_from_dicts(*d)
        st = {}
        want = align_clip_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me, clip=clip, stats=st).encode()
        got, last = _device(d, texts, me, clip=clip)
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == st


def test_random_loci_with_dense_variants():
    """The host test's 60 seeded cases on the kernels: small alphabets, known indels at and near the clip boundaries, ties."""
    for loci, reads, me, clip, want, st in cc.random_cases():
        got, last = _device(align_cases.dicts_of(loci), [cc.fasta(reads)], me, clip=clip)
        assert got == want and (last["route"], last["decline"]) == (2, 0) and _counters(last) == st


def _anchors_case(n):
    """A 21-base read whose first 16 bases stand n times in the locus and whose tail fits none of them."""
    loci, reads = align_cases.limit_case("anchors", n)
    return loci, [("rep", reads[0][1] + "ACGTA")]


def _vars_case(n):
    """A 100-base read with n known singles and a 10-base tail that does not match."""
    loci, reads = align_cases.limit_case("vars", n)
    bb = loci[0].bb
    return loci, [("va", reads[0][1] + cc._not(bb[200]) + cc._junk(9, 9))]


@pytest.mark.parametrize("kind,limit,code", [("anchors", align_cases.DEV_ANCHORS, align.DECLINE_ANCHORS),
                                             ("vars", align_cases.DEV_VARS, align.DECLINE_VARS)])
def test_a_clipped_read_at_a_limit_and_past_it(kind, limit, code):
    for n, route, dec in ((limit, 2, 0), (limit + 1, 0, code)):
        loci, reads = (_anchors_case if kind == "anchors" else _vars_case)(n)
        st = {}
        want = align_clip_ref.align_text(loci, [[(q, s, None) for q, s in reads]], 0, clip=cc.CLIP, stats=st).encode()
        assert want.count(b"\n") == 2 and st["clipped"] == 1
        got, last = _device(align_cases.dicts_of(loci), [align_cases.fasta(reads)], 0, clip=cc.CLIP)
        assert (last["route"], last["decline"]) == (route, dec), (n, last)
        assert got == want and _counters(last) == st
        ix = align.AlignIndex(*align_cases.dicts_of(loci))
        assert ix.align([align_cases.fasta(reads)], max_edits=0, route="host", clip=cc.CLIP) == got


def test_a_decline_behind_a_full_first_chunk():
    """A clipped read past the anchor slots behind a full first chunk: the first chunk's text and counters are taken back and the
    host route writes the whole call."""
    if not _POOL:
        _POOL.append(_pool())
    loci, reads, lines, stats, header = _POOL[0]
    rep_loci, rep_reads = _anchors_case(align_cases.DEV_ANCHORS + 1)
    all_loci = loci + rep_loci
    st = {}
    rep_line = cc.records(align_clip_ref.align_text(all_loci, [[("rep", rep_reads[0][1], None)]], 0, clip=cc.CLIP, stats=st).encode())[0]
    pick = [k % len(reads) for k in range(CHUNK + 20)]
    recs = [("q%d" % k, reads[j][1]) for k, j in enumerate(pick)]
    recs.insert(CHUNK + 8, rep_reads[0])
    body = ["q%d\t%s\n" % (k, lines[j].split("\t", 1)[1]) if lines[j] is not None else "" for k, j in enumerate(pick)]
    body.insert(CHUNK + 8, rep_line + "\n")
    want = (header + "@SQ\tSN:%s\tLN:%d\n" % (rep_loci[0].name, len(rep_loci[0].bb)) + "".join(body)).encode()
    got, last = _device(align_cases.dicts_of(all_loci), [align_cases.fasta(recs)], 0, clip=cc.CLIP)
    assert (last["route"], last["decline"]) == (0, align.DECLINE_ANCHORS), last
    assert got == want
    assert _counters(last) == {c: sum(stats[j][c] for j in pick) + st[c] for c in ("searched", "clipped", "bases")}


with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selftest_loop.json.gz"), "rb") as f:
    CASES = json.loads(f.read().decode())


def test_selftest_loop_with_the_clip_name(tmp_path, monkeypatch):
    """genotyping_locus on pairs_two_genes with aligners=[["hgx.clip", "graph"]]: the kernels run with clip = 32 and as many tests
    pass as in the recorded run."""
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
        passed = hgx.genotyping_locus("hla", list(spec["gene_order"]), "", str(ix_dir), [], True, [["hgx.clip", "graph"]], [], False, "",
                                      1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                      0.0, [], False, "assembly_graph", True, True, False, False, True, [], 0, False, str(out_dir),
                                      False, dict(p["debug"]))
    last = align.align_last()
    assert (last["route"], last["decline"]) == (2, 0), last
    total = [l for l in spec["stderr"].split("\n") if "passed (" in l][-1]
    assert passed == {"hgx.clip graph": int(total.split("\t")[1].split("/")[0])}
