"""The default EM path beyond 4 096 classes (table-lookup mat-vecs, csrc/hgx_em.hip) at the reference's DECISION THRESHOLDS.

Its abundances are good to ~1e-11, and a tolerance check cannot see a decision that flips on that noise.  The reference takes hard
decisions on its own last bits: pruning `prob >= max_prob / 10` (common:1338-1346, 1402), the hand-off cut `i >= 10 and p < 0.03`
(core:1742-1743), the report cut `p < 0.01` and `"%.2f%%" % (p * 100)` (core:2097-2121), the order of the combined list
(core:1771-1782) and the order of the drop-in's whole list (common:1405-1410).  Every case below plants classes whose counts put
the reference's value ON such a threshold (isolated alleles: abundance n / N up to rounding), on top of a random background of more
than 4 096 classes.  The C oracle (oracle/hgx_oracle.c, oracle/orc_pipeline.py) is the reference.

Each case first asserts its premise on the oracle's output (the value lies within 1e-12 relative of its threshold); each family
asserts that the reference takes both branches, and that with the exact re-run switched off (em_skip="tie_rerun") at least one of
its cases decides differently from the reference -- the cases are sharp enough to catch the table-lookup values by themselves."""
import ctypes as C
import importlib

import numpy as np
import pytest

import orc_pipeline
import tables
from hisatgenotype_amd import capi, engine, synth, locus as hl
import hisatgenotype_amd as hgx
from test_gpu_emx import _random_problem

ht = importlib.import_module("hisatgenotype_amd.typing")     # the module (the package's `typing` is the entry point)

pytestmark = pytest.mark.gpu

REL = 1e-12          # how close the reference's value must lie to its threshold


def _near(v, thr):
    return abs(v - thr) <= REL * abs(thr)


def _rows(classes, a_pad):
    rows = np.zeros((len(classes), a_pad // 64), np.uint64)
    for c, mem in enumerate(classes):
        for a in mem:
            rows[c, a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    return rows


# ---- single EMs: Classes.em and the drop-in single_abundance against orc.single_abundance ---------------------------------------

@pytest.fixture(scope="module")
def background():
    """4 300 random classes over 800 of 3 000 alleles (a_pad 3 072: the exact re-run is available), small counts."""
    rng = np.random.RandomState(777)
    A = 3000
    a_pad, name_rank, classes, rows, counts, _ = _random_problem(rng, A, 800, 4300, 0.1)
    used = {a for c in classes for a in c}
    free = [a for a in range(A) if a not in used]
    return dict(A=A, a_pad=a_pad, name_rank=name_rank, classes=classes, rows=rows, counts=counts, free=free)


def _single(orc, bg, planted, remove_low):
    """Planted isolated classes ([(allele, count)], first in dict order) + the background: (oracle (alleles, probs, iters),
    product (prob[A], iters, exact) with the re-run on, product (prob[A], iters) with it off)."""
    A, a_pad = bg["A"], bg["a_pad"]
    classes = [[a] for a, _ in planted] + bg["classes"]
    counts = np.concatenate([np.array([n for _, n in planted], np.int64), bg["counts"]])
    rows = np.concatenate([_rows([[a] for a, _ in planted], a_pad), bg["rows"]])
    oa, op, oit = orc.single_abundance(A, classes, counts, remove_low, None)
    cl = engine.Classes.from_host(rows, counts, a_pad)
    try:
        cl.set_allele_rank(bg["name_rank"])
        p, it = cl.em(A, remove_low, None)
        exact = engine.em_last_exact()
        with engine.test_switches(em_skip="tie_rerun"):
            p_off, it_off = cl.em(A, remove_low, None)
    finally:
        cl.close()
    return (oa, op, oit), (p, it, exact), (p_off, it_off)


def _same_single(o, p, it):
    oa, op, oit = o
    exp = np.full(len(p), -1.0)
    exp[oa] = op
    return it == oit and np.array_equal(p >= 0.0, exp >= 0.0) and np.max(np.abs(p - exp)) <= 1e-9


# (X count, Y count) = (10 k, k): early = the EM is still running at iteration 10 (the ratio decides every pruning step from
# there on); final = it converges before (only the final select_alleles prunes)
PRUNE_EARLY = [10**6 + 37 * j for j in range(12)]
PRUNE_FINAL = [10**12 + 37 * j for j in range(12)]


def test_pruning_at_ten_to_one(orc, background):
    """An allele Y at exactly a tenth of the maximum X (isolated classes counted 10 k and k): the reference keeps or drops Y on its
    own rounding of p_Y >= p_X / 10, from iteration 10 on or in the final select_alleles.  Allele set, iteration count ==,
    abundances <= 1e-9."""
    X, Y = background["free"][5], background["free"][900]
    kept = {"early": set(), "final": set()}
    differs = 0
    for kind, ks in (("early", PRUNE_EARLY), ("final", PRUNE_FINAL)):
        for k in ks:
            o, (p, it, _), (p_off, it_off) = _single(orc, background, [(X, 10 * k), (Y, k)], True)
            oa, op, oit = o
            exp = dict(zip(oa.tolist(), op.tolist()))
            # premise: X is the maximum; Y lies on the line -- in the result if kept, and (kept or dropped) in the same EM
            # without pruning, where the ratio of two alleles that only their own classes support is the same n_Y / n_X
            assert exp[X] == max(exp.values())
            assert (oit >= 11) if kind == "early" else (oit <= 10), (kind, oit)
            if Y in exp:
                assert _near(exp[Y], exp[X] / 10.0), (exp[Y], exp[X] / 10.0)
            classes = [[X], [Y]] + background["classes"]
            counts = np.concatenate([np.array([10 * k, k], np.int64), background["counts"]])
            fa, fp, _ = orc.single_abundance(background["A"], classes, counts, False, None)
            full = dict(zip(fa.tolist(), fp.tolist()))
            assert _near(full[Y], full[X] / 10.0), (full[Y], full[X] / 10.0)
            kept[kind].add(Y in exp)
            assert _same_single(o, p, it), (kind, k, p[Y], exp.get(Y), it, oit)
            differs += not _same_single(o, p_off, it_off)
    assert kept["early"] == {True, False} and kept["final"] == {True, False}, kept
    assert differs >= 1, "no case decides differently on the table-lookup values alone: the family has no teeth"


TAIL_DELTAS = [-3, -2, -1, 1, 2, 3]


def test_drop_in_tail_order_beyond_rank_32(orc, background):
    """Two alleles X, Y of different membership < 1e-12 apart at rank 40 (below 0.005): the drop-in returns the WHOLE list, and the
    reference orders it by its own doubles.  Names of the whole list ==."""
    bg = background
    A, name_rank = bg["A"], bg["name_rank"]
    free = bg["free"]
    Z = free[10:50]
    X, Y = free[60], free[61]
    names = ["a%05d" % int(name_rank[a]) for a in range(A)]       # names whose sort order is the name rank
    orders, differs = set(), 0
    for d in TAIL_DELTAS:
        planted = [(z, (5 + i) * 10**12) for i, z in enumerate(Z)] + [(X, 4 * 10**12), (Y, 4 * 10**12 + d)]
        classes = [[a] for a, _ in planted] + bg["classes"]
        counts = np.concatenate([np.array([n for _, n in planted], np.int64), bg["counts"]])
        oa, op, _ = orc.single_abundance(A, classes, counts, False, None)
        ranked = sorted(zip(oa.tolist(), op.tolist()), key=lambda t: -t[1])       # the reference's stable sort
        want = [names[a] for a, _ in ranked]
        exp = dict(zip(oa.tolist(), op.tolist()))
        assert _near(exp[Y], exp[X]) and exp[X] != exp[Y] and exp[X] < 0.005
        assert want.index(names[X]) >= 32 and want.index(names[Y]) >= 32
        orders.add(want.index(names[X]) < want.index(names[Y]))
        cmpt = {}
        for mem, n in zip(classes, counts.tolist()):
            cmpt["-".join(sorted(names[a] for a in mem))] = n
        got = hgx.single_abundance(cmpt, False, {})
        assert [a for a, _ in got] == want, d
        assert max(abs(p - q) for (_, p), (_, q) in zip(got, ranked)) <= 1e-9
        with engine.test_switches(em_skip="tie_rerun"):
            got_off = hgx.single_abundance(cmpt, False, {})
        differs += [a for a, _ in got_off] != want
    assert orders == {True, False}, orders
    assert differs >= 1, "no case decides differently on the table-lookup values alone: the family has no teeth"


# ---- the typing chain: hgx_type_classes on hand-built class tables against orc_pipeline.finish ----------------------------------

@pytest.fixture(scope="module")
def chain():
    """An HLA-like locus of 2 500 alleles; exon-level background: 4 200 random classes over representatives that no case plants;
    gene-level background over alleles outside the planted groups."""
    loc = synth.make_hla_like_locus(n_alleles=2500, n_vars=900, seed=7)
    pl = hl.PackedLocus.from_synth(loc)
    t = tables.oracle_tables(loc)
    assert list(pl.names) == t["names"]
    names, aidx = t["names"], t["aidx"]
    lengths = np.array([loc.allele_length(n) for n in names], np.int32)
    groups = {aidx[r]: [aidx[m] for m in mem] for r, mem in t["rep_groups"].items()}
    reps = sorted(groups)
    g1 = [r for r in reps if len(groups[r]) == 1]
    g2 = [r for r in reps if len(groups[r]) >= 2]
    g2eq = [r for r in reps if len(groups[r]) == 2 and lengths[groups[r][0]] == lengths[groups[r][1]]]
    rng = np.random.RandomState(99)
    pick1 = list(rng.choice(g1, 24, replace=False))
    pick2eq = list(rng.choice(g2eq, 8, replace=False))
    pick2 = list(rng.choice([r for r in g2 if r not in pick2eq], 12, replace=False))
    planted = set(pick1) | set(pick2eq) | set(pick2)
    pool = np.array([r for r in reps if r not in planted])
    _, _, bclasses, _, bcounts, _ = _random_problem(rng, len(pool), 900, 4200, 0.1)
    ebg = [sorted(int(pool[i]) for i in c) for c in bclasses]
    in_groups = {m for r in planted for m in groups[r]}
    others = np.array([a for a in range(len(names)) if a not in in_groups])
    gbg = []
    for _ in range(300):
        mem = rng.choice(others, rng.randint(1, 40), replace=False)
        gbg.append(sorted(int(a) for a in mem))
    return dict(loc=loc, pl=pl, t=t, lengths=lengths, groups=groups, g1=[int(a) for a in pick1], g2eq=[int(a) for a in pick2eq],
                g2=[int(a) for a in pick2], ebg=ebg, ebg_counts=bcounts, gbg=gbg, gbg_counts=rng.randint(1, 300, len(gbg)).astype(np.int64))


def _chain_tables(fx, exon_planted, gene_planted, total):
    """Class tables of one case: planted isolated classes first, then the background; the LAST exon-level planted entry is a filler
    whose count brings the planted total to `total`.  EM #1 prunes the background (its mass is far below a tenth of the maximum), so
    a planted count n ends as an abundance n / total up to rounding."""
    a_pad = fx["pl"].a_pad
    ex = list(exon_planted)
    fill = total - sum(n for _, n in ex[:-1])
    assert fill > 0
    ex[-1] = (ex[-1][0], fill)
    erows = np.concatenate([_rows([[a] for a, _ in ex], a_pad), _rows(fx["ebg"], a_pad)])
    ecnt = np.concatenate([np.array([n for _, n in ex], np.int64), fx["ebg_counts"]])
    grows = np.concatenate([_rows([[a] for a, _ in gene_planted], a_pad), _rows(fx["gbg"], a_pad)])
    gcnt = np.concatenate([np.array([n for _, n in gene_planted], np.int64), fx["gbg_counts"]])
    return erows, ecnt, grows, gcnt


def _product(fx, erows, ecnt, grows, gcnt):
    pl = fx["pl"]
    L = capi.lib()
    ecl = engine.Classes.from_host(erows, ecnt, pl.a_pad)
    gcl = engine.Classes.from_host(grows, gcnt, pl.a_pad)
    try:
        res = ht.LocusResult()
        res.num_reads, res.num_pairs = 2000, 1000
        o = ht.TypeOpts(1, 0, 0, 0, None, None, None, None, None)
        h = C.c_void_p()
        capi.check(L.hgx_type_classes(C.byref(h), pl.h, ecl.h, gcl.h, C.c_int32(res.num_reads), C.c_int32(res.num_pairs),
                                      C.byref(o), None))
        try:
            ht._result_from_handle(h, pl, res, False)
        finally:
            L.hgx_typing_destroy(h)
    finally:
        ecl.close()
        gcl.close()
    return res


def _oracle_result(res, exp, names):
    """`res` with the oracle's gene_prob: the report the reference prints for these class tables."""
    o = ht.LocusResult()
    o.__dict__.update(res.__dict__)
    o.gene_prob = [[names[a], p] for a, p in exp["gene_prob"]]
    return o


def _chain_matches(res, exp, names):
    """Every EM's allele list, order and iteration count ==, abundances <= 1e-9; gene_prob the same; the report text ==."""
    if len(res.em) != len(exp["em"]):
        return False
    for got, (_, it, lst) in zip(res.em, exp["em"]):
        if got["n_iter"] != it or [a for a, _ in got["result"]] != [names[a] for a, _ in lst]:
            return False
        if any(abs(p - q) > 1e-9 for (_, p), (_, q) in zip(got["result"], lst)):
            return False
    if [a for a, _ in res.gene_prob] != [names[a] for a, _ in exp["gene_prob"]]:
        return False
    if any(abs(p - q) > 1e-9 for (_, p), (_, q) in zip(res.gene_prob, exp["gene_prob"])):
        return False
    return ht.report_lines(res)[0] == ht.report_lines(_oracle_result(res, exp, names))[0]


def _run_chain(orc, fx, exon_planted, gene_planted, total):
    """-> (oracle output, product with the exact re-run, product without it)"""
    t = fx["t"]
    erows, ecnt, grows, gcnt = _chain_tables(fx, exon_planted, gene_planted, total)
    A = t["n_alleles"]
    exp = orc_pipeline.finish(orc, t, erows, ecnt, grows, gcnt, np.zeros(A, np.int64), np.full(A, -1, np.int32), True,
                              fx["lengths"], remove_low=True)
    res = _product(fx, erows, ecnt, grows, gcnt)
    with engine.test_switches(em_skip="tie_rerun"):
        res_off = _product(fx, erows, ecnt, grows, gcnt)
    return exp, res, res_off


def _gene_counts(fx, rep, weights, scale):
    """Gene-level isolated classes for the members of `rep`'s group: member k counted weights[k] * length^2 * scale, so that EM #2's
    abundances are proportional to `weights` (single_abundance divides by the length in every step and once more at the end)."""
    mem = fx["groups"][rep]
    return [(m, int(w) * int(fx["lengths"][m]) ** 2 * scale) for m, w in zip(mem, weights)]


def _check_chain(exp, res, names):
    assert _chain_matches(res, exp, names), (
        [(g["n_iter"], g["result"][:14]) for g in res.em], [(it, [(names[a], p) for a, p in lst[:14]]) for _, it, lst in exp["em"]],
        res.gene_prob[:12], [(names[a], p) for a, p in exp["gene_prob"][:12]])


def test_hand_off_cut_at_three_percent(orc, chain):
    """Eleven representatives above 0.03, then P (an exon group of two) at 0.03 exactly: the reference hands P's group to EM #2 or
    leaves P in the exon-level list on its own rounding of `p < 0.03` at rank 11."""
    fx = chain
    names = fx["t"]["names"]
    R = fx["g2"][:5] + fx["g1"][:5]
    P = fx["g2eq"][0]
    F = fx["g1"][5]
    cut = set()
    differs = 0
    for j in range(12):
        N = 10**12 + 100 * j
        ex = [(r, N * (850 - 30 * i) // 10000) for i, r in enumerate(R)] + [(P, 3 * N // 100), (F, 0)]
        gene = []
        for r in fx["g2"][:5] + [P]:
            gene += _gene_counts(fx, r, range(3, 3 + len(fx["groups"][r])), 10**3)
        exp, res, res_off = _run_chain(orc, fx, ex, gene, N)
        e1 = exp["em"][0][2]
        rank = [a for a, _ in e1].index(P)
        pP = dict(e1)[P]
        assert rank >= 10 and all(p > 0.03 for _, p in e1[:rank]) and _near(pP, 0.03), (rank, pP)
        handed = pP >= 0.03
        cut.add(handed)
        assert (fx["groups"][P][1] in dict(exp["gene_prob"])) == handed
        _check_chain(exp, res, names)
        differs += not _chain_matches(res_off, exp, names)
    assert cut == {True, False}, cut
    assert differs >= 1, "no case decides differently on the table-lookup values alone: the family has no teeth"


def _fmt(p):
    return "%.2f%%" % (p * 100.0)


def test_report_cut_and_print_boundaries(orc, chain):
    """gene_prob values on the report's lines, at the report cut 0.01 and at print boundaries (k + 0.5) / 10^4.  Exon-level values
    0.15675 and 0.12345 (groups of one: never handed off); two groups of two at 0.09 and 0.11 go to EM #2, whose values 0.05,
    0.22825, 0.33925 and 0.3825 reach the list as `p * exon_prob_sum` (exon_prob_sum = 0.2): 0.01, 0.04565, 0.06785 and 0.0765.
    The reference prints each, rounded up or down, or cuts the list before 0.01, on its own last bits."""
    fx = chain
    names = fx["t"]["names"]
    E1, E2, F = fx["g1"][6], fx["g1"][7], fx["g1"][8]
    R1, R2 = fx["g2eq"][1], fx["g2eq"][3]
    ma, mb = fx["groups"][R1]
    mc, md = fx["groups"][R2]
    printed, up, differs = set(), set(), 0
    for j in range(12):
        N = 10**12 + 10**5 * j
        ex = [(R1, 9 * N // 100), (R2, 11 * N // 100), (E1, 15675 * N // 100000), (E2, 12345 * N // 100000), (F, 0)]
        gene = _gene_counts(fx, R1, (5000, 22825), 10) + _gene_counts(fx, R2, (33925, 38250), 10)
        exp, res, res_off = _run_chain(orc, fx, ex, gene, N)
        gp = dict(exp["gene_prob"])
        for a, k in ((E1, 1567), (E2, 1234), (mb, 456), (mc, 678)):
            assert _near(gp[a] * 1e4, k + 0.5), (names[a], gp[a])
            up.add((a, _fmt(gp[a]) == "%.2f%%" % ((k + 1) / 100.0)))
        assert _near(gp[ma], 0.01), gp[ma]
        assert [a for a, _ in exp["gene_prob"]].index(ma) < 10
        printed.add(gp[ma] >= 0.01)
        _check_chain(exp, res, names)
        differs += not _chain_matches(res_off, exp, names)
    assert printed == {True, False}, printed
    assert {u for _, u in up} == {True, False}, up
    assert differs >= 1, "no case decides differently on the table-lookup values alone: the family has no teeth"


def test_combined_order_near_tie(orc, chain):
    """An exon-level value E (a group of one: never handed off) 1e-12 from EM #2's value of m1 times exon_prob_sum (0.45 x 0.4):
    the reference's stable sort on its own doubles orders them; the combined list and the report follow."""
    fx = chain
    names = fx["t"]["names"]
    E, F = fx["g1"][10], fx["g1"][11]
    R = fx["g2eq"][2]
    m1, _ = fx["groups"][R]
    orders, differs = set(), 0
    N = 10**14
    for d in (-12, -6, -3, -1, 1, 3, 6, 12):
        ex = [(R, 45 * N // 100), (E, 18 * N // 100 + d), (F, 0)]
        gene = _gene_counts(fx, R, (4, 6), 10**3)
        exp, res, res_off = _run_chain(orc, fx, ex, gene, N)
        gp = dict(exp["gene_prob"])
        assert _near(gp[E], gp[m1]) and gp[E] != gp[m1], (gp[E], gp[m1])
        order = [a for a, _ in exp["gene_prob"]]
        orders.add(order.index(E) < order.index(m1))
        _check_chain(exp, res, names)
        differs += not _chain_matches(res_off, exp, names)
    assert orders == {True, False}, orders
    assert differs >= 1, "no case decides differently on the table-lookup values alone: the family has no teeth"


def test_many_task_reference_mode_takes_the_checked_chain():
    """The many-task call in the reference's order (em_fast=False) with an EM #1 above 4 096 classes: that task's EM #1 runs on the
    one-task table-lookup EM and the rest of its chain through the same checked chain as the one-task call -- task for task the
    one-task result, and the report of the reference's order at every size."""
    loc = synth.make_hla_like_locus(n_alleles=7000, n_vars=2500, seed=101)
    pl = hl.PackedLocus.from_synth(loc)
    batches = [pl.parse_sam(synth.simulate_sam_fast(loc, synth.pick_sample(loc, 60 + s), n, err_rate=0.002, seed=11 + s))
               for s, n in enumerate((150000, 2000))]
    many = engine.ManyBatch(pl, batches)
    got = ht.type_many(pl, many, em_fast=False)
    assert got[0].em[0]["n_classes"] > 4096
    for g, b in zip(got, batches):
        for em_fast in (False, -1):
            res = ht.LocusResult()
            res.num_reads, res.num_pairs = b.n_reads, b.n_pairs
            one = ht._type_batch(pl, b, res, True, em_fast=em_fast)
            if em_fast is False:
                assert [(e["n_iter"], [a for a, _ in e["result"]]) for e in g.em] == \
                    [(e["n_iter"], [a for a, _ in e["result"]]) for e in one.em]
                assert g.gene_prob == one.gene_prob
            assert hgx.report_lines(g) == hgx.report_lines(one)
