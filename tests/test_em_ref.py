"""tests/em_ref.py pinned to the C oracle (and, on the smallest cases, to oracle/pyref.py), and the PREMISES of every case of
tests/test_gpu_em_edges.py checked on the CPU: the reference's decisions lie at least 1e-7 from their thresholds (100 x the
table-lookup EM's documented 1e-9, so its values alone must take them), the element on either side of every size edge carries
weight, and the reference's iteration counts cover the host's batching.  The cases and their seeds are tests/em_edge_cases.py;
nothing is skipped or filtered here."""
import numpy as np
import pytest

import em_edge_cases as ec
import em_ref
import pyref

MARGIN = 1e-7          # 100 x the documented bound of the table-lookup path (README)
WEIGHT = 1e-6          # what the removal of an edge element must move some surviving abundance by

IDS = [c.id for c in ec.CASES]


def oracle_run(orc, c):
    b = ec.build(c)
    return orc.single_abundance_flat(c.n_alleles, b.off, b.idx, b.counts, c.remove_low, b.lengths)


def sensitivity(c):
    """{("allele", j) | ("class", i): the largest change of a surviving abundance when that element is taken out}"""
    b = ec.build(c)
    pr, base = ec.reference(c)
    want = base.dense(c.n_alleles)
    out = {}
    for kind, els in (("allele", ec.edge_alleles(c)), ("class", ec.edge_classes(c))):
        for e in els:
            if kind == "allele" and c.n == 1:
                continue                                        # (the only allele: nothing is left without it)
            sub = pr.without(alleles=[b.actives[e]]) if kind == "allele" else pr.without(classes=[e])
            try:
                got = sub.run(c.remove_low, b.lengths).dense(c.n_alleles)
            except KeyError:
                out[(kind, e)] = 1.0                            # (the run does not even end the same way)
                continue
            keep = want >= 0.0
            if kind == "allele":
                keep[b.actives[e]] = False
            out[(kind, e)] = float(np.abs(np.where(got[keep] >= 0.0, got[keep], 0.0) - want[keep]).max()) if keep.any() else 0.0
    return out


def expectation_failures(c):
    """the case's `expect` entries that the reference's run does not meet"""
    _, r = ec.reference(c)
    bad = []
    first = None if r.after_first_prune is None else len(r.after_first_prune)
    for k, v in c.expect:
        if k == "n_iter":
            ok = r.n_iter == v
        elif k == "min_iter":
            ok = r.n_iter >= v
        elif k == "max_iter":
            ok = r.n_iter <= v
        elif k == "first_prune":
            ok = first == v
        elif k == "min_first_prune":
            ok = first is not None and first >= v
        elif k == "max_first_prune":
            ok = first is not None and first <= v
        elif k == "masks":
            ok = first is not None and ec.survivor_masks(c, r.after_first_prune) == v
        elif k == "max_masks":
            ok = first is not None and ec.survivor_masks(c, r.after_first_prune) <= v
        elif k == "pruned":
            ok = (len(r.alleles) < c.n) == v
        elif k == "lone":
            ok = (len(r.alleles) == 1) == v
        else:
            raise KeyError(k)
        if not ok:
            bad.append((k, v, r.n_iter, first))
    return bad


@pytest.mark.parametrize("c", ec.CASES, ids=IDS)
def test_em_ref_agrees_with_the_oracle(orc, c):
    """Same survivors, same iteration count, abundances within 1e-12 (the summation order differs); first classes as the
    definition says; a KeyError of the oracle is a KeyError here."""
    b = ec.build(c)
    try:
        oa, op, oit = oracle_run(orc, c)
    except KeyError:
        with pytest.raises(KeyError):
            ec.reference(c)
        return
    _, r = ec.reference(c)
    exp = np.full(c.n_alleles, -1.0)
    exp[oa] = op
    got = r.dense(c.n_alleles)
    assert r.n_iter == oit
    assert np.array_equal(got >= 0.0, exp >= 0.0)
    assert np.max(np.abs(got - exp)) <= 1e-12
    cls = np.repeat(np.arange(c.C), np.diff(b.off))
    for a, f in zip(r.alleles.tolist(), r.first_class.tolist()):
        assert f == cls[b.idx == a].min()


@pytest.mark.parametrize("c", [c for c in ec.CASES if c.pyref], ids=[c.id for c in ec.CASES if c.pyref])
def test_em_ref_agrees_with_pyref(c):
    """The smallest cases through the dict-of-strings statement (oracle/pyref.py:single_abundance)."""
    b = ec.build(c)
    name = lambda a: "a%05d" % a
    cmpt = {}
    for i in range(c.C):
        cmpt["-".join(name(a) for a in b.idx[b.off[i]:b.off[i + 1]].tolist())] = int(b.counts[i])
    assert len(cmpt) == c.C
    lens = None if b.lengths is None else {name(a): int(b.lengths[a]) for a in b.actives.tolist()}
    stats = {}
    exp = dict(pyref.single_abundance(cmpt, c.remove_low, lens, stats))
    _, r = ec.reference(c)
    assert stats["n_iter"] == r.n_iter
    assert sorted(exp) == [name(a) for a in r.alleles.tolist()]
    assert max(abs(exp[name(a)] - p) for a, p in zip(r.alleles.tolist(), r.prob.tolist())) <= 1e-12


@pytest.mark.parametrize("c", ec.CASES, ids=IDS)
def test_margins(c):
    """No pruning comparison and no stopping test of the reference's run within 1e-7 of its threshold."""
    _, r = ec.reference(c)
    assert r.prune_margin >= MARGIN, r.prune_margin
    assert r.stop_margin >= MARGIN, r.stop_margin


@pytest.mark.parametrize("c", ec.CASES, ids=IDS)
def test_edges_carry_weight(c):
    """Taking out the last element before a size edge, or the first after it, moves some surviving abundance by 1e-6 or more."""
    if dict(c.expect).get("lone"):               # one survivor at 1.0 whatever the input holds (test_case_premises asserts it is one)
        _, r = ec.reference(c)
        assert r.prob.tolist() == [1.0]
        return
    s = sensitivity(c)
    assert s
    weak = {k: v for k, v in s.items() if v < WEIGHT}
    assert not weak, weak


@pytest.mark.parametrize("c", ec.CASES, ids=IDS)
def test_case_premises(c):
    """What the case's family needs of the reference's run (iteration count, alleles left by the first pruning, distinct class
    masks over them)."""
    assert not expectation_failures(c)


def test_iteration_counts_cover_the_batching():
    """4 = the last iteration of the host's first batch, 5 = the first of the second, 11 = the first pruning iteration is the last
    one, 12 = one after it, and one long run; one case converges within 10 iterations so that only the final pruning acts."""
    its = {c.id: ec.reference(c)[1].n_iter for c in ec.CASES if c.family == "batching"}
    assert {4, 5, 11, 12} <= set(its.values()), its
    assert max(its.values()) >= 20, its
    final_only = [c for c in ec.CASES if c.remove_low and ec.reference(c)[1].n_iter <= 10 and len(ec.reference(c)[1].alleles) < c.n]
    assert final_only


def test_every_edge_is_in_the_table():
    """The values the families name are in the case list."""
    by = {}
    for c in ec.CASES:
        by.setdefault(c.family, []).append(c)
    assert [c.n for c in by["compact_length"]] == [1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025]
    assert {c.layout for c in by["layout"]} == {"one_word", "gap_word", "last_bit", "ragged"}
    assert [c.a_pad // 64 for c in by["row_width"]] == [8, 128, 136, 520]
    assert [c.C for c in by["classes"]] == [65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385]
    assert {(c.n, c.remove_low, c.lengths) for c in by["long_vectors"]} >= {(n, low, not low) for n in (8191, 8192, 8193) for low in (True, False)}
    assert all(c.a_pad == 8704 and c.C == 4097 for c in by["long_vectors"])
    assert all(c.n == 2049 for c in by["empty_chunk"]) and len(by["empty_chunk"]) == 3
    assert {c.remove_low for c in by["lengths"]} == {True, False} and all(c.lengths for c in by["lengths"])
    assert len({c.id for c in ec.CASES}) == len(ec.CASES)
    for c in ec.CASES:
        if c.C > 4096:
            assert 2 <= c.mem[0] and c.mem[1] <= 12
            assert np.diff(ec.build(c).off).max() <= 12


def test_without_takes_the_element_out():
    """`without` on a hand-made problem: {0, 1} x 3, {1, 2} x 1, {2} x 2."""
    pr = em_ref.Problem([0, 1, 1, 2, 2], [0, 2, 4, 5], [3, 1, 2])
    a = pr.without(alleles=[1])
    assert a.idx.tolist() == [0, 2, 2] and a.off.tolist() == [0, 1, 2, 3] and a.counts.tolist() == [3, 1, 2]
    b = pr.without(classes=[1])
    assert b.idx.tolist() == [0, 1, 2] and b.off.tolist() == [0, 2, 3] and b.counts.tolist() == [3, 2]
    r = a.run()
    assert r.alleles.tolist() == [0, 2] and np.allclose(r.prob, [0.5, 0.5]) and r.n_iter == 1


def test_margins_see_a_decision_on_its_threshold():
    """Isolated alleles counted 10 k and k: the pruning comparison p_Y >= p_X / 10 sits on its threshold and the margin says so."""
    r = em_ref.em_ref([0, 1, 2], [0, 1, 2, 3], [10000, 1000, 50], remove_low=True)
    assert r.prune_margin < 1e-15 and r.n_iter == 1
    r = em_ref.em_ref([0, 1, 2], [0, 1, 2, 3], [10000, 1200, 50], remove_low=True)
    assert abs(r.prune_margin - 200 / 11250) < 1e-12 and r.alleles.tolist() == [0, 1]
