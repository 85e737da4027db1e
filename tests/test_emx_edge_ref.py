"""The PREMISES of every case of tests/test_gpu_emx_edges.py (tests/emx_edge_cases.py), checked on the CPU: tests/em_ref.py agrees
with the C oracle on it (1e-12, same survivors and iteration count, KeyError where the oracle raises), the cases that also run with
table lookups keep every decision 1e-7 from its threshold and carry weight on both sides of their edges, the family premises hold
(alleles left by the first pruning and the iterations after it, the trajectories of the deep-decay cases, the shapes of the
handed-back cases against the gates they name), and `==` is sharper than a tolerance on these inputs: em_ref, which sums in numpy's
order, differs from the oracle in some bit.  Nothing is skipped or filtered here.

One departure from the issue's premises: `prune1`, which also runs with table lookups, ends with ONE survivor at exactly 1.0 whatever
the input holds, so taking an edge element out cannot move a surviving abundance; the WEIGHT premise is replaced there by the
assertion that the result is that lone 1.0 (as tests/test_em_ref.py does for its `lone` cases)."""
import numpy as np
import pytest

import em_edge_cases as ec
import emx_edge_cases as xc
from test_em_ref import MARGIN, WEIGHT, sensitivity

IDS = [x.id for x in xc.CASES]
CHECKED = [x for x in xc.CASES if (x.lookup or x.family == "handed_back") and x.family != "keyerror"]      # decided by table-lookup values somewhere

GATE = 2.0 ** -600          # cols_share's lane_fast
BELOW, ABOVE = 2.0 ** -620, 2.0 ** -580
# the gates of hgx_emx_run / k_emx (hgx_emx.hpp: HGX_EMX_MAX_CLASSES, HGX_EMX_HARD_MAX_CLASSES, HGX_EMX_MAX_ALLELES; w64 <= 128)
MAX_CLASSES, HARD_MAX_CLASSES, MAX_W64 = 4096, 32768, 128


def oracle_run(orc, x):
    b = xc.xbuild(x)
    return orc.single_abundance_flat(b.n_alleles, b.off, b.kidx, b.counts, x.base.remove_low, b.lengths)


def oracle_dense(orc, x):
    oa, op, oit = oracle_run(orc, x)
    exp = np.full(x.base.n_alleles, -1.0)
    exp[oa] = op
    return exp, oit


def agreement_failures(orc, x):
    try:
        exp, oit = oracle_dense(orc, x)
    except KeyError:
        try:
            xc.reference(x)
        except KeyError:
            return []
        return ["the oracle raises KeyError, em_ref does not"]
    _, r = xc.reference(x)
    got = r.dense(x.base.n_alleles)
    bad = []
    if r.n_iter != oit:
        bad.append(("n_iter", r.n_iter, oit))
    if not np.array_equal(got >= 0.0, exp >= 0.0):
        bad.append("survivors")
    elif np.max(np.abs(got - exp)) > 1e-12:
        bad.append(("difference", float(np.max(np.abs(got - exp)))))
    return bad


def near_tie_gap(x):
    """smallest relative difference between two survivors' abundances (the library re-runs a table-lookup EM in the reference's
    order when two alleles of different membership are closer than 1e-8, and then reports `exact`)"""
    _, r = xc.reference(x)
    p = np.sort(r.prob)
    return float(np.min(np.diff(p) / p[1:])) if len(p) > 1 else np.inf


def premise_failures(x):
    """the case's family premises that the reference's run does not meet"""
    c, bad = x.base, []
    e = dict(x.expect)
    if x.family == "keyerror":
        try:
            xc.reference(x)
            bad.append("no KeyError")
        except KeyError:
            pass
        return bad
    if "decay" in e:
        b = xc.xbuild(x)
        seen, r = xc.trajectory(x, b.X)
        order = xc.dict_order(x).tolist()
        if len(order) <= 64:
            bad.append("64 alleles or fewer")
        tiles = {order.index(a) // 64 for a in b.Xs}
        strong = [order.index(int(a)) // 64 for a in ec.build(c).actives[ec.build(c).strong]]
        if tiles & set(strong):
            bad.append(("X shares a tile with a strong allele", sorted(tiles), strong))
        if e["decay"] == "band":
            # (application, allele) operands just above the denormal range; every decaying allele stays in the dict
            allv, ids, _ = xc.record(x)
            v = allv[:, np.searchsorted(ids, b.Xs)]
            n_band = int(((v >= 2.0 ** -1045) & (v < 2.0 ** -1022)).sum())
            if np.isnan(v).any() or n_band < 60:
                bad.append(("operands in [2^-1045, 2^-1022)", n_band))
            return bad
        if b.X not in r.alleles.tolist():
            bad.append("X is not in the result")
        if any(v is None for v in seen):
            bad.append("X leaves the dict")
        vals = [v for v in seen if v is not None]
        if e["decay"] == "gate":
            low = [i for i, v in enumerate(vals) if 0.0 < v < BELOW]
            if len(low) < 3:
                bad.append(("applications below 2^-620", len(low)))
            elif not all(v > ABOVE for v in vals[:low[0]]) or low[0] < 3:
                bad.append("no applications above 2^-580 before the gate")
            if any(BELOW <= v <= ABOVE for v in vals):
                bad.append("an application inside [2^-620, 2^-580]")
        elif e["decay"] == "zero":
            # some dict member: positive going into an iteration, exactly 0.0 in the input of its THIRD application (the extrapolated
            # estimate, max(0.0, x)), in the dict to the end and +0.0 in the result
            allv, ids, _ = xc.record(x)
            hit = []
            for it in range(r.n_iter):
                z = np.nonzero((allv[3 * it] > ABOVE) & (allv[3 * it + 1] > ABOVE) & (allv[3 * it + 2] == 0.0))[0]
                hit += [int(ids[j]) for j in z if not np.isnan(allv[:, j]).any()]
            res = dict(zip(r.alleles.tolist(), r.prob.tolist()))
            hit = [a for a in hit if a in res and res[a] == 0.0 and not np.signbit(res[a])]
            if not r.clamped or not hit:
                bad.append("no member clamped to +0.0 that stays in the result")
            if not any(0.0 < v < GATE for v in vals):
                bad.append("no tile takes the plain `/` in this run")
        elif e["decay"] == "denormal":
            tiny = [i for i, v in enumerate(vals) if 0.0 < v < 2.0 ** -1022]
            if not tiny:
                bad.append(("never denormal: smallest positive value", min(v for v in vals if v > 0.0)))
            elif not all(v == 0.0 for v in vals[tiny[-1] + 1:]) or vals[-1] != 0.0:
                bad.append("does not end at 0.0")
            if float(r.prob[r.alleles.tolist().index(b.X)]) != 0.0:
                bad.append("X's abundance is not 0.0")
        return bad
    _, r = xc.reference(x)
    first = None if r.after_first_prune is None else len(r.after_first_prune)
    if "first_prune" in e and first != e["first_prune"]:
        bad.append(("first_prune", first))
    if "after_prune" in e and r.n_iter < ec.em_ref.PRUNE_FROM + 1 + e["after_prune"]:
        bad.append(("n_iter", r.n_iter))
    if x.family == "sum_groups" and (c.remove_low or len(r.alleles) != c.n):
        bad.append(("npos", len(r.alleles)))
    if x.family == "handed_back":
        C, w64 = c.C, c.a_pad // 64
        over = [w64 > MAX_W64, x.em_fast == 0 and C > MAX_CLASSES, x.em_fast < 0 and C > HARD_MAX_CLASSES]
        if sum(over) != 1:
            bad.append(("gates exceeded", over))
        if near_tie_gap(x) < 1e-6:
            bad.append(("near tie", near_tie_gap(x)))
    if x.family == "any_size" and not (x.em_fast < 0 and MAX_CLASSES < c.C <= HARD_MAX_CLASSES and c.a_pad // 64 <= MAX_W64):
        bad.append("not an any-size problem")
    if x.family not in ("handed_back",) and not (c.a_pad // 64 <= MAX_W64 and c.C <= (HARD_MAX_CLASSES if x.em_fast < 0 else MAX_CLASSES)):
        bad.append("beyond the kernel's gates")
    return bad


def margin_failures(x):
    _, r = xc.reference(x)
    return [(k, v) for k, v in (("prune", r.prune_margin), ("stop", r.stop_margin)) if v < MARGIN]


def weight_failures(x):
    if len(xc.reference(x)[1].alleles) == 1:         # one survivor at 1.0 whatever the input holds: nothing to move
        return [] if xc.reference(x)[1].prob.tolist() == [1.0] else ["lone"]
    s = sensitivity(x.base)
    return sorted((k, v) for k, v in s.items() if v < WEIGHT) if s else ["no edge element"]


@pytest.mark.parametrize("x", xc.CASES, ids=IDS)
def test_em_ref_agrees_with_the_oracle(orc, x):
    """The oracle gets the members of every class in key order (ascending rank); same survivors, same iteration count, abundances
    within 1e-12; a KeyError of the oracle is a KeyError of em_ref."""
    assert not agreement_failures(orc, x)


@pytest.mark.parametrize("x", CHECKED, ids=[x.id for x in CHECKED])
def test_margins(x):
    """No pruning comparison and no stopping test of the reference's run within 1e-7 of its threshold."""
    assert not margin_failures(x)


@pytest.mark.parametrize("x", CHECKED, ids=[x.id for x in CHECKED])
def test_edges_carry_weight(x):
    """Taking out the last element before a size edge, or the first after it, moves some surviving abundance by 1e-6 or more."""
    assert not x.extra                               # (sensitivity works on the base problem)
    assert not weight_failures(x)


@pytest.mark.parametrize("x", xc.CASES, ids=IDS)
def test_case_premises(x):
    assert not premise_failures(x)


def test_rank_kinds():
    """Every rank is a permutation; sparse_words leaves empty 64-rank words between full ones and uses ranks 0 and n_alleles - 1."""
    kinds = set()
    for x in xc.CASES:
        b = xc.xbuild(x)
        kinds.add(x.rank)
        assert np.array_equal(np.sort(b.rank), np.arange(b.n_alleles))
        cls = np.repeat(np.arange(len(b.counts)), np.diff(b.off))
        assert np.array_equal(np.sort(b.kidx), np.sort(b.idx))
        key = cls * (1 << 20) + b.rank[b.kidx]
        assert (np.diff(key) > 0).all()              # classes in order, members ascending by rank inside each
        if x.rank == "sparse_words":
            r = np.sort(b.rank[b.actives])
            words = np.bincount(r >> 6, minlength=(b.n_alleles + 63) // 64)
            full = np.nonzero(words == 64)[0]
            assert r[0] == 0 and r[-1] == b.n_alleles - 1
            assert len(full) == 0 or (words[full[0]:full[-1]:2] == 64).all() and (words[full[0] + 1:full[-1]:2] == 0).all()
            assert len(full) >= 1 or len(r) < 66
    assert kinds == set(xc.RANKS)


def test_every_edge_is_in_the_table():
    by = {}
    for x in xc.CASES:
        by.setdefault(x.family, []).append(x)
    assert [x.base.n for x in by["sum_groups"]] == [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33]
    assert [dict(x.expect)["first_prune"] for x in by["sum_after_prune"]] == [1, 8, 9, 16, 17, 64, 65]
    assert [x.base.n for x in by["allele_tiles"]] == [63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8191, 8192]
    assert [x.base.C for x in by["class_tiles"]] == [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096]
    assert [x.base.C for x in by["any_size"]] == [4097, 8191, 8192, 8193, 32767, 32768] and all(x.em_fast == -1 for x in by["any_size"])
    assert [x.base.a_pad // 64 for x in by["row_width"]] == [8, 56, 64, 72, 120, 128]
    lay = collections_count((x.base.layout for x in by["layout"]))
    assert lay == {"one_word": 2, "gap_word": 2, "last_bit": 2, "ragged": 2}
    assert all(len({x.rank for x in by["layout"] if x.base.layout == k}) == 2 for k in lay)
    assert {x.base.remove_low for x in by["lengths"]} == {True, False} and all(x.base.lengths and x.rank == "random" for x in by["lengths"])
    assert [(x.base.a_pad // 64, x.base.C, x.em_fast) for x in by["handed_back"]] == [(136, 130, 0), (16, 4097, 0), (8, 32769, -1)]
    assert [x.id for x in by["keyerror"]] == ["keyerror", "keyerror_cluster", "keyerror_any"]
    assert [xc.cluster_sized(x) or x.em_fast < 0 for x in by["keyerror"]] == [False, True, True]
    assert [x.id for x in by["deep_decay"]] == ["decay_gate", "decay_gate_cluster", "decay_zero", "decay_denormal", "decay_band", "decay_band2"]
    assert xc.cluster_sized(xc.BY_ID["decay_gate_cluster"]) and not xc.cluster_sized(xc.BY_ID["decay_gate"])
    assert len({x.id for x in xc.CASES}) == len(xc.CASES)
    # table lookups hold four classes per thread: every case that runs with them is inside the default gate
    assert all(x.base.C <= MAX_CLASSES and x.em_fast == 0 for x in xc.CASES if x.lookup)


def collections_count(it):
    out = {}
    for k in it:
        out[k] = out.get(k, 0) + 1
    return out


@pytest.mark.parametrize("family", ["sum_groups", "allele_tiles", "class_tiles", "layout"])
def test_equality_is_sharper_than_a_tolerance(orc, family):
    """em_ref sums in numpy's order, the oracle in the reference's: on some case of the family the two results differ in a bit, so
    a kernel that summed in another order would fail `==` there."""
    differ = []
    for x in xc.CASES:
        if x.family != family or x.base.C * x.base.n > 300000:
            continue
        exp, _ = oracle_dense(orc, x)
        if not np.array_equal(xc.reference(x)[1].dense(x.base.n_alleles), exp):
            differ.append(x.id)
    print(family, "em_ref differs from the oracle in some bit on", differ)
    assert differ


def test_where_the_last_dict_is_not_in_first_class_order():
    """The reference fills a dict over the classes it WALKS.  Everywhere but in decay_band2 every survivor enters the last dict at its
    first class, so the dict order is engine.em_order(first, rank, present); in decay_band2 the last application skips a class whose
    members are all at 0.0, one survivor enters later and the order differs: derive_order's `walk` argument at work."""
    import hisatgenotype_amd.engine as engine
    odd = []
    for x in xc.CASES:
        if x.family == "keyerror":
            continue
        b = xc.xbuild(x)
        r = xc.reference(x)[1]
        if not np.array_equal(r.first_walked, r.first_class):
            first, walked, present = (np.full(b.n_alleles, -1, np.int64) for _ in range(3))
            first[r.alleles], walked[r.alleles], present[r.alleles] = r.first_class, r.first_walked, 1
            assert engine.em_order(first, b.rank, present > 0) != engine.em_order(walked, b.rank, present > 0)
            odd.append(x.id)
    assert odd == ["decay_band2"]


def test_the_recorder_sees_every_application():
    """em_ref.Problem.on_step: three applications of the map per iteration (the third on the extrapolated estimate), the first
    one on the initial estimate."""
    x = xc.BY_ID["sum8"]
    b = xc.xbuild(x)
    seen, r = xc.trajectory(x, int(b.actives[0]))
    assert not r.sv_failed and len(seen) == 3 * r.n_iter
    pr = ec.em_ref.Problem(b.idx, b.off, b.counts)
    cnt = np.bincount(pr.cidx, weights=pr.cnt_el / pr.size[pr.cls], minlength=pr.n)
    assert seen[0] == (cnt / cnt.sum())[0]
