"""The reference-order EM k_emx (csrc/hgx_emx.hip: all four instantiations) at its STRUCTURAL EDGES, judged by the C oracle.

The contract of this kernel is `==`: bit-identical doubles, the reference's iteration count, the reference's dict order (README,
DESIGN.md 4).  The cases are tests/emx_edge_cases.py, whose premises tests/test_emx_edge_ref.py checks on the CPU.  The class set is
Classes.from_host(...) plus set_allele_rank(rank); the oracle gets every class's members in key order (ascending rank).

form  what runs                                                          asserted
(a)   reference order on ONE workgroup (emx_no_cluster; em_skip="wave"    p == oracle, n_iter, em_last_exact, first classes == em_ref's,
      where C <= 64)                                                      em_last_order in the order of engine.em_order over the classes
                                                                          walked, ties as in the oracle's list, 2nd call == 1st
(b)   the default route (k_em_wave for <= 64 classes x <= 64 alleles,     == (a)
      a cluster for a lone big problem)
(c)   reference-order cluster, emx_cluster_wg = 2 | 3 | 64, where         == (a); emx_cluster_stats counts the job; fallbacks are
      C x a_pad >= 512 x 4 096 and for `any_size`                         printed, not asserted (a fallback re-runs on one workgroup)
(d)   table lookups on one workgroup (em_set_fast(True), emx_fast_wg=1)   survivors, n_iter, max |p - exp| <= 1e-9, not exact
(e)   table-lookup cluster, emx_fast_wg = 2 | 3 | 4                       == (d)
(f)   handed_back: status 1, the caller goes on                           <= 1e-9, survivors, n_iter, not exact
(g)   keyerror: forms (a) - (e), (c) on the two big cases                 HgxError HGX_EKEY; emx_cluster_stats counts the cluster forms

family            case ids                   what sits on the edge (csrc/hgx_emx.hip)
sum_groups        sum1 .. sum33              seq_sum / seq_sum2: groups of eight, two a trip, an exit each for n8 = 8, 16, 24, 32; pad_ordered's tail
sum_after_prune   prune1 .. prune65          the same sums on the dict the first pruning leaves: derive_order, pad_ordered again
allele_tiles      A63 .. A8192               A1w tiles of 64, tile pairs of the Mk build, keep0 / keep1 at tile 64, items of eight tiles in the
                                             transpose, 512-element slabs and tid + 1024 k of the lookup mode, the sort's N, XA = 8 192
class_tiles       C1 .. C4096                four classes a pass up to CpA, Cw tiles of 64, 512-class slabs, two 1 024-row tiles at 1 025 (mine_of)
any_size          any4097 .. any32768        em_fast = -1 up to the hard gate; cluster tile loops strided wave * n_wg + wg
row_width         w8 .. w128                 rows staged in two 64-lane halves (`lane + 64 < w64`)
layout            one_word_* .. ragged_*     rbm[(r >> 6) & 127] / rpre / srt against where the bits are, two ranks each
lengths           len_low len_full           vlen by allele id on a random rank
handed_back       back_w136 back_C4097       the gates w64 > 128, C > 4 096, C > 32 768 (em_fast = -1)
                  back_C32769
keyerror          keyerror keyerror_any      status 2, on one workgroup and reported by the leader of a cluster (260 classes at a_pad 8 192;
                  keyerror_cluster           4 098 classes with em_fast = -1)
deep_decay        decay_gate decay_zero      cols_share's plain `/` for a tile with 0 < p < 2^-600 beside fast tiles, the flag in a cluster,
                  decay_gate_cluster         p == 0.0 and denormal p in the dict
                  decay_denormal decay_band  (decay_band*: 64 alleles at once just above the denormal range)
                  decay_band2
"""
import numpy as np
import pytest

import emx_edge_cases as xc
from hisatgenotype_amd import capi, engine

pytestmark = pytest.mark.gpu

BOUND = 1e-9           # the bound tests/test_gpu_emx.py asserts for the table-lookup forms of this kernel
WORST = {}             # family -> largest |p - exp| of the table-lookup forms (printed by the last test: a measurement, not a bound)
FELL_BACK = {}         # family -> [cluster problems, those that fell back to one workgroup]

EXACT = [x for x in xc.CASES if x.family not in ("handed_back", "keyerror")]
LOOKUP = [x for x in xc.CASES if x.lookup and x.family != "keyerror"]
BACK = [x for x in xc.CASES if x.family == "handed_back"]


def _ids(xs):
    return [x.id for x in xs]


def _oracle(orc, x):
    b = xc.xbuild(x)
    oa, op, oit = orc.single_abundance_flat(b.n_alleles, b.off, b.kidx, b.counts, x.base.remove_low, b.lengths)
    exp = np.full(b.n_alleles, -1.0)
    exp[oa] = op
    return exp, oit, oa


def _classes(x):
    b = xc.xbuild(x)
    cl = engine.Classes.from_host(b.rows(), b.counts, b.a_pad)
    cl.set_allele_rank(b.rank)
    return cl


def _em(cl, x, default_route=False, **switches):
    """One EM of the case.  default_route: no switch at all, so that the library routes the problem itself (form (b): k_em_wave takes
    <= 64 classes over <= 64 alleles); every other form names its kernel, and for that k_em_wave is skipped where C <= 64."""
    b = xc.xbuild(x)
    assert default_route == (not switches)
    if not default_route and len(b.counts) <= 64:
        switches.setdefault("em_skip", "wave")
    with engine.test_switches(**switches):
        return cl.em_ordered(b.n_alleles, x.base.remove_low, b.lengths)


def _count_cluster(x, j, f):
    t = FELL_BACK.setdefault(x.family, [0, 0])
    t[0] += j
    t[1] += f


@pytest.mark.parametrize("x", EXACT, ids=_ids(EXACT))
def test_reference_order_at_the_edge(orc, x):
    """Forms (a), (b) and (c)."""
    b = xc.xbuild(x)
    exp, oit, oa = _oracle(orc, x)
    _, ref = xc.reference(x)
    want_first = np.full(b.n_alleles, -1, np.int64)
    want_first[ref.alleles] = ref.first_class
    cl = _classes(x)
    old = engine.em_set_fast(x.em_fast)
    try:
        p, first, it = _em(cl, x, emx_no_cluster="1")                                  # (a)
        exact = engine.em_last_exact()
        order = engine.em_last_order(b.n_alleles)
        same = np.array_equal(p >= 0.0, exp >= 0.0)
        print("%s (a): iterations %d (oracle %d), survivors %d, max |p - exp| %.3e" % (x.id, it, oit, int((p >= 0.0).sum()),
                                                                                       float(np.max(np.abs(p - exp))) if same else np.inf))
        assert it == oit
        assert same
        assert np.array_equal(p, exp), float(np.max(np.abs(p - exp)))
        assert exact
        assert np.array_equal(first, want_first)
        assert order is not None and np.array_equal(order >= 0, p >= 0.0)
        present = np.nonzero(p >= 0.0)[0]
        assert len(set(order[present].tolist())) == len(present)
        by_pos = present[np.argsort(order[present], kind="stable")]
        # the last dict is filled class by class over the classes that were WALKED: (first walked class, rank).  That is
        # engine.em_order(first, ...) unless the last application skipped an earlier class of the allele because every member of it
        # was at 0.0 (decay_band2: test_emx_edge_ref.py pins which cases); the reference's result list, a stable sort of that dict
        # by abundance, shows the order in its ties
        walked = np.full(b.n_alleles, -1, np.int64)
        walked[ref.alleles] = ref.first_walked
        static = by_pos.tolist() == engine.em_order(first, b.rank, p >= 0.0)
        dynamic = by_pos.tolist() == engine.em_order(walked, b.rank, p >= 0.0)
        ranked = by_pos[np.argsort(-p[by_pos], kind="stable")].tolist() == oa.tolist()
        print("%s (a): dict order is (first class, rank): %s, (first walked class, rank): %s; ties of the result list in the oracle's "
              "order: %s" % (x.id, static, dynamic, ranked))
        assert dynamic
        assert static or not np.array_equal(walked, want_first)
        assert ranked
        p2, first2, it2 = _em(cl, x, emx_no_cluster="1")
        assert it2 == it and np.array_equal(p2, p) and np.array_equal(first2, first)
        j0, f0 = engine.emx_cluster_stats()
        q, qf, qit = _em(cl, x, default_route=True)                                    # (b)
        j1, f1 = engine.emx_cluster_stats()
        assert engine.em_last_exact()
        assert qit == it and np.array_equal(q, p), float(np.max(np.abs(q - p)))
        assert np.array_equal(qf, first)
        big = xc.cluster_sized(x) or x.family == "any_size"
        assert j1 - j0 == (1 if big else 0)
        _count_cluster(x, j1 - j0, f1 - f0)
        if big:                                                                        # (c)
            for wg in (2, 3, 64):
                q, qf, qit = _em(cl, x, emx_cluster_wg=wg)
                assert engine.em_last_exact()
                j2, f2 = engine.emx_cluster_stats()
                print("%s (c): %d workgroups, fell back %d" % (x.id, wg, f2 - f1))
                assert j2 - j1 == 1 and 0 <= f2 - f1 <= 1
                _count_cluster(x, j2 - j1, f2 - f1)
                j1, f1 = j2, f2
                assert qit == it and np.array_equal(q, p), (wg, float(np.max(np.abs(q - p))))
                assert np.array_equal(qf, first)
    finally:
        engine.em_set_fast(old)
        cl.close()


@pytest.mark.parametrize("x", LOOKUP, ids=_ids(LOOKUP))
def test_table_lookups_at_the_edge(orc, x):
    """Forms (d) and (e)."""
    b = xc.xbuild(x)
    exp, oit, _ = _oracle(orc, x)
    _, ref = xc.reference(x)
    want_first = np.full(b.n_alleles, -1, np.int64)
    want_first[ref.alleles] = ref.first_class
    cl = _classes(x)
    old = engine.em_set_fast(True)
    try:
        p, first, it = _em(cl, x, emx_fast_wg=1)                                       # (d)
        exact = engine.em_last_exact()
        err = float(np.max(np.abs(p - exp))) if np.array_equal(p >= 0.0, exp >= 0.0) else np.inf
        print("%s (d): iterations %d (oracle %d), survivors %d, max |p - exp| %.3e" % (x.id, it, oit, int((p >= 0.0).sum()), err))
        WORST[x.family] = max(WORST.get(x.family, 0.0), err)
        assert it == oit
        assert np.array_equal(p >= 0.0, exp >= 0.0)
        assert err <= BOUND
        assert not exact
        assert np.array_equal(first, want_first)
        j0, f0 = engine.emx_cluster_stats()
        for wg in (2, 3, 4):                                                           # (e)
            q, qf, qit = _em(cl, x, emx_fast_wg=wg)
            assert not engine.em_last_exact()
            assert qit == it and np.array_equal(q, p), (wg, float(np.max(np.abs(q - p))))
            assert np.array_equal(qf, first)
        j1, f1 = engine.emx_cluster_stats()
        print("%s (e): fell back %d of %d" % (x.id, f1 - f0, j1 - j0))
        assert j1 - j0 == 3 and 0 <= f1 - f0 <= 3
        _count_cluster(x, j1 - j0, f1 - f0)
    finally:
        engine.em_set_fast(old)
        cl.close()


@pytest.mark.parametrize("x", BACK, ids=_ids(BACK))
def test_handed_back(orc, x):
    """Form (f): beyond a gate the kernel hands the problem back (status 1); the call goes on along the table-lookup path, succeeds,
    and does not report `exact`."""
    b = xc.xbuild(x)
    exp, oit, _ = _oracle(orc, x)
    cl = _classes(x)
    old = engine.em_set_fast(x.em_fast)
    try:
        reruns = engine.em_tie_reruns()
        p, first, it = _em(cl, x, default_route=True)
        exact = engine.em_last_exact()
        err = float(np.max(np.abs(p - exp))) if np.array_equal(p >= 0.0, exp >= 0.0) else np.inf
        print("%s (f): iterations %d (oracle %d), survivors %d, max |p - exp| %.3e" % (x.id, it, oit, int((p >= 0.0).sum()), err))
        WORST[x.family] = max(WORST.get(x.family, 0.0), err)
        assert it == oit
        assert np.array_equal(p >= 0.0, exp >= 0.0)
        assert err <= BOUND
        assert not exact
        assert engine.em_last_order(b.n_alleles) is None
        assert engine.em_tie_reruns() == reruns
    finally:
        engine.em_set_fast(old)
        cl.close()


KEYERR = [x for x in xc.CASES if x.family == "keyerror"]


@pytest.mark.parametrize("x", KEYERR, ids=_ids(KEYERR))
def test_keyerror(orc, x):
    """Form (g): where the reference raises KeyError (a class of count 0 whose members occur nowhere else), every form raises
    HgxError HGX_EKEY: one workgroup, the default route, the reference-order cluster where the problem is big enough for one
    (keyerror_cluster, keyerror_any: emx_cluster_stats must count the job), and the table-lookup forms where the case has them."""
    with pytest.raises(KeyError):
        _oracle(orc, x)
    big = xc.cluster_sized(x) or x.em_fast < 0
    forms = [(x.em_fast, dict(emx_no_cluster="1"), 0), (x.em_fast, {}, 1 if big else 0)]
    forms += [(x.em_fast, dict(emx_cluster_wg=wg), 1 if big else 0) for wg in (2, 3, 64)]
    if x.lookup:
        forms += [(True, dict(emx_fast_wg=1), 0)] + [(True, dict(emx_fast_wg=wg), 1) for wg in (2, 3, 4)]
    cl = _classes(x)
    try:
        for fast, sw, clusters in forms:
            old = engine.em_set_fast(fast)
            j0, f0 = engine.emx_cluster_stats()
            try:
                with pytest.raises(capi.HgxError) as e:
                    _em(cl, x, default_route=not sw, **sw)
            finally:
                engine.em_set_fast(old)
            j1, f1 = engine.emx_cluster_stats()
            print("%s (g): em_fast %s %s: code %d, cluster problems %d, fell back %d" % (x.id, fast, sw, e.value.code, j1 - j0, f1 - f0))
            assert e.value.code == -4, (fast, sw)               # HGX_EKEY
            assert j1 - j0 == clusters, (fast, sw)
            _count_cluster(x, j1 - j0, f1 - f0)
    finally:
        cl.close()


def test_a_table_lookup_call_forgets_the_reference_order_call_before_it():
    """State a call leaves for its thread (em_last_exact, em_last_order) is reset by the next call, whichever path that one takes: C65
    of this table on k_emx (exact, with an order), then C65 of em_edge_cases without a rank on the table-lookup path."""
    import em_edge_cases as ec
    x = xc.BY_ID["C65"]
    b = xc.xbuild(x)
    assert len(b.counts) == 65                                 # the smallest class count k_em_wave does not take
    cl = _classes(x)
    try:
        cl.em_ordered(b.n_alleles, x.base.remove_low, b.lengths)
        assert engine.em_last_exact() and engine.em_last_order(b.n_alleles) is not None
    finally:
        cl.close()
    c = next(c for c in ec.CASES if c.id == "C65")
    t = ec.build(c)
    cl = engine.Classes.from_host(t.rows(c.a_pad), t.counts, c.a_pad)
    try:
        cl.em_ordered(c.n_alleles, c.remove_low, t.lengths)
        assert not engine.em_last_exact()
        assert engine.em_last_order(c.n_alleles) is None
    finally:
        cl.close()


def test_report_largest_differences():
    """Prints what the cases above measured, family by family (run with -s; profiles/emx_edges_mi355x.txt keeps one such run)."""
    for fam, err in sorted(WORST.items()):
        print("emx_edges %-16s table lookups: max |p - exp| = %.3e" % (fam, err))
    for fam, (j, f) in sorted(FELL_BACK.items()):
        print("emx_edges %-16s cluster problems %d, fell back to one workgroup %d" % (fam, j, f))
    assert all(err <= BOUND for err in WORST.values())
