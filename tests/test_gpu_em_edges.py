"""The chip-wide table-lookup EM (csrc/hgx_em.hip: hgx_ensure_compact, k_lutmatvec<ROWS|COLS>, k_lut_rows_fused<0|1>, k_em_squarem,
k_em_advance, k_em_tail, k_em_finish) at its STRUCTURAL EDGES, judged by the C oracle.

The class sets are built with Classes.from_host and carry NO allele rank: there is no reference-order kernel and no tie re-run to
rescue a wrong value, and the table-lookup path runs for every case (all have more than 64 classes).  Every case of
tests/em_edge_cases.py -- whose premises tests/test_em_ref.py checks on the CPU: every decision of the reference at least 1e-7
from its threshold, weight on both sides of every size edge -- is run

  * twice on the same class set (the compaction is cached on it; the kernels state a fixed summation order): second `==` first;
  * against orc.single_abundance: same survivors, same iteration count, max |p - exp| <= 1e-9 (the bound of the README's table and
    DESIGN.md 5.4), first classes `==` em_ref's;
  * with em_skip="fuse" (standalone k_em_squarem / k_em_advance) and em_skip="defer" (the rows pass combines its own slabs through the
    ticket): `==` the default form, as the kernels' comments claim (same element-to-thread map, same slab order);
  * with em_skip="tail" (the full passes go on after the pruning): <= 1e-9, same survivors and iteration count.

Where the oracle raises KeyError the product must raise HgxError HGX_EKEY.

family           case ids                 what sits on the edge (csrc/hgx_em.hip)
compact_length   n1 .. n1025              a1p = max(512, ceil512(n)), k_zero_padding rows [n, a1p), k_act_from_mask; 2nd allele slab at 513, 2nd cols chunk at 1 025
layout           one_word gap_word        k_col_or, k_transpose_compact's `m == 0` return and base[aw] + popc; h_act[j] < n_alleles
                 last_bit ragged
row_width        w8 w128 w136 w520        k_col_or 128 / 256 threads at w64 = 128; host-uploaded base / act above w64 = 512
classes          C65 .. C16385            c64 rounded to 8 words; slabs of 512 and chunks of 1 024 classes; 17 class slabs (groups of 16 in the cols
                                          prologue) at 8 193; 33 (groups of 32 in the ticket combine, em_skip="defer") at 16 385
long_vectors     long8191 .. long8193     fuse needs a1p <= 8 192: above, the strided k_em_squarem / k_em_advance and 17 allele slabs
empty_chunk      chunk_high chunk_low     k_lutmatvec<COLS>'s return for a 1 024-row chunk without a present allele (n = 2 049: three chunks)
                 chunk_last
lengths          len_low len_full         l[j] = allele_len[h_act[j]]; k_em_finish's p / len / tot
batching         iter4 .. iter_ge20       the host loop: 4 iterations, up to 7 more, then the speculative tail
tail             surv64 surv65 masks64    k_em_tail: `A1 > 64`, `n_keys > 64`, the second round of its class-word loop at 8 193 classes, a
                 masks65 tail_C*          ragged last class word
"""
import numpy as np
import pytest

import em_edge_cases as ec
from hisatgenotype_amd import capi, engine

pytestmark = pytest.mark.gpu

BOUND = 1e-9           # README's table and DESIGN.md 5.4: the table-lookup EM against the reference
WORST = {}             # family -> largest |p - exp| seen (printed by the last test: a measurement, not a bound)


def _em(cl, c, lengths):
    p, first, it = cl.em_ordered(c.n_alleles, c.remove_low, lengths)
    return p, first, it


@pytest.mark.parametrize("c", ec.CASES, ids=[c.id for c in ec.CASES])
def test_table_lookup_em_at_the_edge(orc, c):
    b = ec.build(c)
    try:
        oa, op, oit = orc.single_abundance_flat(c.n_alleles, b.off, b.idx, b.counts, c.remove_low, b.lengths)
        exp = np.full(c.n_alleles, -1.0)
        exp[oa] = op
    except KeyError:
        exp = None
    cl = engine.Classes.from_host(b.rows(c.a_pad), b.counts, c.a_pad)
    try:
        reruns = engine.em_tie_reruns()
        if exp is None:
            for skip in (None, "fuse", "defer", "tail"):
                with engine.test_switches(**({"em_skip": skip} if skip else {})):
                    with pytest.raises(capi.HgxError) as e:
                        _em(cl, c, b.lengths)
                assert e.value.code == -4                       # HGX_EKEY
            return
        p, first, it = _em(cl, c, b.lengths)
        assert not engine.em_last_exact()
        err = float(np.max(np.abs(p - exp))) if np.array_equal(p >= 0.0, exp >= 0.0) else np.inf
        print("%s: iterations %d (oracle %d), survivors %d, max |p - exp| %.3e" % (c.id, it, oit, int((p >= 0.0).sum()), err))
        WORST[c.family] = max(WORST.get(c.family, 0.0), err)
        assert it == oit
        assert np.array_equal(p >= 0.0, exp >= 0.0)
        assert err <= BOUND
        _, ref = ec.reference(c)
        want_first = np.full(c.n_alleles, -1, np.int64)
        want_first[ref.alleles] = ref.first_class
        assert np.array_equal(first, want_first)
        p2, first2, it2 = _em(cl, c, b.lengths)                 # the cached compaction, the same sums
        assert it2 == it and np.array_equal(p2, p) and np.array_equal(first2, first)
        for skip in ("fuse", "defer"):
            with engine.test_switches(em_skip=skip):
                q, qf, qit = _em(cl, c, b.lengths)
                assert not engine.em_last_exact()
            assert qit == it, (skip, qit, it)
            assert np.array_equal(q, p), (skip, float(np.max(np.abs(q - p))))
            assert np.array_equal(qf, first)
        with engine.test_switches(em_skip="tail"):
            t, tf, tit = _em(cl, c, b.lengths)
            assert not engine.em_last_exact()
        assert tit == oit and np.array_equal(t >= 0.0, exp >= 0.0) and np.max(np.abs(t - exp)) <= BOUND
        assert np.array_equal(tf, first)
        assert engine.em_tie_reruns() == reruns
    finally:
        cl.close()


def test_report_largest_differences():
    """Prints what the cases above measured, family by family (run with -s; profiles/em_edges_mi355x.txt keeps one such run)."""
    for fam, err in sorted(WORST.items()):
        print("em_edges %-16s max |p - exp| = %.3e" % (fam, err))
    assert all(err <= BOUND for err in WORST.values())
