"""The class dedup (csrc/hgx_dedup.hip) and the per-allele count pass (csrc/hgx_counts.hip) against a Python-dict reference
(tests/dedup_ref.py, pinned to the C oracle by tests/test_dedup_ref.py) on the structural edges of their kernels: the 1024-row
insert workgroup, the table size rule, the 4096-element scan tile, the one-round-trip switch at 65536 rows, the second trip of the
64-lane word loops (w64 > 64) and of the 128-bit compare (w64 > 128), probe chains that wrap, forged key collisions, and the
2^24 / 2^32 switches between the two Gene_counts forms.  Integers and bit rows only: every comparison is exact."""
import numpy as np
import pytest

import dedup_ref as dr
import tables
from hisatgenotype_amd import engine, locus as hl

pytestmark = pytest.mark.gpu


def _check(case, claim=None, keys=None):
    """dedup on the GPU == dedup_ref: class count, bit rows, counts, first rows (`keys` replace the case's own)"""
    rows, wts, mask, case_keys = case
    n, w64 = rows.shape
    dev = [engine.DevArray.from_host(x) if x is not None else None for x in (rows, case_keys if keys is None else keys, wts, mask)]
    cl = engine.Classes.dedup(dev[0], n, 64 * w64, hashes=dev[1], weights=dev[2], and_mask=dev[3])
    got = cl.to_host()
    want = dr.dedup_ref(case[0], case[1], case[2])
    assert cl.n_classes == len(want[1]), (cl.n_classes, len(want[1]))
    if claim is not None:
        assert cl.n_classes == claim
    for name, g, w in zip(("bits", "counts", "first rows"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    cl.close()


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193,
         65535, 65536, 65537]


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("texture", dr.TEXTURES)
@pytest.mark.parametrize("n_rows", SIZES)
def test_sizes_with_honest_keys(n_rows, texture, zeros):
    """a_pad = 512 (8 of 64 lanes carry words), keys from k_hash_rows; every size edge of insert, table rule, scan tile and the
    one-round-trip switch, crossed with all distinct / all identical / n // 3 + 1 classes (one founded by the last row) / two
    alternating classes, without and with zero rows at index 0, at the last index and beside every multiple of 1024."""
    case, claim = dr.make_claim(texture + ("_zeros" if zeros else ""), n_rows, 8, seed=n_rows)
    _check(case, claim)


@pytest.mark.parametrize("n_rows", [1, 1024, 4097, 65537])
def test_all_zero_input_gives_no_class(n_rows):
    _check((np.zeros((n_rows, 8), np.uint64), None, None, None), 0)


@pytest.mark.parametrize("a_pad", [512, 4096, 4608, 8704])
@pytest.mark.parametrize("n_rows", [257, 4097, 65537])
def test_row_width_one_bit_classes(n_rows, a_pad):
    """Classes that differ in exactly one bit -- bit 0 of word 0, bit 63 of the last word, odd-indexed words, words >= 64
    (a_pad 4608, 8704), words 130 and 131 (a_pad 8704): a kernel that drops a position merges two classes."""
    case, claim = dr.make_claim("onebit", n_rows, a_pad // 64, seed=a_pad + n_rows)
    assert claim == len(dr.onebit_positions(a_pad // 64)) + 1
    _check(case, claim)


@pytest.mark.parametrize("mask", ["mask_high", "mask_merge", "mask_third", "mask_all"])
@pytest.mark.parametrize("n_rows", [257, 4097, 65537])
def test_masks(n_rows, mask):
    """a_pad = 4608: a mask that keeps only words >= 64; one that erases the bits in which classes differ (they merge, counts add,
    the earlier first row, masked bits out); one that empties a third of the rows; one that empties all.  Then the same with
    useless supplied keys (all equal): keys are ignored when a mask is given."""
    case, claim = dr.make_claim(mask, n_rows, 72, seed=n_rows)
    _check(case, claim)
    _check(case, claim, keys=np.full(n_rows, 0x0123456789ABCDEF, np.uint64))


@pytest.mark.parametrize("n_rows", [1025, 65537])
def test_weights_beyond_32_and_40_bits(n_rows):
    """int64 weights with 0, 1 and values up to 2^40: class sums pass 2^32 and 2^40; a class of weight-0 rows is still a class."""
    case, claim = dr.make_claim("weights", n_rows, 8, seed=n_rows)
    want = dr.dedup_ref(*case[:3])[1]
    assert want.max() > 1 << 40 and want.min() == 0
    _check(case, claim)


@pytest.mark.parametrize("chain,n_rows", [("chain_global", 600), ("chain_global", 1500), ("chain_lds", 1024), ("chain_lds", 5000),
                                          ("chain_both", 1200)])
def test_steered_keys_probe_chains_wrap(chain, n_rows):
    """Supplied keys that honour the contract and steer the probing: every key of chain_global starts at slot T - 2 of the global
    table (T = max(1024, next power of two >= 2n), today's rule), every key of chain_lds at slot 2046 of the 2048-slot LDS table,
    chain_both both: the chains run over the end of the table and wrap.  Should the table rule change, the case still has to pass;
    it merely stops wrapping."""
    case, claim = dr.make_claim(chain, n_rows, 8, seed=n_rows)
    _check(case, claim)


def _forged_name(kind, weighted, masked):
    return "forged_" + kind + ("_w" if weighted else "") + ("_m" if masked else "")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["first", "last", "three", "five"])
@pytest.mark.parametrize("n_rows,a_pad", [(3000, 512), (70000, 512), (3000, 8704)])
def test_forged_collisions_against_the_reference(n_rows, a_pad, kind, weighted, masked):
    """Several DIFFERENT contents under one supplied key (each content under exactly one key, so the contract holds): the
    minority content at row 0 -- the slot's founder is the odd one out and the whole majority class is re-keyed -- or at the last
    row; three and five contents under one key; both sides of the one-round-trip switch; at a_pad = 8704 the contents of one key
    differ only in words >= 128 (the second trip of the 128-bit compare)."""
    case, claim = dr.make_claim(_forged_name(kind, weighted, masked), n_rows, a_pad // 64, seed=n_rows + a_pad)
    _check(case, claim)


@pytest.mark.parametrize("n_rows", [3, 1500, 70000])
def test_forged_all_rows_distinct_under_one_key(n_rows):
    """n - 1 rows on the re-key list"""
    case, claim = dr.make_claim("forged_all", n_rows, 8, seed=n_rows)
    _check(case, claim)


@pytest.mark.parametrize("name,n_rows", [("distinct", 65537), ("forged_five_w", 70000)])
def test_two_calls_on_the_same_buffers_give_the_same_result(name, n_rows):
    case = dr.make(name, n_rows, 8, seed=1)
    rows, wts, mask, keys = case
    dev = [engine.DevArray.from_host(x) if x is not None else None for x in (rows, keys, wts, mask)]
    out = []
    for _ in range(2):
        cl = engine.Classes.dedup(dev[0], n_rows, 512, hashes=dev[1], weights=dev[2], and_mask=dev[3])
        out.append(cl.to_host())
        cl.close()
    for x, y, w in zip(out[0], out[1], dr.dedup_ref(rows, wts, mask)):
        assert np.array_equal(x, y) and np.array_equal(x, w)


# ---- Gene_counts and first classes on hand-made class sets ----------------------------------------------------------------------------

def _random_bits(rng, n, w64, density):
    if density == 0:
        return np.zeros((n, w64), np.uint64)
    if density == 1:
        return np.full((n, w64), dr.EMPTY, np.uint64)
    return rng.randint(0, 256, size=(n, 8 * w64)).astype(np.uint8).view(np.uint64).reshape(n, w64)      # every bit set with p = 0.5


def _set_column(bits, a, members):
    bits[:, a >> 6] &= ~(np.uint64(1) << np.uint64(a & 63))
    bits[members, a >> 6] |= np.uint64(1) << np.uint64(a & 63)


def _check_counts(bits, cnt, a_pad, groups=()):
    cl = engine.Classes.from_host(bits, cnt, a_pad)
    want_c, want_f = dr.counts_ref(bits, cnt)
    got_c, got_f = cl.allele_counts()
    assert got_c.shape == want_c.shape and np.array_equal(got_c, want_c)
    assert np.array_equal(got_f.astype(np.int64), want_f)
    for alleles in groups:
        assert np.array_equal(cl.first_classes(alleles).astype(np.int64), want_f[np.asarray(alleles, np.int64)])
    cl.close()


@pytest.mark.parametrize("density", [0, 0.5, 1])
@pytest.mark.parametrize("n_classes", [1, 7, 8, 9, 255, 256, 257, 1023, 1025, 5000])
@pytest.mark.parametrize("a_pad", [512, 4608, 8704])
def test_allele_counts_and_first_classes(a_pad, n_classes, density):
    """a_pad 512: 48 of 64 lanes hold no half-word; 4608, 8704: a partial last span of half-words; class counts around the 8-row
    prefetch batch and the 256-class workgroup range.  At density 0.5 one allele sits only in the last class, one only in
    class 0 and one in none; first_classes() is asked for those and for one allele per word."""
    rng = np.random.RandomState(a_pad + n_classes)
    w64 = a_pad // 64
    bits = _random_bits(rng, n_classes, w64, density)
    groups = [np.array([64 * w + (7 * w) % 64 for w in range(w64)], np.int32)]
    if density == 0.5:
        only_last, only_first, nowhere = a_pad - 2, 37, [a_pad // 2 + 1, a_pad // 2 + 65, 0, a_pad - 1]
        _set_column(bits, only_last, [n_classes - 1])
        _set_column(bits, only_first, [0])
        for a in nowhere:
            _set_column(bits, a, [])
        groups += [np.array([only_last], np.int32), np.array(nowhere, np.int32), np.array([only_first], np.int32)]
    cnt = rng.randint(1, 1000, n_classes).astype(np.int64)
    _check_counts(bits, cnt, a_pad, groups)


def _switch_counts():
    full = (1 << 24) - 1
    return {
        "all 2^24 - 1, total 2^32 - 256": [full] * 256,
        "all 2^24 - 1 and one 1": [full] * 256 + [1],
        "one class at 2^24": [5] * 100 + [1 << 24] + [9] * 100,
        "one class at 2^24 - 1": [5] * 100 + [full] + [9] * 100,
        "total 2^32 - 1": [full] * 256 + [255],
        "total 2^32": [full] * 256 + [256],
        "total 2^32 + 1": [full] * 256 + [257],
        "one count of 2^44": [3] * 50 + [1 << 44] + [4] * 50,
    }


@pytest.mark.parametrize("a_pad", [512, 4608])
@pytest.mark.parametrize("which", sorted(_switch_counts()))
def test_allele_counts_on_both_sides_of_the_form_switches(which, a_pad):
    """Class counts at the limits that choose between the 24 x 32-bit integer form and the 64-bit form (every count < 2^24, total
    < 2^32): allele 3 is in every class, so its sum IS the total.  The result must be right on either side; which kernel ran is
    not asserted."""
    cnt = np.array(_switch_counts()[which], np.int64)
    rng = np.random.RandomState(len(cnt) + a_pad)
    bits = _random_bits(rng, len(cnt), a_pad // 64, 0.5)
    _set_column(bits, 3, np.arange(len(cnt)))
    _set_column(bits, a_pad - 1, np.arange(len(cnt)))
    want_c, _ = dr.counts_ref(bits, cnt)
    assert want_c[3] == want_c[a_pad - 1] == int(cnt.sum())
    _check_counts(bits, cnt, a_pad, [np.array([3, a_pad - 1], np.int32)])


# ---- the grouped route (pairs grouped by ref list, one row per list, weighted row dedup) against the oracle ------------------------------

N_PAIRS_MAX = 65537


@pytest.fixture(scope="module")
def level_case(orc):
    """65537 pairs drawn from 48 piece lists (repeats dominate) on a 700-allele locus, scored ONCE by the C oracle; a test of
    n pairs takes the first n.  Lists without a ref at one level, and lists that hold the same pieces in another order."""
    from hisatgenotype_amd import synth
    loc = synth.make_hla_like_locus(n_alleles=700, n_vars=300, seed=21)
    t = tables.oracle_tables(loc)
    pl = hl.PackedLocus.from_synth(loc)
    rng = np.random.RandomState(4)
    names = [n for n in loc.allele_names[1:] if n in loc.allele_vars]
    protos = []
    for _ in range(30):
        l = rng.randint(0, len(loc.backbone) - 200)
        r = l + rng.randint(20, 180)
        vs = [v for v in loc.allele_vars[names[rng.randint(len(names))]] if l <= loc.var_pos[v] <= r]
        if rng.rand() < 0.2 and vs:
            vs = vs[1:]
        protos.append((l, r, vs))
    lists = []                                             # a list = [(piece, levels)]
    for k in range(20):
        lists.append([(int(rng.randint(30)), ((0, 1), (1,), (0,), (1, 0))[rng.randint(4)]) for _ in range(rng.randint(1, 4))])
    lists += [list(reversed(x)) for x in lists[:12] if len(x) > 1]             # the same pieces in another order
    lists += [[(int(rng.randint(30)), (1,))] for _ in range(4)]               # no ref at the exon level
    lists += [[(int(rng.randint(30)), (0,))] for _ in range(4)]               # no ref at the gene level
    lists.append([])                                                          # no ref at all
    pick = np.concatenate([[0], rng.permutation(len(lists)), rng.randint(0, len(lists), N_PAIRS_MAX - len(lists) - 1)])
    pair_off, level, left, right, id_off, ids = [0], [], [], [], [0], []
    for p in pick.tolist():
        for piece, lvs in lists[p]:
            l, r, vs = protos[piece]
            for lv in lvs:
                level.append(lv); left.append(l); right.append(r)
                ids += vs
                id_off.append(len(ids))
        pair_off.append(len(level))
    arrs = (np.array(pair_off, np.int32), np.array(level, np.uint8), np.array(left, np.int32), np.array(right, np.int32),
            np.array(id_off, np.int32), np.array(ids, np.int32))
    eb, gb, _, _ = orc.score_pairs(orc.make_locus(t), t["exon_keys"], t["gene_keys"], *arrs)
    return pl, arrs, (eb, gb), (t["n_alleles"] + 63) // 64


@pytest.mark.parametrize("n_pairs", [1, 255, 256, 257, 513, 4097, N_PAIRS_MAX])
def test_grouped_route_against_the_oracle(level_case, n_pairs):
    """Classes.of_level at both levels == the oracle's per-pair rows through dedup_ref: bits, pair counts and first pairs -- a
    reference that shares no code with the GPU's own per-pair route."""
    pl, (pair_off, level, left, right, id_off, ids), ref_rows, w = level_case
    n_refs = int(pair_off[n_pairs])
    batch = pl.batch_from_haplotypes(pair_off[:n_pairs + 1], level[:n_refs], left[:n_refs], right[:n_refs], id_off[:n_refs + 1],
                                     ids[:int(id_off[n_refs])])
    assert batch.n_pairs == n_pairs
    db = engine.DeviceBatch(batch)
    bufs = engine.ScoreBuffers(pl, db)
    engine.piece_compat(pl, db, bufs)
    for lv in (0, 1):
        want_b, want_c, want_f = dr.dedup_ref(ref_rows[lv][:n_pairs])
        cl = engine.Classes.of_level(pl, db, bufs, lv)
        got_b, got_c, got_f = cl.to_host()
        assert cl.n_classes == len(want_c)
        assert np.array_equal(got_b[:, :w], want_b) and not got_b[:, w:].any()
        assert np.array_equal(got_c, want_c) and np.array_equal(got_f, want_f)
        cl.close()
