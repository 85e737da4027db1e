"""The grouped route of the class tables -- hgx_group_pairs + hgx_level_classes_grouped (csrc/hgx_dedup.hip) -- on the structural
edges of its kernels: the wavefront (equal keys elect a leader), the 1024-row insert workgroup on 4 and on 16 wavefronts, the
4096-element scan tile that also writes first rows and counts.  Judged by the per-pair route (hgx_pair_classes +
hgx_dedup_classes) and by the dict reference of tests/dedup_ref.py on the per-pair rows; a_pad = 512 throughout (the structure,
not the width, is under test).  Integers and bit rows only: every comparison is exact."""
import ctypes as C
import types

import numpy as np
import pytest

import dedup_ref as dr
from hisatgenotype_amd import capi, engine, locus as hl

pytestmark = pytest.mark.gpu

N_MAX = 4097
OTHER = np.uint32(1 << 31)          # level bit of a piece ref: 0 = exon level, 1 = gene level


@pytest.fixture(scope="module")
def ctx():
    """A 400-allele locus (a_pad 512) with ~30 distinct pieces, their allele bitsets computed once; every test brings its own
    pair -> ref lists over those pieces."""
    from hisatgenotype_amd import synth
    loc = synth.make_hla_like_locus(n_alleles=400, n_vars=300, seed=21)
    pl = hl.PackedLocus.from_synth(loc)
    assert pl.w64 == 8
    rng = np.random.RandomState(4)
    names = [n for n in loc.allele_names[1:] if n in loc.allele_vars]
    left, right, id_off, ids = [], [], [0], []
    for _ in range(30):
        l = rng.randint(0, len(loc.backbone) - 200)
        r = l + rng.randint(20, 180)
        vs = [v for v in loc.allele_vars[names[rng.randint(len(names))]] if l <= loc.var_pos[v] <= r]
        left.append(l); right.append(r)
        ids += vs
        id_off.append(len(ids))
    batch = pl.batch_from_haplotypes(np.arange(31), np.zeros(30, np.uint8), left, right, id_off, ids)     # one piece per pair
    db = engine.DeviceBatch(batch)
    bufs = engine.ScoreBuffers(pl, types.SimpleNamespace(n_pairs=N_MAX, n_pieces=db.n_pieces))
    engine.piece_compat(pl, db, bufs)
    return pl, db, bufs, db.n_pieces


def _list_of(k, n_pieces, length=3):
    """list number k: the digits of k in base n_pieces -- distinct numbers give distinct ORDERED lists of one length"""
    out = []
    for _ in range(length):
        out.append(k % n_pieces)
        k //= n_pieces
    assert k == 0
    return out


def _upload(lists):
    """[[ref, ...] per pair] -> an object with the fields the engine's stage wrappers read"""
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    refs = np.array([r for x in lists for r in x] or [0], np.uint32)
    return types.SimpleNamespace(n_pairs=len(lists), pair_off=capi.DevArray.from_host(off), pair_ref=capi.DevArray.from_host(refs))


def _level_list(x, level):
    return tuple(int(r) & 0x7fffffff for r in x if (int(r) >> 31) == level)


def _check(ctx, lists, level=0):
    """grouped route == per-pair route == dict reference on the per-pair rows: class count, rows, counts, first pairs (all in
    first-seen order); and the number of groups == the number of distinct ordered lists at the level"""
    pl, _, bufs, _ = ctx
    n = len(lists)
    fake = _upload(lists)
    g = engine.Groups(fake, level)
    cl = engine.Classes.of_level(pl, fake, bufs, level, groups=g)
    assert g.n_groups == len({_level_list(x, level) for x in lists})
    got = cl.to_host()
    cl.close()
    g.close()
    engine.pair_classes(pl, fake, bufs, exon=level == 0, gene=level == 1)
    rows_dev, hash_dev = (bufs.exon_bits, bufs.exon_hash) if level == 0 else (bufs.gene_bits, bufs.gene_hash)
    per_pair = engine.Classes.dedup(rows_dev, n, 512, hashes=hash_dev)
    plain = per_pair.to_host()
    per_pair.close()
    want = dr.dedup_ref(rows_dev.to_host()[:n])
    for name, a, b, w in zip(("bits", "counts", "first pairs"), got, plain, want):
        assert a.shape == w.shape and np.array_equal(a, w), name + " (grouped route against the reference)"
        assert np.array_equal(b, w), name + " (per-pair route against the reference)"
    return got


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_sizes(ctx, n_pairs):
    """the wavefront, both forms of the insert workgroup (256 lanes x 4 rows, 1024 lanes) and the scan tile; n // 3 + 1 lists, the
    last pair founds one of them"""
    P = ctx[3]
    rng = np.random.RandomState(n_pairs)
    k = n_pairs // 3 + 1
    lab = np.concatenate([rng.randint(0, max(k - 1, 1), n_pairs - 1), [k - 1]]).astype(np.int64)
    _check(ctx, [_list_of(int(x), P) for x in lab])


def _labels(kind, n, rng):
    lab = np.arange(1, n + 1)                                   # all distinct; 0 = the hot key
    if kind == "one_key":
        lab[:] = 0
    elif kind == "wave_mix":                                    # every lane of the even wavefronts, exactly one lane of the odd ones
        wave = np.arange(n) // 64
        lab[wave % 2 == 0] = 0
        lab[(wave % 2 == 1) & (np.arange(n) % 64 == 17)] = 0
    elif kind == "last_lane_first":                             # first seen by the LAST lane of the LAST wavefront of workgroup 0
        lab[[1023, 1024 + 5, 1024 + 64, 2047, 2048 + 700, n - 1]] = 0
        lab[[255, 256, 700]] = n + 7                            # ... and by the last lane of the 256-lane workgroup's first round
    elif kind == "fifth_empty":
        lab = rng.randint(1, 300, n)
        lab[rng.rand(n) < 0.2] = -1                             # the empty list
    elif kind == "repeats":
        lab = rng.randint(0, 40, n)
    else:
        assert kind == "distinct"
    return lab


@pytest.mark.parametrize("kind", ["one_key", "wave_mix", "last_lane_first", "distinct", "fifth_empty"])
def test_key_distributions(ctx, kind):
    """2 900 pairs = three insert workgroups, 46 wavefronts.  A pair without refs still has a class (Q4)."""
    P = ctx[3]
    n = 2900
    lab = _labels(kind, n, np.random.RandomState(7))
    got = _check(ctx, [[] if x < 0 else _list_of(int(x), P) for x in lab])
    if kind == "one_key":
        assert len(got[1]) == 1 and got[1][0] == n and got[2][0] == 0


def test_lists_that_differ_only_in_order_stay_separate_groups(ctx):
    P = ctx[3]
    lists = []
    for p in range(1500):
        a, b = p % 5, 5 + p % 3
        lists.append([a, b] if (p // 7) % 2 == 0 else [b, a])
    assert len({tuple(x) for x in lists}) == 30
    _check(ctx, lists)                                          # (_check counts the groups: 30, whatever the classes)


def test_a_pair_with_400_refs(ctx):
    P = ctx[3]
    rng = np.random.RandomState(11)
    long_list = [int(x) for x in rng.randint(0, P, 400)]
    lists = [_list_of(int(x), P) for x in rng.randint(0, 50, 1300)]
    for p in (0, 64, 1023, 1299):
        lists[p] = list(long_list)
    lists[700] = long_list[:399]                                # one ref short: another list
    _check(ctx, lists)


@pytest.mark.parametrize("level", [0, 1])
def test_refs_of_the_other_level_interleaved(ctx, level):
    """pairs whose lists agree at the level under test group together whatever they carry at the other level"""
    P = ctx[3]
    rng = np.random.RandomState(13 + level)
    mine, other = np.uint32(level << 31), np.uint32((1 - level) << 31)
    lists = []
    for p in range(2100):
        own = [int(np.uint32(r) | mine) for r in _list_of(int(rng.randint(0, 60)), P)]
        out = []
        for r in own:
            out += [int(np.uint32(x) | other) for x in rng.randint(0, P, rng.randint(0, 3))] + [r]
        out += [int(np.uint32(x) | other) for x in rng.randint(0, P, rng.randint(0, 2))]
        lists.append(out)
    lists[5] = [int(np.uint32(3) | other)]                      # nothing at this level: the empty list
    _check(ctx, lists, level)


# ---- many tasks in one launch chain: groups and classes never cross tasks -------------------------------------------------------------

def _seg_calls():
    """the segment-aware forms are C++ entry points of libhgx (csrc/hgx_common.hpp; hgx_type_many calls them), not part of the C ABI"""
    L = capi.lib()
    return (getattr(L, "_Z19hgx_group_pairs_segPP10hgx_groupsPKiPKjiiS5_Pv"),
            getattr(L, "_Z29hgx_level_classes_grouped_segPP11hgx_classesPK9hgx_indexPKmPKiPKjP10hgx_groupsPmSD_SA_Pv"),
            getattr(L, "_Z21hgx_dedup_classes_segPP11hgx_classesPKmS3_liPKjPv"))


def _vp(a):
    return C.c_void_p(a.ptr)


def test_segmented_forms_with_identical_lists_in_three_tasks(ctx):
    pl, _, bufs, P = ctx
    group_seg, grouped_seg, dedup_seg = _seg_calls()
    rng = np.random.RandomState(17)
    per_task = 700
    one = [_list_of(int(x), P) for x in rng.randint(0, 25, per_task)]
    one[3] = []
    lists = one + one + one                                     # the same lists in every task
    n = len(lists)
    seg = np.repeat(np.arange(3, dtype=np.uint32), per_task)
    fake = _upload(lists)
    d_seg = capi.DevArray.from_host(seg)
    g, h = C.c_void_p(), C.c_void_p()
    capi.check(group_seg(C.byref(g), _vp(fake.pair_off), _vp(fake.pair_ref), C.c_int32(n), C.c_int32(0), _vp(d_seg), None))
    ng = C.c_int64()
    capi.check(capi.lib().hgx_groups_dims(g, C.byref(ng), None))
    assert ng.value == 3 * len({tuple(x) for x in one})
    capi.check(grouped_seg(C.byref(h), pl.index(), _vp(bufs.compat),
                           _vp(fake.pair_off), _vp(fake.pair_ref), g, _vp(bufs.exon_bits), _vp(bufs.exon_hash), _vp(d_seg), None))
    cl = engine.Classes(h)
    got = cl.to_host()
    cl.close()
    capi.lib().hgx_groups_destroy(g)
    engine.pair_classes(pl, fake, bufs, gene=False)
    h2 = C.c_void_p()
    capi.check(dedup_seg(C.byref(h2), _vp(bufs.exon_bits), _vp(bufs.exon_hash), C.c_int64(n), C.c_int32(512), _vp(d_seg), None))
    cl2 = engine.Classes(h2)
    plain = cl2.to_host()
    cl2.close()
    rows = bufs.exon_bits.to_host()[:n]
    tagged = np.concatenate([rows, (seg.astype(np.uint64) + np.uint64(1))[:, None]], axis=1)      # the reference: the task is part of the row
    wb, wc, wf = dr.dedup_ref(tagged)
    want = (np.ascontiguousarray(wb[:, :8]), wc, wf)
    assert len(wc) == 3 * len(dr.dedup_ref(rows[:per_task])[1])
    for name, a, b, w in zip(("bits", "counts", "first pairs"), got, plain, want):
        assert a.shape == w.shape and np.array_equal(a, w), name + " (grouped, segmented)"
        assert np.array_equal(b, w), name + " (per pair, segmented)"


# ---- the weighted row dedup and forged key collisions through supplied keys (the route of test_gpu_dedup_edges.py) --------------------------

def _check_rows(case, claim=None):
    rows, wts, mask, keys = case
    n, w64 = rows.shape
    dev = [capi.DevArray.from_host(x) if x is not None else None for x in (rows, keys, wts, mask)]
    cl = engine.Classes.dedup(dev[0], n, 64 * w64, hashes=dev[1], weights=dev[2], and_mask=dev[3])
    got = cl.to_host()
    want = dr.dedup_ref(rows, wts, mask)
    assert cl.n_classes == len(want[1]) and (claim is None or cl.n_classes == claim)
    for name, a, w in zip(("bits", "counts", "first rows"), got, want):
        assert a.shape == w.shape and np.array_equal(a, w), name
    cl.close()


@pytest.mark.parametrize("kind", ["one_key", "wave_mix", "last_lane_first", "repeats"])
def test_weights_near_2_40_on_the_row_dedup(kind):
    """every row weighs 2^40 - 1, 2^40 or 2^40 + 1: the wavefront's sum, the LDS sum and the global sum all pass 2^32 and 2^40"""
    n = 2900
    rng = np.random.RandomState(23)
    lab = _labels(kind, n, rng)
    uniq, cls = np.unique(lab, return_inverse=True)
    pool = rng.randint(0, 256, size=(len(uniq), 64)).astype(np.uint8).view(np.uint64)
    pool[:, 0] = np.arange(1, len(uniq) + 1, dtype=np.uint64)                      # distinct and non-zero
    rows = np.ascontiguousarray(pool[cls])
    wts = ((1 << 40) + rng.randint(-1, 2, n)).astype(np.int64)
    want = dr.dedup_ref(rows, wts)[1]
    assert want.max() > 1 << 41
    _check_rows((rows, wts, None, None), len(uniq))


@pytest.mark.parametrize("n_rows", [1025, 4097])
@pytest.mark.parametrize("kind", ["first", "last"])
def test_forged_key_collision_with_the_odd_row_first_and_last(kind, n_rows):
    """two different rows under one supplied 64-bit key, the minority content at row 0 or at the last row: the salted
    re-insertion resolves it; weighted"""
    case, claim = dr.make_claim("forged_" + kind + "_w", n_rows, 8, seed=n_rows)
    _check_rows(case, claim)
