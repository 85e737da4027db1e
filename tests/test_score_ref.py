"""The plain statements of the scoring stage (tests/score_ref.py) against the C oracle and against hand-worked cases, and the
edge-case generators' own promises under those statements -- pinned here, on the CPU, before tests/test_gpu_score_edges.py
lets them judge a kernel."""
import numpy as np
import pytest

import score_ref as sr
import tables
from hisatgenotype_amd import locus as hl

LEVEL_COUNTS = (3, 4, 15, 16, 255, 256)


def _locus(kind):
    from hisatgenotype_amd import synth
    if kind == "hla":
        return synth.make_hla_like_locus(n_alleles=300, n_vars=400, seed=31)
    return synth.make_str_like_locus()


@pytest.mark.parametrize("kind", ["hla", "str"])
def test_statements_equal_the_c_oracle(orc, kind):
    """classes_ref(compat_ref(host masks of batch_from_haplotypes on the locus's host link_bits)) == orc.score_pairs, both levels,
    word for word; among the pairs are some whose refs of one level number exactly 3, 4, 15, 16, 255 and 256."""
    loc = _locus(kind)
    t = tables.oracle_tables(loc)
    pl = hl.PackedLocus.from_synth(loc)
    rng = np.random.RandomState(11)
    names = [n for n in loc.allele_names[1:] if n in loc.allele_vars]
    pair_off, level, left, right, id_off, ids = [0], [], [], [], [0], []

    def piece(lv):
        l = rng.randint(0, len(loc.backbone) - 200)
        r = l + rng.randint(1, 150)
        a = names[rng.randint(len(names))]
        vs = [v for v in loc.allele_vars[a] if l <= loc.var_pos[v] <= r]
        if rng.rand() < 0.3 and vs:
            vs = vs[:-1]
        level.append(lv); left.append(l); right.append(r)
        ids.extend(vs)
        id_off.append(len(ids))

    shapes = [(n, 2) for n in LEVEL_COUNTS] + [(1, n) for n in LEVEL_COUNTS] + [(0, 0), (0, 3), (2, 0), (1, 1), (5, 7)]
    for n_exon, n_gene in shapes:
        lvs = [0] * n_exon + [1] * n_gene
        for lv in rng.permutation(lvs).tolist():
            piece(lv)
        pair_off.append(len(level))
    arrs = (np.array(pair_off, np.int32), np.array(level, np.uint8), np.array(left, np.int32), np.array(right, np.int32),
            np.array(id_off, np.int32), np.array(ids, np.int32))
    eb, gb, _, _ = orc.score_pairs(orc.make_locus(t), t["exon_keys"], t["gene_keys"], *arrs)
    batch = pl.batch_from_haplotypes(*arrs)
    assert batch.n_pairs == len(shapes)
    pt = pl.tables()
    refs = batch.pair_ref
    per_pair = [refs[batch.pair_off[p]:batch.pair_off[p + 1]] >> 31 for p in range(batch.n_pairs)]
    assert [(int((x == 0).sum()), int((x == 1).sum())) for x in per_pair] == shapes
    compat = sr.compat_ref(pt["link_bits"], batch.pieces, batch.masks)
    w = (t["n_alleles"] + 63) // 64
    for lv, want, mask in ((0, eb, pt["exon_mask"]), (1, gb, pt["gene_mask"])):
        got = sr.classes_ref(compat, batch.pair_off, refs, lv, mask)
        assert np.array_equal(got[:, :w], want), (kind, lv, np.flatnonzero((got[:, :w] != want).any(axis=1)))
        assert not got[:, w:].any()


def test_hand_worked_classes():
    """four alleles under the mask 0b01111 of five, rows written out: ties, a masked-out winner, no refs, a duplicate ref"""
    compat = np.zeros((4, 8), np.uint64)
    compat[:, 0] = [0b00011, 0b00110, 0b10101, 0b00000]
    mask = np.zeros(8, np.uint64)
    mask[0] = 0b01111
    L = np.uint32(1 << 31)
    pairs = [
        ([0, 1], 0, 0b00010),                       # counts 1 2 1 0 0: allele 1
        ([0, 2], 0, 0b00001),                       # counts 2 1 1 0 1: allele 0
        ([1, 2], 0, 0b00100),                       # counts 1 1 2 0 1: allele 2
        ([0], 0, 0b00011),                          # a tie of two
        ([2, 2, 2, 0, 1], 0, 0b00101),              # counts 4 2 4 0 3: alleles 0 and 2 tie at 4
        ([3], 0, 0b01111),                          # a row that holds nobody: every masked allele at count 0
        ([], 0, 0b01111),                           # no refs at all
        ([0 | L, 1 | L], 0, 0b01111),               # refs of the other level only
        ([0 | L, 1 | L], 1, 0b00010),               # ... which the other level counts
        ([0, 1, 2], 0, 0b00111),                    # counts 2 2 2 0 1: three tie
        ([0, 0, 1, 2], 0, 0b00011),                 # ... and with row 0 twice it counts twice: 3 3 2 0 1
    ]
    off = np.cumsum([0] + [len(r) for r, _, _ in pairs]).astype(np.int32)
    refs = np.array([x for r, _, _ in pairs for x in r], np.uint32)
    for lv in (0, 1):
        got = sr.classes_ref(compat, off, refs, lv, mask)
        assert not got[:, 1:].any()
        for p, (_, level, want) in enumerate(pairs):
            if level == lv:
                assert int(got[p, 0]) == want, (p, bin(int(got[p, 0])))
    # the mask excludes the allele with the largest count: allele 4 alone in three rows, allele 1 in one
    compat[:, 0] = [0b10000, 0b10000, 0b10010, 0]
    got = sr.classes_ref(compat, np.array([0, 3], np.int32), np.array([0, 1, 2], np.uint32), 0, mask)
    assert int(got[0, 0]) == 0b00010
    full = mask.copy()
    full[0] = 0b11111
    assert int(sr.classes_ref(compat, np.array([0, 3], np.int32), np.array([0, 1, 2], np.uint32), 0, full)[0, 0]) == 0b10000
    assert not sr.classes_ref(compat, np.array([0, 3], np.int32), np.array([0, 1, 2], np.uint32), 0, np.zeros(8, np.uint64)).any()


def test_hand_worked_compat():
    bits = np.array([[0b1010, 0b1000, 0b0010, 0], [0b0001, 0b0001, 0b0011, 0]], np.uint32)
    bits = np.concatenate([bits, np.zeros((2, 60), np.uint32)], axis=1)
    pieces = np.array([(0, 0, 1), (2, 0, 2), (6, 1, 1), (8, 0, 1), (10, 0, 1)], sr.PIECE_DTYPE)
    masks = np.array([0b1010, 0b1000,                   # word 0: bit 3 set, bit 1 clear: allele 1 only
                      0b1000, 0b1000, 0b0011, 0b0001,   # word 0 bit 3 set AND word 1 == 01 under 11: alleles 0, 1
                      0b0010, 0b0000,                   # word 1 bit 1 clear: everyone but allele 2, the padding included
                      0, 0,                             # passes everything
                      0b0001, 0b0011], np.uint32)       # a P bit outside MP: nobody
    got = sr.compat_ref(bits, pieces, masks)
    assert got.shape == (5, 1)
    assert [int(x) for x in got[:, 0]] == [0b0010, 0b0011, sr.M64 ^ 0b0100, sr.M64, 0]


@pytest.mark.parametrize("w64", [8, 72])
@pytest.mark.parametrize("n", sr.N_TOTALS)
def test_pair_generator_keeps_its_promises(n, w64):
    """x has count n_lv, y has n_lv - 1, nobody else more than n_lv - 2; the class is what Pair.promised_class says; the refs
    split as asked"""
    n_alleles, em, gm = sr.level_masks(w64)
    masks = (em, gm)
    assert n_alleles == 64 * w64 - 1 and not sr.members(em | gm)[n_alleles:].any()
    assert (em != gm).any() and (~sr.members(em | gm))[:n_alleles].sum() > 10 and sr.members(em & gm).sum() > 10
    pairs = sr.sweep_pairs(w64, masks, n)
    assert len(pairs) == 12
    compat, off, refs = sr.assemble(pairs, w64)
    assert np.array_equal(np.diff(off), [n] * 12)
    for lv in (0, 1):
        got = sr.classes_ref(compat, off, refs, lv, masks[lv])
        for p, pr in enumerate(pairs):
            if pr.level != lv:
                continue
            mine = refs[off[p]:off[p + 1]]
            assert int(((mine >> 31) == lv).sum()) == pr.n_lv
            count = sr.counts_of_pair(compat, mine, lv)
            assert count[pr.x] == pr.n_lv and count[pr.y] == max(pr.n_lv - 1, 0)
            rest = np.delete(count, [pr.x, pr.y])
            assert rest.max() <= max(pr.n_lv - 2, 0)
            under = sr.members(masks[lv])
            assert under[pr.y] and under[pr.x] == pr.x_masked
            assert np.array_equal(got[p], pr.promised_class(masks[lv])), (n, lv, p)
    splits = {(pr.n_lv, pr.n_refs - pr.n_lv) for pr in pairs}
    assert splits == {sr.split_counts(n, s) for s in sr.SPLITS}


def test_special_alleles_are_where_the_widths_need_them():
    for w64 in (8, 64, 72, 128, 136, 256, 264, 512):
        n_alleles, em, gm = sr.level_masks(w64)
        sp = sr.special_alleles(w64)
        assert 0 in sp and 64 * w64 - 2 in sp and 64 * (w64 - 2) + 63 in sp
        for edge in (64, 128, 256):
            if edge < w64:
                assert {a >> 6 for a in sp} >= {edge - 1, edge} and 64 * edge - 1 in sp and 64 * edge in sp
        for m in (em, gm):
            assert sr.members(m)[sp].all()
        assert set(sr.winner_places(w64)) <= set(sp) and len(sr.winner_places(w64)) == 3 + 2 * sum(e < w64 for e in (64, 128, 256))
    assert not sr.level_masks(8, exon_zero=True)[1].any() and sr.level_masks(8, exon_zero=True)[2].any()


def test_wide_slab_generator_keeps_its_promises():
    w64 = 264
    _, em, gm = sr.level_masks(w64)
    for lv in (0, 1):
        cases = sr.wide_slab_pairs(w64, (em, gm), lv)
        assert [c[1] for c in cases] == [(0,), (1,), (2,), (3,), (4,), (1, 3)]
        for pr, slabs, winners in cases:
            compat, off, refs = sr.assemble([pr], w64)
            count = sr.counts_of_pair(compat, refs, lv)
            assert pr.n_refs == 300 and [a >> 12 for a in winners] == list(slabs)
            per_slab = [int(count[4096 * s:4096 * (s + 1)].max()) for s in range(5)]
            assert per_slab == [300 if s in slabs else 299 - s for s in range(5)]
            assert (count == 300).sum() == len(slabs)
            assert np.array_equal(sr.classes_ref(compat, off, refs, lv, (em, gm)[lv])[0], sr.bit_row(w64, winners))


def test_ceiling_case_keeps_its_promise():
    _, em, gm = sr.level_masks(8)
    compat, off, refs, want_e, want_g = sr.ceiling_case(8, (em, gm))
    per_level = [[int(((refs[off[p]:off[p + 1]] >> 31) == lv).sum()) for lv in (0, 1)] for p in (0, 1)]
    assert per_level == [[65535, 65534], [65535, 2]] and sr.CEILING == 65535
    mem = sr.members(compat)
    a, b = mem[1], mem[2]
    assert (b & ~a).sum() == 1 and not (a & ~b).any() and (a & sr.members(em)).any() and (a & sr.members(gm)).any()
    count = sr.counts_of_pair(compat, refs[off[1]:off[2]], 0)
    assert set(count[a].tolist()) == {65535} and count[b & ~a].tolist() == [65534]
    assert np.array_equal(sr.classes_ref(compat, off, refs, 0, em), want_e) and want_e.any(axis=1).all()
    assert np.array_equal(sr.classes_ref(compat, off, refs, 1, gm), want_g) and not np.array_equal(want_g[0], want_g[1])


def test_repeat_lists_repeats_ref_lists():
    off, refs = np.array([0, 2, 2, 5], np.int32), np.array([7, 8, 1, 2, 3], np.uint32)
    o, r = sr.repeat_lists(off, refs, [2, 0, 1, 2, 1])
    assert o.tolist() == [0, 3, 5, 5, 8, 8] and r.tolist() == [1, 2, 3, 7, 8, 1, 2, 3] and r.dtype == np.uint32


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n_values", [511, 512, 513])
def test_value_edge_index_has_exactly_the_claimed_number_of_values(n_values, padded):
    for chosen in (7, 11):
        rng = np.random.RandomState(n_values + chosen)
        bits, n_alleles = sr.value_edge_bits(rng, 12, chosen, n_values, padded)
        assert bits.shape == (12, 1024) and n_alleles == (1000 if padded else 1024)
        vc = sr.value_counts(bits)
        assert vc[chosen] == n_values and np.delete(vc, chosen).max() <= 8
        assert (0 in bits[chosen]) == padded and not bits[:, n_alleles:].any()
        pl = sr.value_edge_pieces(bits, n_alleles, chosen, rng)
        pieces, masks, cut_from = pl.arrays("given")
        lo, hi = pieces["lo_word"].astype(int), pieces["lo_word"].astype(int) + pieces["n_words"].astype(int)
        covers = (lo <= chosen) & (hi > chosen)
        assert covers.any() and (~covers).any() and (lo < chosen).any() and (lo > chosen).any() == (chosen < 11)
        assert len(pieces) <= 256 and sr.window_starts(pieces) == [chosen - j for j in range(sr.WINDOW)]
        assert hi.max() <= 12 and pieces["n_words"].max() <= sr.WINDOW
        _cut_alleles_pass(bits, pieces, masks, cut_from)


def _cut_alleles_pass(bits, pieces, masks, cut_from):
    """the allele a piece was cut from passes it; a spoiled piece is not passed by its allele -- and somebody fails every cut piece"""
    mem = sr.members(sr.compat_ref(bits, pieces, masks))
    some = 0
    for p, a in enumerate(cut_from):
        if a is not None:
            assert mem[p, a]
            some += 1
    assert some


def test_piece_generators_keep_their_promises():
    rng = np.random.RandomState(3)
    for n_words, n_vars in ((1, 20), (2, 64), (7, 200), (8, 256), (9, 270), (20, 640)):
        bits = sr.low_value_bits(rng, n_words, 500, 512, n_vars)
        assert sr.value_counts(bits).max() <= 8
        if n_vars % 32:
            assert int(bits[-1].max()) < 1 << (n_vars % 32)
        pl = sr.window_edge_pieces(bits, 500, rng)
        for order in ("front", "reversed", "shuffled"):
            pieces, masks, cut_from = pl.arrays(order)
            _cut_alleles_pass(bits, pieces, masks, cut_from)
            mem = sr.members(sr.compat_ref(bits, pieces, masks))
            assert mem.all(axis=1).sum() == 3 and (~mem.any(axis=1)).sum() >= 3           # pass-all and impossible masks
        shapes = {(int(p["lo_word"]), int(p["n_words"])) for p in pl.arrays()[0]}
        want = [(0, 1), (n_words - 1, 1)]
        if n_words == 20:
            want += [(0, 7), (0, 8), (0, 9), (1, 7), (1, 8), (7, 1), (8, 1), (3, 9), (4, 8), (10, 1), (11, 1), (11, 9), (8, 12)]
        assert shapes >= set(want)
    bits = sr.low_value_bits(rng, 20, 500, 512)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        pl, wide_at = sr.counted_pieces(bits, 500, n, rng)
        pieces, masks, cut_from = pl.arrays("given")
        assert len(pieces) == n and wide_at == sorted({i for i in (0, 63, 255, n - 1) if i < n})
        assert all(pieces[i]["n_words"] == 9 for i in wide_at) and (np.delete(pieces["n_words"], wide_at) <= 5).all()
    for n_alleles in (1, 511, 512, 513, 4096, 4097, 8192, 8193, 16385):
        a_pad = (n_alleles + 511) // 512 * 512
        bits = sr.founder_bits(rng, 10, n_alleles, a_pad)
        assert sr.value_counts(bits).max() <= sr.PAT_D and not bits[:, n_alleles:].any()
        pl, cut = sr.allele_edge_pieces(bits, n_alleles, rng)
        assert {0, n_alleles - 1} <= set(cut) and ({8191, 8192} <= set(cut)) == (n_alleles > 8192)
        pieces, masks, cut_from = pl.arrays()
        _cut_alleles_pass(bits, pieces, masks, cut_from)


def test_row_hash_properties():
    rng = np.random.RandomState(5)
    rows = rng.randint(0, 256, size=(50, 64)).astype(np.uint8).view(np.uint64)
    rows[:10] = 0
    rows[20] = rows[21]
    rows[30, 2:] = 0                                            # two non-zero words ...
    rows[31] = rows[30]
    rows[31, [0, 1]] = rows[30, [1, 0]]                        # ... swapped
    rows[32] = 0
    rows[32, 7] = 1                                            # a single bit
    h = sr.row_hash_ref(rows)
    assert h.dtype == np.uint64 and h.shape == (50,)
    assert np.all(h[:10] == np.uint64(sr.EMPTY)) and not np.any(h[10:] == np.uint64(sr.EMPTY))
    assert h[20] == h[21] and h[30] != h[31]
    assert len(set(h[10:].tolist())) == 39
    assert np.array_equal(sr.row_hash_ref(rows[::-1])[::-1], h)               # a row's hash does not depend on its neighbours
    # the sum is over word_hash(word, index): one word at index i, written out
    w, i = 0x0123456789ABCDEF, 5
    x = (w + 0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64)
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 % (1 << 64)
    x ^= x >> 27; x = x * 0x94D049BB133111EB % (1 << 64)
    x ^= x >> 31
    one = np.zeros((1, 8), np.uint64)
    one[0, i] = w
    assert int(sr.row_hash_ref(one)[0]) == x
    two = one.copy()
    two[0, 0] = 1
    y = (1 + 0x9E3779B97F4A7C15) % (1 << 64)
    y ^= y >> 30; y = y * 0xBF58476D1CE4E5B9 % (1 << 64)
    y ^= y >> 27; y = y * 0x94D049BB133111EB % (1 << 64)
    y ^= y >> 31
    assert int(sr.row_hash_ref(two)[0]) == (x + y) % (1 << 64)
    # a sum equal to EMPTY becomes EMPTY - 1; only an all-zero row is EMPTY
    assert sr.finish_hash_ref(sr.EMPTY, True) == sr.EMPTY - 1 and sr.finish_hash_ref(5, False) == sr.EMPTY
    assert sr.finish_hash_ref(5, True) == 5 and sr.finish_hash_ref(sr.EMPTY - 1, True) == sr.EMPTY - 1
