"""The scoring kernels (csrc/hgx_device.hip: k_piece_compat_pat, k_pair_classes, k_pair_classes_x2, class_for_level_wide)
against the plain statements of tests/score_ref.py (pinned to the C oracle by tests/test_score_ref.py) on the structural edges
of the kernels: the counter widths chosen at 3 / 15 / 255 refs with an allele AT the counter's capacity, two pairs of different
lengths in one wavefront, pair counts around the 8 pairs of a workgroup, row widths on both sides of every 64-word slab, the
slab-wise form's maximum over slabs, the 65 535-ref ceiling, a word with exactly 511 / 512 / 513 distinct values, pieces that
fill or overhang the 8-word window, piece counts around a 64-piece group and a 256-piece workgroup, and allele counts around the
8 192 alleles of a workgroup row.  Everything goes through the C ABI on hand-built arrays; every output has two guard rows
behind it.  Bit rows and integers only: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import dedup_ref as dr
import score_ref as sr
from hisatgenotype_amd import capi, engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 2


class Index:
    """hgx_index made straight from host arrays"""

    def __init__(self, n_alleles, n_vars, bits, exon_mask, gene_mask):
        self.h = C.c_void_p()
        self.a_pad = capi.a_pad(n_alleles)
        self.w64 = self.a_pad // 64
        bits = np.ascontiguousarray(bits, np.uint32)
        assert bits.shape == (max(1, (n_vars + 31) // 32), self.a_pad)
        em, gm = np.ascontiguousarray(exon_mask, np.uint64), np.ascontiguousarray(gene_mask, np.uint64)
        assert em.shape == gm.shape == (self.w64,)
        self.masks = (em, gm)
        capi.check(capi.lib().hgx_index_create(C.byref(self.h), C.c_int32(n_alleles), C.c_int32(n_vars), capi.ptr(bits),
                                                capi.ptr(em), capi.ptr(gm)))

    def close(self):
        if self.h:
            capi.lib().hgx_index_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def mask_index():
    """get(w64, exon_zero) -> an index of 64 * w64 - 1 alleles and one variant word with score_ref.level_masks as its masks"""
    made = {}

    def get(w64, exon_zero=False):
        if (w64, exon_zero) not in made:
            n_alleles, em, gm = sr.level_masks(w64, exon_zero=exon_zero)
            made[w64, exon_zero] = Index(n_alleles, 32, np.zeros((1, 64 * w64), np.uint32), em, gm)
        return made[w64, exon_zero]
    yield get
    for ix in made.values():
        ix.close()


def _guarded(n, w64=None):
    shape = (n + GUARD,) if w64 is None else (n + GUARD, w64)
    return capi.DevArray.from_host(np.full(shape, SENTINEL, np.uint64))


def _taken(dev, n, what):
    got = dev.to_host()
    assert np.all(got[n:] == np.uint64(SENTINEL)), what + ": a guard row was written"
    return got[:n]


LEVELS = {"both": (True, True), "exon": (True, False), "gene": (False, True)}
OUTPUTS = {"rows+hashes": (True, True), "rows": (True, False), "hashes": (False, True)}


def _pair_classes(ix, compat, off, refs, levels=tuple(LEVELS), want=None):
    """hgx_pair_classes in every form -- both levels in one launch, exon only, gene only, each with rows + hashes, rows only and
    hashes only -- == classes_ref and row_hash_ref of those rows; guard rows intact.  -> the reference rows"""
    n = len(off) - 1
    w64 = ix.w64
    d_compat = capi.DevArray.from_host(np.ascontiguousarray(compat, np.uint64))
    d_off = capi.DevArray.from_host(np.ascontiguousarray(off, np.int32))
    d_refs = capi.DevArray.from_host(np.ascontiguousarray(refs if len(refs) else np.zeros(1), np.uint32))
    want_rows = [sr.classes_ref(compat, off, refs, lv, ix.masks[lv]) for lv in (0, 1)]
    if want is not None:
        for lv in (0, 1):
            assert np.array_equal(want_rows[lv], want[lv])
    want_hash = [sr.row_hash_ref(r) for r in want_rows]
    for lname in levels:
        for oname, (with_rows, with_hash) in OUTPUTS.items():
            rows = [_guarded(n, w64) if LEVELS[lname][lv] and with_rows else None for lv in (0, 1)]
            hashes = [_guarded(n) if LEVELS[lname][lv] and with_hash else None for lv in (0, 1)]
            capi.check(capi.lib().hgx_pair_classes(ix.h, capi.ptr(d_compat), capi.ptr(d_off), capi.ptr(d_refs), C.c_int32(n),
                                                   capi.ptr(rows[0]), capi.ptr(rows[1]), capi.ptr(hashes[0]), capi.ptr(hashes[1]),
                                                   None))
            capi.sync()
            for lv in (0, 1):
                what = "%s / %s, level %d" % (lname, oname, lv)
                if rows[lv] is not None:
                    got = _taken(rows[lv], n, what)
                    bad = np.flatnonzero((got != want_rows[lv]).any(axis=1))
                    assert len(bad) == 0, (what, "rows of pairs", bad.tolist(), "refs", np.diff(off)[bad].tolist())
                if hashes[lv] is not None:
                    got = _taken(hashes[lv], n, what)
                    bad = np.flatnonzero(got != want_hash[lv])
                    assert len(bad) == 0, (what, "hashes of pairs", bad.tolist(), "refs", np.diff(off)[bad].tolist())
    return want_rows


# ---- pair classes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sr.N_TOTALS)
def test_total_refs_on_both_sides_of_every_counter_width(mask_index, n):
    """Pairs of n refs in all: every ref of the level under test, every ref of the other level, n - 1 and 1; one masked allele in
    every ref of the level (at n = 3, 15, 255 it fills the counter, at 4, 16, 256 it would wrap a counter one size too small)
    and one in all but one; then the same with the full-count allele outside the mask."""
    ix = mask_index(8)
    pairs = sr.sweep_pairs(8, ix.masks, n)
    compat, off, refs = sr.assemble(pairs, 8)
    want = _pair_classes(ix, compat, off, refs)
    for p, pr in enumerate(pairs):
        assert np.array_equal(want[pr.level][p], pr.promised_class(ix.masks[pr.level]))


NEIGHBOURS = [(3, 4), (4, 3), (15, 16), (16, 15), (255, 256), (256, 255), (0, 15), (15, 0), (1, 300)]


@pytest.mark.parametrize("split", ["level", "mixed"])
@pytest.mark.parametrize("level", [0, 1])
def test_a_short_and_a_long_pair_in_one_wavefront(mask_index, level, split):
    """pairs 2k and 2k + 1 share a wavefront of the one-level kernel: the counter width is chosen for the longer of the two"""
    ix = mask_index(8)
    rng = np.random.RandomState(level)
    pairs = [sr.make_pair(rng, 8, ix.masks, level, n, split) for ab in NEIGHBOURS for n in ab]
    compat, off, refs = sr.assemble(pairs, 8)
    assert [tuple(x) for x in np.diff(off).reshape(-1, 2).tolist()] == NEIGHBOURS
    _pair_classes(ix, compat, off, refs)


PAIR_TOTALS = [3, 4, 1, 0, 15, 16, 2, 5, 14, 17, 3, 0, 4, 255, 1, 256, 6]


@pytest.mark.parametrize("n_pairs", [1, 2, 7, 8, 9, 15, 16, 17])
def test_pair_counts_around_a_workgroup(mask_index, n_pairs):
    """4 pairs per workgroup in the two-level kernel, 8 in the one-level kernel; an odd count leaves the last wavefront of the
    latter without a second pair; the last pair differs from its neighbour"""
    ix = mask_index(8)
    rng = np.random.RandomState(n_pairs)
    pairs = [sr.make_pair(rng, 8, ix.masks, p & 1, PAIR_TOTALS[p], "mixed", x_masked=p % 3 != 2) for p in range(n_pairs)]
    compat, off, refs = sr.assemble(pairs, 8)
    want = _pair_classes(ix, compat, off, refs)
    if n_pairs > 1:
        assert not np.array_equal(want[0][-1], want[0][-2]) and not np.array_equal(want[1][-1], want[1][-2])


WIDTHS = [8, 64, 72, 128, 136, 256, 264, 512]
WIDTH_TOTALS = (2, 5, 20, 260)         # one per counter form


@pytest.mark.parametrize("w64", WIDTHS)
def test_row_widths_on_both_sides_of_every_slab(mask_index, w64):
    """n_alleles = 64 * w64 - 1.  The winning allele at bit 0 of word 0, at the last allele, at bit 63 of the word before the last,
    in the last word of a 64-word slab and in the first of the next -- under each counter form (2, 4, 8 planes, slab-wise)."""
    ix = mask_index(w64)
    rng = np.random.RandomState(w64)
    pairs = [sr.make_pair(rng, w64, ix.masks, (i + k) & 1, n, "mixed", x=x)
             for i, x in enumerate(sr.winner_places(w64)) for k, n in enumerate(WIDTH_TOTALS)]
    compat, off, refs = sr.assemble(pairs, w64)
    want = _pair_classes(ix, compat, off, refs)
    for p, pr in enumerate(pairs):
        assert np.array_equal(want[pr.level][p], sr.bit_row(w64, [pr.x]))


def test_more_than_32768_alleles_are_refused_on_the_host():
    n_alleles = 32769
    a_pad = capi.a_pad(n_alleles)
    w64 = a_pad // 64
    assert w64 == 520
    ix = Index(n_alleles, 32, np.zeros((1, a_pad), np.uint32), np.zeros(w64, np.uint64), np.zeros(w64, np.uint64))
    try:
        d_compat = capi.DevArray.from_host(np.zeros((2, w64), np.uint64))
        d_off = capi.DevArray.from_host(np.array([0, 1], np.int32))
        d_refs = capi.DevArray.from_host(np.array([1], np.uint32))
        for exon, gene in LEVELS.values():
            rows, hashes = [_guarded(1, w64), _guarded(1, w64)], [_guarded(1), _guarded(1)]
            with pytest.raises(capi.HgxError) as e:
                capi.check(capi.lib().hgx_pair_classes(ix.h, capi.ptr(d_compat), capi.ptr(d_off), capi.ptr(d_refs), C.c_int32(1),
                                                       capi.ptr(rows[0]) if exon else None, capi.ptr(rows[1]) if gene else None,
                                                       capi.ptr(hashes[0]) if exon else None, capi.ptr(hashes[1]) if gene else None,
                                                       None))
            assert e.value.code == -1 and "more than 32768 alleles per locus are not supported (a_pad=33280)" in str(e.value)
            capi.sync()
            for d in rows + hashes:
                assert np.all(d.to_host() == np.uint64(SENTINEL))
    finally:
        ix.close()


@pytest.mark.parametrize("level", [0, 1])
def test_slab_wise_form_takes_the_maximum_over_all_slabs(mask_index, level):
    """300 refs at w64 = 264 (five slabs): the largest count only in slab 0, 1, 2, 3, 4 in turn with smaller non-zero counts in
    every other slab, and in two slabs at once"""
    ix = mask_index(264)
    cases = sr.wide_slab_pairs(264, ix.masks, level)
    compat, off, refs = sr.assemble([c[0] for c in cases], 264)
    want = _pair_classes(ix, compat, off, refs)
    for p, (_, _, winners) in enumerate(cases):
        assert np.array_equal(want[level][p], sr.bit_row(264, winners))


@pytest.mark.parametrize("levels", sorted(LEVELS))
def test_the_ceiling_of_65535_refs_per_pair_and_level(mask_index, levels):
    """every one of the 16 counter planes set; an allele one below must lose"""
    ix = mask_index(8)
    compat, off, refs, want_e, want_g = sr.ceiling_case(8, ix.masks)
    _pair_classes(ix, compat, off, refs, levels=(levels,), want=(want_e, want_g))


def test_an_index_whose_exon_mask_is_all_zero(mask_index):
    """every exon row is zero and every exon hash EMPTY; the gene rows are what they are with any other exon mask"""
    ix = mask_index(8, exon_zero=True)
    other = mask_index(8)
    assert not ix.masks[0].any() and np.array_equal(ix.masks[1], other.masks[1])
    rng = np.random.RandomState(9)
    pairs = [sr.make_pair(rng, 8, other.masks, p & 1, n, "mixed") for p, n in enumerate((0, 1, 2, 3, 4, 15, 16, 40, 255, 256, 300))]
    compat, off, refs = sr.assemble(pairs, 8)
    want = _pair_classes(ix, compat, off, refs)
    assert not want[0].any() and np.all(sr.row_hash_ref(want[0]) == np.uint64(sr.EMPTY))
    assert np.array_equal(want[1], sr.classes_ref(compat, off, refs, 1, other.masks[1])) and want[1].any(axis=1).all()


@pytest.mark.parametrize("level", [0, 1])
def test_level_classes_on_repeated_ref_lists(mask_index, level):
    """hgx_level_classes (one row per distinct ref list, chosen through a selection) on 41 pairs drawn from 17 lists on both
    sides of every counter width == dedup_ref(classes_ref): bits, pair counts, first pairs, order"""
    ix = mask_index(8)
    rng = np.random.RandomState(level + 20)
    totals = (4, 1, 2, 16, 3, 5, 256, 16, 17, 255, 0, 300, 3, 14, 0, 15, 1)        # every third has all its refs at the level
    pairs = [sr.make_pair(rng, 8, ix.masks, level, n, ("level", "mixed", "other")[p % 3], x_masked=p % 4 != 1)
             for p, n in enumerate(totals)]
    assert {pr.n_lv for pr in pairs if pr.x_masked} >= {3, 4, 15, 16, 256}
    compat, off, refs = sr.assemble(pairs, 8)
    # (the 4-ref list and the 1-ref list come first: if rows are made in first-seen order of the lists they share a wavefront)
    pick = np.concatenate([[0, 0, 1], rng.permutation(len(totals)), rng.randint(0, len(totals), 21)]).tolist()
    off, refs = sr.repeat_lists(off, refs, pick)
    n = len(pick)
    assert n == 41
    want_b, want_c, want_f = dr.dedup_ref(sr.classes_ref(compat, off, refs, level, ix.masks[level]))
    assert 1 < len(want_c) < n and want_c.max() > 1
    d_compat, d_off, d_refs = capi.DevArray.from_host(compat), capi.DevArray.from_host(off), capi.DevArray.from_host(refs)
    for scratch in (False, True):
        rows, hashes = (_guarded(n, 8), _guarded(n)) if scratch else (None, None)
        h = C.c_void_p()
        capi.check(capi.lib().hgx_level_classes(C.byref(h), ix.h, capi.ptr(d_compat), capi.ptr(d_off), capi.ptr(d_refs), C.c_int32(n),
                                                C.c_int32(level), capi.ptr(rows), capi.ptr(hashes), None))
        cl = engine.Classes(h)
        got_b, got_c, got_f = cl.to_host()
        assert cl.n_classes == len(want_c)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c) and np.array_equal(got_f, want_f)
        cl.close()
        if scratch:
            capi.sync()
            _taken(rows, n, "row scratch")
            _taken(hashes, n, "hash scratch")


# ---- piece compat ------------------------------------------------------------------------------------------------------------------

def _piece_compat(ix, bits, pieces, masks):
    """hgx_piece_compat == compat_ref over all a_pad columns; guard rows intact"""
    n = len(pieces)
    want = sr.compat_ref(bits, pieces, masks)
    d_pieces, d_masks = capi.DevArray.from_host(pieces), capi.DevArray.from_host(masks)
    out = _guarded(n, ix.w64)
    capi.check(capi.lib().hgx_piece_compat(ix.h, capi.ptr(d_pieces), capi.ptr(d_masks), C.c_int32(n), capi.ptr(out), None))
    capi.sync()
    got = _taken(out, n, "compat")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, ("pieces", bad.tolist()[:20], [(int(pieces[p]["lo_word"]), int(pieces[p]["n_words"])) for p in bad[:20]])


def _bits_index(bits, n_alleles, n_vars=None):
    zero = np.zeros(bits.shape[1] // 64, np.uint64)
    return Index(n_alleles, 32 * bits.shape[0] if n_vars is None else n_vars, bits, zero, zero)


@pytest.mark.parametrize("chosen", [7, 11])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n_values", [511, 512, 513])
def test_a_word_with_exactly_511_512_513_values(n_values, padded, chosen):
    """An index of 12 words; one word -- the 8th, or the index's last -- has exactly that many distinct values over its a_pad
    columns (HGX_PAT_D = 512 is the most the pattern form takes), with the padding's 0 among them or without padding; it stands
    at each of the positions 0..7 of a window, under pieces that start before it, at it and after it."""
    rng = np.random.RandomState(n_values + chosen)
    bits, n_alleles = sr.value_edge_bits(rng, 12, chosen, n_values, padded)
    pieces, masks, _ = sr.value_edge_pieces(bits, n_alleles, chosen, rng).arrays("given")
    ix = _bits_index(bits, n_alleles)
    try:
        _piece_compat(ix, bits, pieces, masks)
        for order in ("front", "reversed"):
            pieces, masks, _ = sr.value_edge_pieces(bits, n_alleles, chosen, rng).arrays(order)
            _piece_compat(ix, bits, pieces, masks)
    finally:
        ix.close()


@pytest.mark.parametrize("n_words,n_vars", [(1, 20), (2, 64), (7, 200), (8, 256), (9, 270), (20, 640), (20, 613)])
def test_pieces_that_fill_or_overhang_the_window(n_words, n_vars):
    """pieces of 1, 7, 8, 9 words from a window's first word, 7 and 8 from its second, one word on its 8th and 9th, pieces ending on
    the index's last word, masks that pass everything and masks nothing passes -- in the front end's order, reversed and shuffled,
    on indices of fewer words than a window, exactly a window, and more"""
    rng = np.random.RandomState(n_vars)
    bits = sr.low_value_bits(rng, n_words, 500, 512, n_vars)
    pl = sr.window_edge_pieces(bits, 500, rng)
    ix = _bits_index(bits, 500, n_vars)
    try:
        for order in ("front", "reversed", "shuffled"):
            pieces, masks, _ = pl.arrays(order)
            _piece_compat(ix, bits, pieces, masks)
    finally:
        ix.close()


@pytest.fixture(scope="module")
def counted_index():
    rng = np.random.RandomState(77)
    bits = sr.low_value_bits(rng, 20, 1000, 1024, 640)
    ix = _bits_index(bits, 1000)
    yield ix, bits
    ix.close()


@pytest.mark.parametrize("n_pieces", [1, 63, 64, 65, 255, 256, 257, 513])
def test_piece_counts_around_a_group_and_a_workgroup(counted_index, n_pieces):
    """64 pieces per group, 256 per workgroup; a 9-word piece (straight from the index) as the first, the 64th, the 256th and the
    last of the list"""
    ix, bits = counted_index
    pl, _ = sr.counted_pieces(bits, 1000, n_pieces, np.random.RandomState(n_pieces))
    pieces, masks, _ = pl.arrays("given")
    _piece_compat(ix, bits, pieces, masks)


@pytest.mark.parametrize("n_alleles", [1, 511, 512, 513, 4096, 4097, 8192, 8193, 16385])
def test_allele_counts_around_a_workgroup_row(n_alleles):
    """a_pad 512 (one wavefront), 1024, 4096, 4608, 8192 (one full workgroup), 8704 and 16896 (a second and a third workgroup row)
    on founder-like bits, so the pattern path runs in every workgroup row; masks cut from alleles of the first and the last
    64-allele word and of each side of allele 8192"""
    rng = np.random.RandomState(n_alleles)
    a_pad = capi.a_pad(n_alleles)
    bits = sr.founder_bits(rng, 10, n_alleles, a_pad)
    pl, _ = sr.allele_edge_pieces(bits, n_alleles, rng)
    ix = _bits_index(bits, n_alleles)
    try:
        for order in ("front", "shuffled"):
            pieces, masks, _ = pl.arrays(order)
            _piece_compat(ix, bits, pieces, masks)
    finally:
        ix.close()
