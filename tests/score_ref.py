"""Plain statements of the scoring stage -- piece x allele compatibility, the per-pair arg-max classes and the row hash -- and
the inputs that put its kernels (csrc/hgx_device.hip) on their structural edges (TEST INFRASTRUCTURE: numpy and Python ints,
no GPU, no torch).

`compat_ref`, `classes_ref` and `row_hash_ref` are the contracts of hgx_piece_compat and hgx_pair_classes as include/hgx.h
states them.  tests/test_score_ref.py pins them to the C oracle and to hand-worked cases before tests/test_gpu_score_edges.py
lets them judge a kernel.  Every generator returns its inputs together with what its construction promises; the promises are
checked under the statements by tests/test_score_ref.py.
"""
import numpy as np

EMPTY = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1
PAT_D = 512                      # HGX_PAT_D: most distinct values of a variant word the pattern form of the compat kernel takes
WINDOW = 8                       # PP_W = PP_NW: variant words per window / widest piece of the pattern form
PIECE_DTYPE = np.dtype([("mask_off", np.uint32), ("lo_word", np.uint16), ("n_words", np.uint16)])      # hgx_piece


# ---- statements -------------------------------------------------------------------------------------------------------------------

def pack(member):
    """[..][64 * w64] bool -> [..][w64] uint64, allele a at bit a & 63 of word a >> 6"""
    return np.ascontiguousarray(np.packbits(np.asarray(member, bool), axis=-1, bitorder="little")).view(np.uint64)


def members(rows):
    """[..][w64] uint64 -> [..][64 * w64] bool"""
    rows = np.ascontiguousarray(rows, np.uint64)
    return np.unpackbits(rows.view(np.uint8), axis=-1, bitorder="little").astype(bool)


def compat_ref(bits, pieces, masks):
    """compat[p][a] <=> for every word i of piece p: (bits[lo + i][a] & MP_i) == P_i, over all a_pad columns."""
    bits = np.asarray(bits, np.uint32)
    masks = np.asarray(masks, np.uint32)
    a_pad = bits.shape[1]
    ok = np.ones((len(pieces), a_pad), bool)
    for p in range(len(pieces)):
        mo, lo, nw = int(pieces[p]["mask_off"]), int(pieces[p]["lo_word"]), int(pieces[p]["n_words"])
        for i in range(nw):
            ok[p] &= (bits[lo + i] & masks[mo + 2 * i]) == masks[mo + 2 * i + 1]
    return pack(ok).reshape(len(pieces), a_pad // 64)


def counts_of_pair(compat, refs, level):
    """count[a] = the number of refs of `level` whose compat row holds a (a ref that occurs twice counts twice): int64 sums"""
    refs = np.asarray(refs, np.uint32).astype(np.int64)
    rows = refs[(refs >> 31) == level] & 0x7FFFFFFF
    count = np.zeros(64 * compat.shape[1], np.int64)
    if len(rows):
        used, times = np.unique(rows, return_counts=True)
        for r0 in range(0, len(used), 64):
            count += times[r0:r0 + 64].astype(np.int64) @ members(compat[used[r0:r0 + 64]]).astype(np.int64)
    return count


def classes_ref(compat, pair_off, refs, level, mask):
    """class of a pair = {a under mask : count[a] == max over the alleles under mask} -- `mask` itself when the pair has no ref
    of the level or no allele under the mask is in any of its rows."""
    compat = np.ascontiguousarray(compat, np.uint64)
    w64 = compat.shape[1]
    under = members(np.asarray(mask, np.uint64))
    out = np.zeros((len(pair_off) - 1, w64), np.uint64)
    if not under.any():
        return out
    for p in range(len(pair_off) - 1):
        count = counts_of_pair(compat, refs[int(pair_off[p]):int(pair_off[p + 1])], level)
        out[p] = pack(under & (count == count[under].max()))
    return out


def _mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def row_hash_py(row):
    """One row in Python ints: sum mod 2^64 over the non-zero words of mix64(word + golden * (index + 1)); an all-zero row is
    EMPTY, a sum equal to EMPTY becomes EMPTY - 1 (word_hash / finish_hash, csrc/hgx_common.hpp)."""
    words = [int(w) for w in row]
    if not any(words):
        return EMPTY
    h = sum(_mix64((w + 0x9E3779B97F4A7C15 * (i + 1)) & M64) for i, w in enumerate(words) if w) & M64
    return EMPTY - 1 if h == EMPTY else h


def finish_hash_ref(h, nonzero):
    return EMPTY if not nonzero else (EMPTY - 1 if h == EMPTY else h)


def row_hash_ref(rows):
    rows = np.ascontiguousarray(rows, np.uint64)
    return np.array([row_hash_py(r) for r in rows.tolist()], np.uint64)


# ---- masks and small helpers ----------------------------------------------------------------------------------------------------------

def bit_row(w64, alleles):
    r = np.zeros(w64, np.uint64)
    for a in alleles:
        r[a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    return r


def special_alleles(w64):
    """the places a row kernel can drop: bit 0 of word 0, the last allele (n_alleles = 64 * w64 - 1), bit 63 of the word before
    the last, and both sides of every 64-word slab edge"""
    n_alleles = 64 * w64 - 1
    s = [0, n_alleles - 1, 64 * (w64 - 2) + 63]
    for edge in (64, 128, 256):
        if edge < w64:
            s += [64 * (edge - 1) + 63, 64 * (edge - 1) + 17, 64 * edge, 64 * edge + 40]
    return sorted(set(s))


def winner_places(w64):
    """of the special alleles: bit 0 of word 0, bit 63 of the last word that has one, the last allele, bit 63 of the last word of
    every slab and bit 0 of the first word of the next"""
    s = [0, 64 * (w64 - 2) + 63, 64 * w64 - 2]
    for edge in (64, 128, 256):
        if edge < w64:
            s += [64 * edge - 1, 64 * edge]
    return sorted(set(s))


def level_masks(w64, seed=0, exon_zero=False):
    """-> (n_alleles, exon mask, gene mask): n_alleles = 64 * w64 - 1, so the last bit is padding and under no mask; the masks are
    random halves (a quarter of the alleles under neither, a quarter under both), different from one another; the special
    alleles are under both, their upper neighbours under neither."""
    rng = np.random.RandomState(1000 + w64 + seed)
    n_alleles = 64 * w64 - 1
    m = rng.rand(2, 64 * w64) < 0.5
    sp = np.array(special_alleles(w64))
    m[:, sp] = True
    m[:, [a + 1 for a in sp.tolist() if a + 1 not in set(sp.tolist())]] = False
    m[:, n_alleles:] = False
    if exon_zero:
        m[0] = False
    return n_alleles, pack(m[0]), pack(m[1])


def alleles_under(mask, words=None):
    """allele ids under `mask` (in the given 64-allele words only), ascending"""
    a = np.flatnonzero(members(np.asarray(mask, np.uint64)))
    if words is not None:
        a = a[np.isin(a >> 6, np.asarray(list(words)))]
    return a


# ---- pair classes: one pair with a promised winner ------------------------------------------------------------------------------------

SPLITS = ("level", "other", "mixed")
N_TOTALS = (0, 1, 2, 3, 4, 5, 14, 15, 16, 17, 63, 64, 65, 254, 255, 256, 257, 300)


class Pair:
    """The compat rows of one pair (its refs point into them in order) and what the construction promises at `level`."""

    def __init__(self, rows, ref_level, level, x, y, n_lv, x_masked):
        self.rows, self.ref_level, self.level = rows, np.asarray(ref_level, np.uint32), level
        self.x, self.y, self.n_lv, self.x_masked = x, y, n_lv, x_masked

    @property
    def n_refs(self):
        return len(self.ref_level)

    def promised_class(self, mask):
        """x is in all n_lv refs of the level, y in n_lv - 1, every other allele in at most n_lv - 2: the class is {x} when x is
        under the mask, {y} when it is not and y has a count at all, the mask itself when no masked allele is counted."""
        w64 = len(mask)
        if self.x_masked and self.n_lv >= 1:
            return bit_row(w64, [self.x])
        if not self.x_masked and self.n_lv >= 2:
            return bit_row(w64, [self.y])
        return np.asarray(mask, np.uint64).copy()


def split_counts(n, split):
    """-> (refs of the level under test, refs of the other level) of a pair with n refs in all"""
    if split == "level" or n == 0:
        return n, 0
    if split == "other":
        return 0, n
    return n - 1, 1


def random_members(rng, n, w64):
    """[n][64 * w64] bool, every bit set with p = 0.25"""
    a = np.frombuffer(rng.bytes(n * 8 * w64), np.uint8) & np.frombuffer(rng.bytes(n * 8 * w64), np.uint8)
    return np.unpackbits(a.reshape(n, 8 * w64), axis=1).astype(bool)


def make_pair(rng, w64, masks, level, n, split="level", x_masked=True, x=None):
    """A pair of n refs, n_lv of them of `level` (split_counts).  Of the level's rows every one holds x, all but one hold y; the
    other alleles are in none of two chosen rows, so they count at most n_lv - 2.  The other level's rows hold y, a decoy z
    under the mask and random alleles: counted by mistake they change the class.  x is under the mask or, `x_masked` False,
    under neither mask (the arg-max is taken over masked alleles only); y and z are under the mask."""
    mask = np.asarray(masks[level], np.uint64)
    under = alleles_under(mask)
    neither = np.flatnonzero(~members(np.asarray(masks[0], np.uint64) | np.asarray(masks[1], np.uint64))[:64 * w64 - 1])
    n_lv, n_other = split_counts(n, split)
    if x is None:
        x = int(under[rng.randint(len(under))]) if x_masked else int(neither[rng.randint(len(neither))])
    y, z = [int(a) for a in rng.choice(under[under != x], 2, replace=False)]
    rows = random_members(rng, n, w64)
    rows[:, [x, y, z]] = False
    lv = np.full(n, 1 - level, np.uint32)
    at = rng.permutation(n)[:n_lv]                                # where the level's refs stand among the pair's refs
    lv[at] = level
    if n_lv:
        rows[at, x] = True
        rows[at[1:], y] = True                                    # y misses the row at[0]
        rows[at[:2]] = False                                      # the others miss two rows ...
        rows[at[:2], x] = True                                    # ... which x does not
        if n_lv >= 2:
            rows[at[1], y] = True
    oth = np.flatnonzero(lv != level)
    rows[oth, y] = True
    rows[oth, z] = True
    rows[:, 64 * w64 - 1] = False                                 # compat rows may hold padding bits; these do not
    return Pair(pack(rows).reshape(n, w64), lv, level, x, y, n_lv, x_masked)


def assemble(pairs, w64):
    """-> (compat [n_rows][w64], pair_off int32, refs uint32): the pairs' rows one after the other (one spare row in front, so
    that no ref is 0 by accident), every ref = row | level << 31"""
    rows, refs, off = [np.zeros((1, w64), np.uint64)], [], [0]
    base = 1
    for p in pairs:
        rows.append(p.rows)
        refs.append((np.arange(base, base + p.n_refs).astype(np.uint32)) | (p.ref_level << np.uint32(31)))
        base += p.n_refs
        off.append(off[-1] + p.n_refs)
    refs = np.concatenate(refs).astype(np.uint32) if refs else np.zeros(0, np.uint32)
    return np.ascontiguousarray(np.concatenate(rows)), np.array(off, np.int32), refs


def sweep_pairs(w64, masks, n, seed=0):
    """the pairs of one total n: three splits x the winner under / outside the mask x either level under test"""
    rng = np.random.RandomState(7 * n + w64 + seed)
    return [make_pair(rng, w64, masks, lv, n, sp, xm) for lv in (0, 1) for sp in SPLITS for xm in (True, False)]


def wide_slab_pairs(w64, masks, level, n=300, seed=0):
    """The slab-wise form's maximum over the slabs of 64 words: per case the largest count (n) is held only by an allele of ONE
    slab -- each slab in turn -- and every other slab holds an allele with a smaller non-zero count (n - 1 - slab) and nothing
    larger; a last case has the largest count in slabs 1 and 3 at once.  -> [(pair, slabs of the winners, the winners)]"""
    rng = np.random.RandomState(w64 + seed)
    n_slabs = (w64 + 63) // 64
    mask = masks[level]
    pick = [int(alleles_under(mask, range(64 * s, min(64 * s + 64, w64)))[3 + s]) for s in range(n_slabs)]
    out = []
    for winners in [(s,) for s in range(n_slabs)] + [(1, 3)]:
        rows = np.zeros((n, 64 * w64), bool)
        for s in range(n_slabs):
            rows[:, pick[s]] = True
            if s not in winners:
                rows[:1 + s, pick[s]] = False                     # count n - 1 - s
        pr = Pair(pack(rows).reshape(n, w64), np.full(n, level, np.uint32), level, pick[winners[0]], None, n, True)
        out.append((pr, winners, [pick[s] for s in winners]))
    return out


CEILING = 65535                   # refs per pair and level (include/hgx.h); the batch builders refuse more


def ceiling_case(w64, masks, seed=0):
    """-> (compat, pair_off, refs, promised exon rows, promised gene rows).  Row A holds random alleles, row B = A and one more
    allele z under both masks.  Pair 0: CEILING exon refs, all to A, and beside them CEILING - 1 gene refs to B: the exon class
    is A under the exon mask, the gene class B under the gene mask.  Pair 1: CEILING - 1 exon refs to B and one to A -- A's
    alleles stand at CEILING (every counter bit set), z one below -- and two gene refs to A: both classes are A under the mask."""
    rng = np.random.RandomState(w64 + seed)
    a = random_members(rng, 1, w64)[0]
    a[64 * w64 - 1] = False
    z = int(alleles_under(np.asarray(masks[0], np.uint64) & np.asarray(masks[1], np.uint64) & ~pack(a))[5])
    b = a.copy()
    b[z] = True
    compat = np.stack([np.zeros(w64, np.uint64), pack(a), pack(b)])
    E, G = np.uint32(0), np.uint32(1 << 31)
    p0 = np.concatenate([np.full(CEILING, 1 | E, np.uint32), np.full(CEILING - 1, 2 | G, np.uint32)])
    p1 = np.concatenate([np.full(CEILING - 1, 2 | E, np.uint32), np.array([1 | E, 1 | G, 1 | G], np.uint32)])
    off = np.array([0, len(p0), len(p0) + len(p1)], np.int32)
    em, gm = np.asarray(masks[0], np.uint64), np.asarray(masks[1], np.uint64)
    return compat, off, np.concatenate([p0, p1]), np.stack([compat[1] & em, compat[1] & em]), np.stack([compat[2] & gm, compat[1] & gm])


def repeat_lists(off, refs, pick):
    """the batch whose pair i carries the ref list of pair pick[i] of (off, refs)"""
    lists = [refs[int(off[p]):int(off[p + 1])] for p in pick]
    new_off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    return new_off, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.uint32)


# ---- piece compat: indices and piece lists---------------------------------------------------------------------------------------------

def value_counts(bits):
    """distinct values per variant word over all a_pad columns (the padding's 0 counts)"""
    return np.array([len(np.unique(r)) for r in np.asarray(bits, np.uint32)], np.int64)


def low_value_bits(rng, n_words, n_alleles, a_pad, n_vars=None, n_values=8):
    """an index whose every word has at most `n_values` distinct values (padding 0 included)"""
    per_word = n_values - (1 if a_pad > n_alleles else 0)
    vals = rng.randint(1, 1 << 32, size=(n_words, per_word), dtype=np.uint64).astype(np.uint32)
    bits = np.zeros((n_words, a_pad), np.uint32)
    bits[:, :n_alleles] = np.take_along_axis(vals, rng.randint(0, per_word, size=(n_words, n_alleles)), axis=1)
    if n_vars is not None and n_vars % 32:
        bits[-1] &= np.uint32((1 << (n_vars % 32)) - 1)
    return bits


def value_edge_bits(rng, n_words, chosen, n_values, padded):
    """-> (bits [n_words][1024], n_alleles): word `chosen` has exactly n_values distinct values over its 1024 columns -- with
    padding (n_alleles = 1000) the padding's 0 is one of them, without (n_alleles = 1024) 0 is not a value; every other word
    has at most 8."""
    a_pad = 1024
    n_alleles = 1000 if padded else 1024
    bits = low_value_bits(rng, n_words, n_alleles, a_pad)
    k = n_values - (1 if padded else 0)
    vals = (rng.permutation(1 << 20)[:k].astype(np.uint32) + np.uint32(1)) * np.uint32(2049)        # distinct, non-zero, bits all over the word
    assert len(np.unique(vals)) == k and vals.min() > 0
    col = np.concatenate([np.arange(k), rng.randint(0, k, n_alleles - k)])
    bits[chosen, :n_alleles] = vals[rng.permutation(col)]
    return bits, n_alleles


def founder_bits(rng, n_words, n_alleles, a_pad, n_founders=150):
    """alleles copy a few founders and carry a few private variants, as real loci do: at most PAT_D values per word"""
    f = rng.randint(0, 1 << 32, size=(n_words, n_founders), dtype=np.uint64).astype(np.uint32) & \
        rng.randint(0, 1 << 32, size=(n_words, n_founders), dtype=np.uint64).astype(np.uint32)
    bits = np.zeros((n_words, a_pad), np.uint32)
    bits[:, :n_alleles] = f[:, rng.randint(0, n_founders, n_alleles)]
    flip = rng.rand(n_words, n_alleles) < min(0.02, 200.0 / n_alleles)
    bits[:, :n_alleles] ^= (flip * (1 << rng.randint(0, 32, size=(n_words, n_alleles)))).astype(np.uint32)
    return bits


class PieceList:
    """pieces + masks under construction; a piece's masks are cut from an allele (so that allele passes) or given"""

    def __init__(self, bits, rng):
        self.bits, self.rng = np.asarray(bits, np.uint32), rng
        self.pieces, self.masks, self.cut_from = [], [], []

    def cut(self, lo, nw, allele, spoil=False):
        """MP random, P = the allele's bits under MP; `spoil` flips one bit of one P under its MP: the allele itself fails"""
        assert 0 <= lo and nw >= 1 and lo + nw <= self.bits.shape[0]
        self.pieces.append((len(self.masks), lo, nw))
        self.cut_from.append(None if spoil else allele)
        bad = int(self.rng.randint(nw)) if spoil else -1
        for i in range(nw):
            mp = int(self.rng.randint(0, 1 << 32, dtype=np.uint64)) | (1 << int(self.rng.randint(32)))
            pw = int(self.bits[lo + i, allele]) & mp
            if i == bad:
                pw ^= mp & -mp
            self.masks += [mp, pw]

    def fixed(self, lo, nw, mp, pw):
        self.pieces.append((len(self.masks), lo, nw))
        self.cut_from.append(None)
        self.masks += [mp, pw] * nw

    def arrays(self, order="front"):
        """order: `front` = the front end's (by first word, then width), `reversed`, `shuffled`, `given`"""
        pieces = np.array(self.pieces, PIECE_DTYPE) if self.pieces else np.zeros(0, PIECE_DTYPE)
        idx = np.arange(len(pieces))
        if order != "given":
            idx = np.lexsort((pieces["n_words"], pieces["lo_word"]))
            if order == "reversed":
                idx = idx[::-1]
            elif order == "shuffled":
                idx = np.random.RandomState(len(pieces)).permutation(len(pieces))
        return np.ascontiguousarray(pieces[idx]), np.array(self.masks, np.uint32), [self.cut_from[i] for i in idx.tolist()]


def window_starts(pieces):
    """First words of the windows the pattern form opens over a piece list (one workgroup's share, at most 256 pieces): a window
    opens on the first word of the next piece and takes the pieces behind it while they start at or above that word, are no
    wider than WINDOW and end inside it.  (A model of the kernel's rule, used only to check where a generator puts a word.)"""
    lo, nw = pieces["lo_word"].astype(int), pieces["n_words"].astype(int)
    out, cur = [], 0
    while cur < len(lo):
        out.append(int(lo[cur]))
        end = cur + 1
        while nw[cur] <= WINDOW and end < len(lo) and lo[end] >= lo[cur] and nw[end] <= WINDOW and lo[end] + nw[end] - lo[cur] <= WINDOW:
            end += 1
        cur = end
    return out


def value_edge_pieces(bits, n_alleles, chosen, rng):
    """The chosen word at each of the positions 0..7 of a window: group j opens with a one-word piece on word chosen - j -- it
    starts below the window before it, so a new window begins there -- followed by pieces inside that window that start
    before the chosen word and cover it, start before and stop short of it, start at it, and start after it.  Order `given`."""
    pl = PieceList(bits, rng)
    n_words = bits.shape[0]
    for j in range(WINDOW):
        w0 = chosen - j
        a = lambda: int(rng.randint(n_alleles))
        pl.cut(w0, 1, a())
        if j:
            pl.cut(w0, j + 1, a())                                    # from the window's first word up to the chosen one
            pl.cut(w0, j, a())                                        # ... and stopping one short of it
        pl.cut(chosen, 1, a())
        pl.cut(chosen, 1, a(), spoil=True)
        if chosen + 1 < n_words and j < WINDOW - 1:
            pl.cut(chosen, 2, a())
            pl.cut(chosen + 1, 1, a())                                # after it
        if j and chosen + 1 < n_words and j < WINDOW - 1:
            pl.cut(chosen - 1, 3, a())                                # across it
    return pl


def window_edge_pieces(bits, n_alleles, rng):
    """On an index of n_words: for a window opened on word w0 (0 and 3) pieces of 1, 7, 8 and 9 words from its first word, of 7
    and 8 words from its second (one fits, one overhangs by one), one-word pieces on its 8th and 9th word, pieces that end on
    the index's last word, masks that pass everything and masks nothing can pass -- as far as the index has the words."""
    pl = PieceList(bits, rng)
    n_words = bits.shape[0]
    shapes = []
    for w0 in (0, 3):
        shapes += [(w0, 1), (w0, 7), (w0, 8), (w0, 9), (w0 + 1, 7), (w0 + 1, 8), (w0 + 7, 1), (w0 + 8, 1)]
    shapes += [(n_words - nw, nw) for nw in (1, 2, 7, 8, 9, 12)]
    for lo, nw in shapes:
        if lo >= 0 and lo + nw <= n_words:
            pl.cut(lo, nw, int(rng.randint(n_alleles)))
            pl.cut(lo, nw, int(rng.randint(n_alleles)), spoil=True)
    for lo, nw in ((0, 1), (0, n_words if n_words <= 9 else 8), (n_words - 1, 1)):
        pl.fixed(lo, nw, 0, 0)                                        # passes everything
        pl.fixed(lo, nw, 0x0000FFFF, 0x00010001)                      # a P bit outside MP: nothing passes
    return pl


def counted_pieces(bits, n_alleles, n_pieces, rng):
    """n_pieces narrow pieces (1..5 words) in the front end's order with a 9-word piece as the first, the 64th, the 256th and the
    last of the list.  Order `given`."""
    n_words = bits.shape[0]
    shapes = []
    for _ in range(n_pieces):
        nw = int(rng.randint(1, 6))
        shapes.append((int(rng.randint(0, n_words - nw + 1)), nw))
    shapes.sort()
    wide_at = sorted({i for i in (0, 63, 255, n_pieces - 1) if i < n_pieces})
    for i in wide_at:
        shapes[i] = (int(rng.randint(0, n_words - 9 + 1)), 9)
    pl = PieceList(bits, rng)
    for lo, nw in shapes:
        pl.cut(lo, nw, int(rng.randint(n_alleles)), spoil=rng.rand() < 0.05)
    return pl, wide_at


def allele_edge_pieces(bits, n_alleles, rng):
    """masks cut from alleles of the first and of the last 64-allele word and from each side of allele 8192 (the second
    workgroup row of the compat kernel), at widths up to the window and one beyond"""
    n_words = bits.shape[0]
    cut = sorted({a for a in (0, 63, n_alleles - 1, n_alleles - 1 - (n_alleles - 1) % 64, 8191, 8192) if 0 <= a < n_alleles})
    pl = PieceList(bits, rng)
    for a in cut:
        for nw in (1, 3, 8, 9):
            if nw <= n_words:
                pl.cut(int(rng.randint(0, n_words - nw + 1)), nw, a)
    return pl, cut
