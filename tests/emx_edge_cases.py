"""The cases of tests/test_gpu_emx_edges.py: the reference-order EM k_emx (csrc/hgx_emx.hip) at its structural edges (TEST
INFRASTRUCTURE: numpy only).  tests/test_emx_edge_ref.py checks every case's premises on the CPU and the seeds in the table were
found by searching there; no case is filtered at run time.

A case is an `XCase`: a problem of tests/em_edge_cases.py (`base`, built by em_edge_cases.build: edge alleles strong, edge classes
counted 20 x), a NAME RANK on top of it (a permutation of the allele ids, what Classes.set_allele_rank takes) and, for three
families, something added to the built problem (`extra`).  `xbuild(x)` gives the problem both ways: the class bit rows plus the
rank for the product, and every class's members sorted by rank (KEY order) for the oracle.

Rank kinds
  identity      rank[a] = a
  reverse       rank[a] = n_alleles - 1 - a
  random        a seeded permutation
  sparse_words  the active alleles get rank 0, the full 64-rank words 2, 4, 6, ... and rank n_alleles - 1: in the kernel's rank bitmap
                (rbm) word 0 holds one bit, odd words are empty between full ones, and the last rank is in use

What could not be built as the issue names it
  * Classes.from_host takes only a_pad % 512 == 0, so a row of 1, 63, 65, 127 or 129 words cannot reach the kernel through it.  The
    `row_width` family uses the widths on either side that can (8, 56, 64, 72, 120, 128 words: `lane + 64 < w64` is false for every
    lane at 64, true for lanes 0..7 at 72 and for all at 128), and the too-wide `handed_back` case is 136 words (a_pad = 8 704).
  * Classes.from_host takes a class of count 0, so the `keyerror` cases stay.
  * `prune1` ends with one survivor at exactly 1.0 whatever the input holds: no edge element can move it, so the WEIGHT premise is
    replaced for it by the assertion that the result is that lone 1.0.

The deep-decay cases (the plain-`/` branch of cols_share)
  A class {Y, X} of count 1 beside counts scaled by 10^k (exact in int64 and in a double, their sum below 2^63), Y strong and X in
  no other class.  One application of the map multiplies p_X by about 1 / (p_Y N), N the sum of the counts, so p_X falls through
  the kernel's 2^-600 gate within a run when the run is long enough; X is the last allele of the dict (its first class is the last
  one), so with more than 64 alleles in the dict it sits in a tile of its own kind: the strong alleles are in earlier tiles.
  decay_gate / decay_gate_cluster: X goes below 2^-620 for at least three applications, after applications above 2^-580.
  decay_zero: the SQUAREM extrapolation clamps a dict member to exactly +0.0 -- max(0.0, x) with x < 0 -- and it stays in the
    returned dict at 0.0 (p == 0.0 counts as "fast" at the gate).  This does not need the decaying X: x < 0 wants a member whose
    decay SLOWS (p1^2 > p p2), and a deep geometric decay has x = p (1 + g - g rho)^2 >= 0; without pruning an ordinary weak allele
    is clamped in most problems of the generator (several of `sum_groups` hold zeros too).  The case keeps the scaled counts and the
    class {Y, X}, so the zero sits beside a tile that takes the plain `/`.
  decay_denormal: X goes on below 2^-1022, through the denormal range, and underflows to 0.0 while it stays in the dict: a run of
    20 iterations or more does that with counts x 10^13 (about 2^-56 per application; the recorded run passes 2^-1061 and 2^-1056).
  decay_band / decay_band2: 64 alleles X_i decay at once, X_i with the strong allele i mod 8 in a class of count i + 1, so they
    cross the range in different places: 60 or more operands in [2^-1045, 2^-1022), where the error term of the three-instruction
    quotient (about 2^-53 of the numerator) underflows -- the part of the range where that form cannot be exact by construction.
  A class sum below 2^-200 is not reachable: one application of the map gives the members of a walked class at least count / N in
  total, and N < 2^63; so the class-sum half of the gate (`slow`, cl_ctl[3]) has no case.
"""
import collections
import functools

import numpy as np

import em_edge_cases as ec
import em_ref

RANKS = ("identity", "reverse", "random", "sparse_words")

XCase = collections.namedtuple("XCase", "id family base rank em_fast lookup extra expect")

def xcase(base, rank="random", em_fast=0, lookup=False, extra=(), expect=None):
    """em_fast: 0 = the default gates, -1 = the reference's order at every size (engine.em_set_fast(-1)); lookup: the case is also
    run with table lookups (forms d and e), so its decisions must be MARGIN from their thresholds and its edges carry WEIGHT;
    extra: ("keyerror",) | ("decay", k) = counts x 10^k plus the class {Y, X} x 1; expect: premises of the REFERENCE's run that
    test_emx_edge_ref.py asserts (those of em_edge_cases.case and after_prune = iterations after the first pruning)"""
    return XCase(base.id, base.family, base, rank, em_fast, lookup, tuple(extra), tuple(sorted((expect or {}).items())))


class XBuilt:
    """a_pad, n_alleles; idx / off / counts: CSR over allele ids, members ascending by id; kidx: the same with every class's members
    in KEY order (ascending rank); rank [n_alleles]; lengths [n_alleles] or None; actives: ids of the alleles that occur, ascending;
    X, Y: allele ids of the (first) decaying allele and its strong partner, Xs: every decaying allele (or None)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def rows(self):
        rows = np.zeros((len(self.counts), self.a_pad // 64), np.uint64)
        cls = np.repeat(np.arange(len(self.counts)), np.diff(self.off))
        np.bitwise_or.at(rows, (cls, self.idx >> 6), np.uint64(1) << (self.idx & 63).astype(np.uint64))
        return rows


def make_rank(kind, actives, n_alleles, seed):
    rng = np.random.RandomState(seed + 977)
    if kind == "identity":
        return np.arange(n_alleles, dtype=np.int32)
    if kind == "reverse":
        return (n_alleles - 1 - np.arange(n_alleles)).astype(np.int32)
    if kind == "random":
        return rng.permutation(n_alleles).astype(np.int32)
    if kind == "sparse_words":
        n = len(actives)
        assert n >= 2
        used, w = [0], 2
        while len(used) < n - 1:
            used += list(range(64 * w, 64 * w + min(64, n - 1 - len(used))))
            w += 2
        assert used[-1] < n_alleles - 1, "too many active alleles for empty words between full ones"
        used.append(n_alleles - 1)
        rank = np.full(n_alleles, -1, np.int64)
        rank[actives] = np.array(used)[rng.permutation(n)]
        rank[rank < 0] = np.setdiff1d(np.arange(n_alleles), used)
        return rank.astype(np.int32)
    raise ValueError(kind)


@functools.lru_cache(maxsize=4)
def xbuild(x):
    c = x.base
    b = ec.build(c)
    idx, off, counts = b.idx, b.off, b.counts
    free = np.setdiff1d(np.arange(c.n_alleles), b.actives)
    X = Y = Xs = None
    if x.extra and x.extra[0] == "keyerror":         # a class of count 0 whose two members occur nowhere else
        add = np.sort(free[[len(free) // 3, 2 * len(free) // 3]])
        idx, off, counts = np.concatenate([idx, add]), np.concatenate([off, [off[-1] + 2]]), np.concatenate([counts, [0]])
    elif x.extra and x.extra[0] == "decay":
        m = x.extra[2] if len(x.extra) > 2 else 1     # m decaying alleles: X_i with the strong allele i mod 8 in a class of count i + 1
        Xs = free[len(free) // 2:len(free) // 2 + m].tolist()
        X, Y = int(Xs[0]), int(b.actives[b.strong[0]])
        counts = counts * 10 ** x.extra[1]
        assert float(counts.sum()) < 2.0 ** 62 and (counts.astype(np.float64).astype(np.int64) == counts).all()
        for i, Xi in enumerate(Xs):
            pair = np.sort([Xi, int(b.actives[b.strong[i % len(b.strong)]])])
            idx, off, counts = np.concatenate([idx, pair]), np.concatenate([off, [off[-1] + 2]]), np.concatenate([counts, [i + 1]])
    elif x.extra:
        raise ValueError(x.extra)
    actives = np.unique(idx)
    rank = make_rank(x.rank, actives, c.n_alleles, c.seed)
    assert np.array_equal(np.sort(rank), np.arange(c.n_alleles))
    cls = np.repeat(np.arange(len(counts)), np.diff(off))
    kidx = idx[np.lexsort((rank[idx], cls))]
    return XBuilt(a_pad=c.a_pad, n_alleles=c.n_alleles, idx=idx.astype(np.int64), off=off.astype(np.int64), counts=counts.astype(np.int64),
                  kidx=kidx.astype(np.int64), rank=rank, lengths=b.lengths, actives=actives, X=X, Y=Y, Xs=Xs)


@functools.lru_cache(maxsize=4)
def reference(x):
    """(the em_ref problem, its run): shared by the tests of one case, never modified.  Raises KeyError where the reference does."""
    b = xbuild(x)
    pr = em_ref.Problem(b.idx, b.off, b.counts)
    return pr, pr.run(x.base.remove_low, b.lengths)


def record(x):
    """(values [applications][n] in the INPUT of every application of the EM map of the reference's run, NaN where the allele is not
    in the dict; the allele id of every column; the run), through em_ref.Problem's recording hook"""
    b = xbuild(x)
    pr = em_ref.Problem(b.idx, b.off, b.counts)
    seen = []
    pr.on_step = lambda v, pres: seen.append(np.where(pres, v, np.nan))
    r = pr.run(x.base.remove_low, b.lengths)
    return np.array(seen), pr.ids, r


def trajectory(x, allele):
    """one allele's column of record(x) as a list, None where it is not in the dict"""
    vals, ids, r = record(x)
    col = vals[:, int(np.searchsorted(ids, allele))]
    return [None if np.isnan(v) else float(v) for v in col], r


def dict_order(x):
    """allele ids in the insertion order of the reference's first dict (common:1300-1305): by first class, then by rank"""
    b = xbuild(x)
    cls = np.repeat(np.arange(len(b.counts)), np.diff(b.off))
    first = np.full(b.n_alleles, -1, np.int64)
    first[b.idx[::-1]] = cls[::-1]
    return b.actives[np.lexsort((b.rank[b.actives], first[b.actives]))]


def cluster_sized(x):
    """what hgx_emx_run shares out over several workgroups when the problem is alone in its launch"""
    return len(xbuild(x).counts) * x.base.a_pad >= 512 * 4096


# ---- the table --------------------------------------------------------------------------------------------------------------------
# Each line: the family of the issue's table, what varies, and the place in csrc/hgx_emx.hip it sits on.

def _table():
    T = []
    kind = lambda i, n, A: RANKS[i % 4] if (RANKS[i % 4] != "sparse_words" or (2 <= n and 2 * n + 192 < A)) else "random"
    # npos = A1 without pruning: seq_sum / seq_sum2 take groups of eight, two groups a trip, with an exit of its own for n8 = 8, 16, 24
    # and 32; pad_ordered zero-fills [npos, ceil8(npos)).  60 classes: the default route is k_em_wave, form (a) skips it
    for i, n in enumerate((1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)):
        T.append(xcase(ec.case("sum%d" % n, "sum_groups", 2048, n, 60, 1, remove_low=False, strong=min(n, 4), mem=(1, 6)), rank=kind(i + 1, n, 2048)))
    # npos after the first pruning (derive_order re-derives the insertion order, pad_ordered pads the shorter dict), then at least two
    # more iterations on it
    for i, (n, C) in enumerate(((1, 260), (8, 260), (9, 260), (16, 260), (17, 260), (64, 2049), (65, 2049))):
        if n == 1:
            base = ec.case("prune1", "sum_after_prune", 8192, 200, C, 1, strong=(150, 151, 1), send=0.5, twins=0)
        else:
            base = ec.case("prune%d" % n, "sum_after_prune", 8192, 200 if n < 64 else 700, C, 1, strong=n, mix=0.1 if n >= 64 else 0.3, send=0.9,
                           twins=1 if n < 64 else 0)
        T.append(xcase(base, rank=kind(i, base.n, 8192), lookup=True, expect=dict(first_prune=n, after_prune=2)))
    # A1: allele tiles of 64 (A1w), pairs of tiles in the Mk build (odd A1w), keep0 / keep1 at tile 64 (A1 = 4 096 | 4 097), items of eight
    # tiles in the transpose, the 512-element slabs and the eight alleles per thread (tid + 1024 k) of the table-lookup mode, the bitonic
    # sort's N = max(1024, pow2 >= A1), XA = 8 192.  From 1 023 on the problem is big enough for a lone-problem cluster
    for i, n in enumerate((63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8191, 8192)):
        T.append(xcase(ec.case("A%d" % n, "allele_tiles", 8192, n, 130 if n < 1023 else 260, 1, strong=min(n, 8 if n < 4095 else 12)),
                       rank=kind(i, n, 8192), lookup=True))
    # C: four classes per pass of the Mk build (c0 += 4 up to CpA), class tiles of 64 (Cw), 512-class slabs and four classes per
    # thread of the table-lookup mode, two 1 024-row tiles at 1 025 (mine_of), XC's default gate at 4 096
    for i, C in enumerate((1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096)):
        T.append(xcase(ec.case("C%d" % C, "class_tiles", 8192, 300, C, 1), rank=kind(i + 2, 300, 8192), lookup=True))
    # em_fast = -1: the kernel's hard gate of 32 768 classes; a cluster by itself (class tiles strided wave * n_wg + wg)
    for i, C in enumerate((4097, 8191, 8192, 8193, 32767, 32768)):
        T.append(xcase(ec.case("any%d" % C, "any_size", 512, 300, C, 1), rank=kind(i, 300, 512), em_fast=-1))
    # row width: rows staged in two 64-lane halves (`lane < w64`, `lane + 64 < w64`), orw / rank over 64 * w64 alleles
    for i, w in enumerate((8, 56, 64, 72, 120, 128)):
        T.append(xcase(ec.case("w%d" % w, "row_width", 64 * w, min(300, 48 * w), 130, 1), rank=kind(i + 1, min(300, 48 * w), 64 * w), lookup=True))
    # layout x rank: rbm[(r >> 6) & 127] / rpre and srt[j] against where the bits are in the rows
    for name, n, kw in (("one_word", 40, {}), ("gap_word", 128, {}), ("last_bit", 600, {}), ("ragged", 600, dict(n_alleles=8192 - 101))):
        for rk in (("reverse", "sparse_words") if n < 600 else ("random", "sparse_words")):
            T.append(xcase(ec.case("%s_%s" % (name, rk), "layout", 8192, n, 130, 1, layout=name, **kw), rank=rk, lookup=True))
    # lengths (vlen) distinct per allele id on a random rank: a length read at the rank or the dict position instead of the id shows
    T.append(xcase(ec.case("len_low", "lengths", 8192, 600, 130, 1, lengths=True), lookup=True))
    T.append(xcase(ec.case("len_full", "lengths", 8192, 600, 130, 1, lengths=True, remove_low=False), lookup=True))
    # status 1: the problem goes back to the caller, which continues on the table-lookup path and must not call the result exact
    T.append(xcase(ec.case("back_w136", "handed_back", 8704, 300, 130, 1)))
    T.append(xcase(ec.case("back_C4097", "handed_back", 1024, 300, 4097, 1)))
    T.append(xcase(ec.case("back_C32769", "handed_back", 512, 300, 32769, 1), em_fast=-1))
    # the reference's KeyError (common:1365-1369): status 2
    T.append(xcase(ec.case("keyerror", "keyerror", 8192, 300, 130, 1), lookup=True, extra=("keyerror",)))
    # ... in a cluster too: the leader breaks out of its loop, the helpers are told to leave, the leader reports the status
    T.append(xcase(ec.case("keyerror_cluster", "keyerror", 8192, 300, 260, 1), lookup=True, extra=("keyerror",)))
    T.append(xcase(ec.case("keyerror_any", "keyerror", 512, 300, 4097, 1), em_fast=-1, extra=("keyerror",)))
    # the plain-`/` branch (see the docstring)
    T.append(xcase(ec.case("decay_gate", "deep_decay", 8192, 100, 130, 1, remove_low=False, strong=8, twins=1, mem=(2, 5)), extra=("decay", 13),
                   expect=dict(decay="gate")))
    T.append(xcase(ec.case("decay_gate_cluster", "deep_decay", 8192, 100, 260, 1, remove_low=False, strong=8, twins=1, mem=(2, 5)), extra=("decay", 13),
                   expect=dict(decay="gate")))
    T.append(xcase(ec.case("decay_zero", "deep_decay", 8192, 100, 130, 1, remove_low=False, strong=8, twins=1, mem=(2, 5)), extra=("decay", 13),
                   expect=dict(decay="zero")))
    T.append(xcase(ec.case("decay_denormal", "deep_decay", 8192, 100, 130, 1, remove_low=False, strong=8, twins=2, mem=(2, 8)), extra=("decay", 13),
                   expect=dict(decay="denormal")))
    # 64 decaying alleles at once, their classes counted 1 .. 64 so that they cross the range in different places: quotients whose
    # numerator count * p lies just above the denormal range, where the error term of the three-instruction form underflows
    for id_, seed in (("decay_band", 1), ("decay_band2", 22)):
        T.append(xcase(ec.case(id_, "deep_decay", 8192, 100, 130, seed, remove_low=False, strong=8, twins=2, mem=(2, 8)), extra=("decay", 13, 64),
                       expect=dict(decay="band")))
    out = []
    for x in T:
        s = SEEDS.get(x.id, 1)
        s, k = s if isinstance(s, tuple) else (s, None)
        out.append(x._replace(base=x.base._replace(seed=s), extra=x.extra if k is None else (x.extra[0], k) + x.extra[2:]))
    return out


# The first seed (from 1) at which the case meets every premise of tests/test_emx_edge_ref.py -- for the decay cases (seed, k), the
# power of ten of the counts; every case not listed does at seed 1.
SEEDS = {"prune8": 9, "prune16": 26, "prune17": 6, "prune64": 3, "prune65": 2, "A511": 2, "A512": 2, "C2": 2, "C3": 3, "C5": 2, "C1023": 2,
         "w72": 3, "w128": 2, "decay_gate": (6, 13), "decay_gate_cluster": (23, 12), "decay_band2": (22, 13)}

CASES = _table()
BY_ID = {x.id: x for x in CASES}
