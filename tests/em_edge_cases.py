"""The cases of tests/test_gpu_em_edges.py: the chip-wide table-lookup EM (csrc/hgx_em.hip) at its structural edges (TEST
INFRASTRUCTURE: numpy only).  tests/test_em_ref.py checks every case's premises on the CPU -- decisions at least 1e-7 from
their thresholds, weight on both sides of every size edge, the iteration counts the host batching needs -- and the seeds in the
table were found by searching there; no case is filtered at run time.

A case is a `Case`; `build(case)` makes its problem.  The generator is a small read model: a few STRONG alleles (the sample's)
send a share `send` of the classes, every class holds its sender plus others up to `mem` members (a share `mix` of the others
strong: the ambiguity among the strong alleles sets how fast the EM converges), the n active alleles are dealt round the classes
so that each occurs, and counts are 1..299.  Every allele and class next to a size edge is made to matter by construction: edge
alleles are strong, edge classes are sent by a strong allele and counted 20 x.
"""
import collections
import functools

import numpy as np

import em_ref

# compact allele index: 64-bit word | 512-element slab, a1p step | 1 024-row cols chunk, register k of the fused steps | third chunk |
# EPT * BLOCK (fuse off, strided vector steps, 17th allele slab)
ALLELE_EDGES = (64, 512, 1024, 2048, 8192)
# class index: 64-bit word | 512-element slab | 1 024-row rows chunk | the reference-order gate | 17th class slab, second round of the
# tail's class-word loop (word 128) | 33rd class slab
CLASS_EDGES = (64, 512, 1024, 4096, 8192, 16384)

Case = collections.namedtuple("Case", "id family a_pad n_alleles n C seed remove_low lengths layout strong mix send mem masks twins expect pyref")


def case(id, family, a_pad, n, C, seed, remove_low=True, lengths=False, layout="scatter", n_alleles=None, strong=8, mix=0.5,
         send=0.85, mem=(2, 12), masks=0, twins=0, expect=None, pyref=False):
    """strong: how many strong alleles (the edge alleles are among them), or (lo, hi, k): k of them, all with compact index in
    [lo, hi); masks: > 0 = every class holds one of exactly `masks` distinct subsets of the strong alleles and weak alleles
    besides; expect: premises about the REFERENCE's run that test_em_ref.py asserts (n_iter, min_iter, max_iter, first_prune =
    alleles left by the first pruning, masks = distinct class masks over them, pruned = the final pruning removes something, lone = the
    result is one allele at abundance 1.0 whatever the input holds, so that taking an element out has nothing to move)"""
    return Case(id, family, a_pad, a_pad if n_alleles is None else n_alleles, n, C, seed, remove_low, lengths, layout, strong,
                mix, send, mem, masks, twins, tuple(sorted((expect or {}).items())), pyref)


class Built:
    """actives [n]: allele id of compact index j; idx / off / counts: CSR over ALLELE IDS; lengths [n_alleles] or None;
    strong: compact indices of the strong alleles"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def rows(self, a_pad):
        """the class bit matrix [C][a_pad / 64] that Classes.from_host takes"""
        rows = np.zeros((len(self.counts), a_pad // 64), np.uint64)
        cls = np.repeat(np.arange(len(self.counts)), np.diff(self.off))
        np.bitwise_or.at(rows, (cls, self.idx >> 6), np.uint64(1) << (self.idx & 63).astype(np.uint64))
        return rows


def _span(c):
    return (c.strong[0], c.strong[1]) if isinstance(c.strong, tuple) else (0, c.n)


def edge_alleles(c):
    """Compact allele indices on either side of every size edge inside the case, and the last one.  Where a family places the
    strong alleles in a range (so that whole chunks lose every allele to the pruning), only the edges in that range."""
    lo, hi = _span(c)
    e = {c.n - 1}
    for b in ALLELE_EDGES:
        if b < c.n:
            e |= {b - 1, b}
    return sorted(j for j in e if lo <= j < hi)


def edge_classes(c):
    e = {c.C - 1}
    for b in CLASS_EDGES:
        if b < c.C:
            e |= {b - 1, b}
    return sorted(e)


def _actives(c, rng):
    """allele ids of the n active alleles, ascending, by layout"""
    A, n = c.n_alleles, c.n
    if c.layout == "scatter":                # over the whole index range, first and last id included
        if n == 1:
            return np.array([A // 2 + 37])
        rest = rng.choice(np.arange(1, A - 1), n - 2, replace=False) if n > 2 else np.zeros(0, np.int64)
        return np.sort(np.concatenate([[0, A - 1], rest])).astype(np.int64)
    if c.layout == "one_word":               # every active allele in one 64-bit word
        assert n <= 64
        return 64 * 77 + np.sort(rng.choice(64, n, replace=False))
    if c.layout == "gap_word":               # two full words with an empty word between them
        assert n == 128
        return np.concatenate([64 * 50 + np.arange(64), 64 * 52 + np.arange(64)])
    if c.layout == "last_bit":               # bit a_pad - 1 set, the rest in the low half
        assert A == c.a_pad
        return np.sort(np.concatenate([rng.choice(A // 2, n - 1, replace=False), [A - 1]]))
    if c.layout == "ragged":                 # n_alleles < a_pad and no multiple of 64: the last allele id is active
        assert A < c.a_pad and A % 64
        return np.sort(np.concatenate([rng.choice(A - 1, n - 1, replace=False), [A - 1]]))
    raise ValueError(c.layout)


@functools.lru_cache(maxsize=4)
def build(c):
    rng = np.random.RandomState(c.seed)
    n, C = c.n, c.C
    actives = _actives(c, rng)
    assert len(actives) == n and (np.diff(actives) > 0).all() and 0 <= actives[0] and actives[-1] < c.n_alleles
    ec = set(edge_classes(c))
    strong = list(edge_alleles(c))
    lo, hi = _span(c)
    k = c.strong[2] if isinstance(c.strong, tuple) else c.strong
    pool = np.setdiff1d(np.arange(lo, hi), strong)
    if len(strong) < k and len(pool):
        strong += rng.choice(pool, min(len(pool), k - len(strong)), replace=False).tolist()
    strong = np.array(sorted(strong))
    weight = rng.uniform(1.0, 3.0 if len(strong) < 32 else 1.5, len(strong))     # (many strong alleles: all well above max / 10)
    weight /= weight.sum()
    subsets = []
    if c.masks:                              # `masks` distinct subsets of 1..3 strong alleles; the first len(strong) are the singletons
        got = {(int(j),) for j in strong}
        subsets = sorted(got)
        while len(subsets) < c.masks:
            s = tuple(sorted(rng.choice(strong, rng.randint(2, 4), replace=False).tolist()))
            if s not in got:
                got.add(s)
                subsets.append(s)
        assert len(subsets) == c.masks
    weak = np.setdiff1d(np.arange(n), strong)
    deal = [[] for _ in range(C)]            # every active allele occurs: dealt round the classes
    for i, j in enumerate(rng.permutation(weak if c.masks else n).tolist()):
        deal[(i * 7 + 3) % C].append(int(j))
    seen, members = set(), []
    for ci in range(C):
        for attempt in range(1000):
            if c.masks:                      # one of the subsets; beyond the first `masks` classes a share 1 - send holds weak alleles only
                m = set(subsets[ci] if ci < c.masks else (subsets[rng.randint(c.masks)] if ci in ec or rng.rand() < c.send else ()))
                m |= set(deal[ci]) or {int(weak[rng.randint(len(weak))])}
                fill = weak
            else:
                if ci in ec or rng.rand() < c.send:
                    src = int(strong[rng.choice(len(strong), p=weight)])
                else:
                    src = int(rng.randint(n))
                m = {src, *deal[ci]}
                fill = None
            want = max(len(m), int(rng.randint(c.mem[0], c.mem[1] + 1)))
            for _ in range(4 * want):        # (bounded: a few strong alleles alone cannot fill a class)
                if len(m) >= min(want, n):
                    break
                if fill is not None:
                    m.add(int(fill[rng.randint(len(fill))]))
                else:
                    m.add(int(strong[rng.randint(len(strong))]) if rng.rand() < c.mix else int(rng.randint(n)))
            for t in range(c.twins):         # strong[2t] and strong[2t + 1] are nearly always together: a flat direction, a slow EM
                a, b = int(strong[2 * t]), int(strong[2 * t + 1])
                if (a in m) != (b in m) and len(m) < c.mem[1] and rng.rand() < 0.97:
                    m |= {a, b}
            key = tuple(sorted(m))
            if key not in seen or n < 8:     # (classes are distinct, as a dedup leaves them; a handful of alleles cannot fill C)
                break
        seen.add(key)
        members.append(key)
    counts = rng.randint(1, 300, C).astype(np.int64)
    for ci in ec:
        counts[ci] *= 20
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    idx = actives[np.concatenate([np.array(m, np.int64) for m in members])].astype(np.int64)
    lengths = None
    if c.lengths:                            # distinct per allele id, so that a length read at the wrong index shows
        lengths = (3000 + rng.permutation(c.n_alleles)).astype(np.int32)
    return Built(actives=actives, idx=idx, off=off, counts=counts, lengths=lengths, strong=strong)


@functools.lru_cache(maxsize=4)
def reference(c):
    """(the em_ref problem, its run): shared by the tests of one case, never modified"""
    b = build(c)
    pr = em_ref.Problem(b.idx, b.off, b.counts)
    return pr, pr.run(c.remove_low, b.lengths)


def survivor_masks(c, alleles):
    """distinct non-empty class masks over the given allele ids: what k_em_tail merges the classes into"""
    b = build(c)
    sel = np.isin(b.idx, alleles)
    cls = np.repeat(np.arange(len(b.counts)), np.diff(b.off))[sel]
    pos = np.searchsorted(np.sort(alleles), b.idx[sel])
    masks = collections.defaultdict(int)
    for ci, p in zip(cls.tolist(), pos.tolist()):
        masks[ci] |= 1 << p
    return len(set(masks.values()))


# ---- the table --------------------------------------------------------------------------------------------------------------------
# Each line: the family of the issue's table, what varies, and the place in csrc/hgx_em.hip it sits on.

def _table():
    T = []
    # compact length n: a1p = max(512, ceil512(n)) and k_zero_padding's rows [n, a1p) (hgx_ensure_compact); k_act_from_mask's scan
    # and rank; a second allele slab at 513 (k_lutmatvec<ROWS> grid.x, the deferred combine's src_slabs); a second cols chunk at
    # 1 025 (k_lutmatvec<COLS> grid.y, `n < N`), register k = 1 of the fused steps
    for n in (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025):
        T.append(case("n%d" % n, "compact_length", 8192, n, 130, 1, strong=min(n, 8), pyref=n in (63, 65), expect=dict(lone=True) if n == 1 else None))
    # layout of the actives: k_col_or / k_act_from_mask / k_transpose_compact's `m == 0` return and `base[aw] + popc`
    T.append(case("one_word", "layout", 8192, 40, 130, 1, layout="one_word", pyref=True))
    T.append(case("gap_word", "layout", 8192, 128, 130, 1, layout="gap_word"))
    T.append(case("last_bit", "layout", 8192, 600, 130, 1, layout="last_bit"))
    T.append(case("ragged", "layout", 8192, 600, 130, 1, layout="ragged", n_alleles=8192 - 101))
    # row width: k_col_or's block size switches at w64 = 128; base / act come from the host above w64 = 512
    for a_pad, n in ((512, 500), (8192, 600), (8704, 600), (33280, 600)):
        T.append(case("w%d" % (a_pad // 64), "row_width", a_pad, n, 130, 1))
    # classes: c64 rounded to 8 words; 512-class slabs and 1 024-row chunks of the rows pass; the deferred combine's groups of 16
    # slabs (17 at 8 193) and the ticket combine's groups of 32 (33 at 16 385, em_skip="defer")
    for C in (65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385):
        T.append(case("C%d" % C, "classes", 8192, 700, C, 1, pyref=C == 65))
    # long vectors: `fuse` needs a1p <= 8 192; above, the strided branches of k_em_squarem / k_em_advance and 17 allele slabs in the
    # cols pass's own ticket combine
    for n in (8191, 8192, 8193):
        T.append(case("long%d_low" % n, "long_vectors", 8704, n, 4097, 1, strong=12))
        T.append(case("long%d_len" % n, "long_vectors", 8704, n, 4097, 1, remove_low=False, lengths=True, strong=12))
    T.append(case("long8193_low_len", "long_vectors", 8704, 8193, 4097, 1, lengths=True, strong=12))
    # empty cols chunk: k_lutmatvec<COLS>'s `!__syncthreads_or(n < N && e_pres)` return, three chunks of alleles (n = 2 049); the
    # GPU test runs these with em_skip="tail" too, where the full passes go on after the pruning
    T.append(case("chunk_high", "empty_chunk", 8192, 2049, 1025, 1, strong=(1024, 2049, 80), expect=dict(min_iter=12, min_first_prune=65)))
    T.append(case("chunk_low", "empty_chunk", 8192, 2049, 1025, 1, strong=(0, 1024, 80), expect=dict(min_iter=12, min_first_prune=65)))
    T.append(case("chunk_last", "empty_chunk", 8192, 2049, 1025, 1, strong=(2048, 2049, 1), send=0.5, expect=dict(min_iter=12, first_prune=1, lone=True)))
    # lengths through compaction: l[j] = allele_len[h_act[j]] (em_impl_inner) and k_em_finish's p / len / tot
    T.append(case("len_low", "lengths", 8192, 600, 130, 1, lengths=True))
    T.append(case("len_full", "lengths", 8192, 600, 130, 1, lengths=True, remove_low=False))
    # batching: 4 iterations, then up to 7 more, then the speculative tail (the host loop of em_impl_inner)
    T.append(case("iter4", "batching", 8192, 700, 4097, 1, mix=0.9, expect=dict(n_iter=4)))
    T.append(case("iter5", "batching", 8192, 700, 4097, 1, mix=0.9, expect=dict(n_iter=5)))
    T.append(case("iter_le10", "batching", 8192, 700, 4097, 1, mix=0.8, expect=dict(max_iter=10, min_iter=6, pruned=True)))
    T.append(case("iter11", "batching", 8192, 700, 4097, 1, mix=0.3, strong=30, expect=dict(n_iter=11)))
    # (a pruning that removes mass kicks `diff` up for two more iterations: 12 needs a run whose first pruning removes next to nothing)
    T.append(case("iter12", "batching", 8192, 8, 130, 1, strong=8, twins=1, mem=(2, 5), expect=dict(n_iter=12)))
    T.append(case("iter_ge20", "batching", 8192, 700, 1025, 1, mix=0.6, strong=8, twins=2, mem=(2, 16), expect=dict(min_iter=20)))
    # tail hand-over: k_em_tail takes <= 64 survivors (`A1 > 64`) and <= 64 distinct masks (`n_keys > 64`); its class-word loop
    # covers 8 192 classes a round
    T.append(case("surv64", "tail", 8192, 700, 2049, 1, strong=64, mix=0.1, send=0.9, expect=dict(min_iter=12, first_prune=64)))
    T.append(case("surv65", "tail", 8192, 700, 2049, 1, strong=65, mix=0.1, send=0.9, expect=dict(min_iter=12, first_prune=65)))
    T.append(case("masks64", "tail", 8192, 600, 130, 1, strong=10, masks=64, send=0.7, expect=dict(min_iter=12, first_prune=10, masks=64)))
    T.append(case("masks65", "tail", 8192, 600, 130, 1, strong=10, masks=65, send=0.7, expect=dict(min_iter=12, first_prune=10, masks=65)))
    T.append(case("tail_C8193", "tail", 8192, 700, 8193, 1, strong=6, mix=0.3, twins=1, expect=dict(min_iter=12, first_prune=6, max_masks=64)))
    T.append(case("tail_C8193_len", "tail", 8192, 700, 8193, 1, strong=6, mix=0.3, twins=1, lengths=True, expect=dict(min_iter=12, max_first_prune=64, max_masks=64)))
    T.append(case("tail_C130_len", "tail", 8192, 600, 130, 1, strong=6, lengths=True, expect=dict(min_iter=12, max_first_prune=64, max_masks=64)))
    return [c._replace(seed=SEEDS.get(c.id, 1)) for c in T]


# The first seed (from 1) at which the case meets every premise of tests/test_em_ref.py; every case not listed does at seed 1.
SEEDS = {"n511": 2, "n512": 2, "n1023": 2, "chunk_high": 3, "chunk_low": 2, "iter4": 45, "iter5": 11, "iter_le10": 7, "iter12": 3, "iter_ge20": 41,
         "surv64": 3, "surv65": 2, "masks64": 25, "masks65": 22, "tail_C8193": 2, "tail_C130_len": 2}

CASES = _table()
