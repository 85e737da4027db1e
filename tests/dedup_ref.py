"""A plain reference of the class dedup and of Gene_counts, and the inputs that put them on their structural edges (TEST
INFRASTRUCTURE: numpy and a Python dict, no GPU, no torch).

`dedup_ref` is the contract of hgx_dedup_classes as include/hgx.h states it; `counts_ref` that of hgx_allele_counts.  Both are
pinned to the C oracle by tests/test_dedup_ref.py before tests/test_gpu_dedup_edges.py lets them judge a kernel.

Every generator is reached through `make(name, n, w64, seed)` and returns `(rows, weights|None, mask|None, keys|None)`;
`make_claim` adds the number of classes the texture promises by construction.  Supplied keys honour the caller's
contract: equal masked rows carry equal keys, an all-zero row carries EMPTY and no other row does.
"""
import numpy as np

EMPTY = 0xFFFFFFFFFFFFFFFF
_U1 = np.uint64(1)


# ---- references -----------------------------------------------------------------------------------------------------------------

def dedup_ref(rows, weights=None, and_mask=None):
    """-> (bits [C][w64] uint64, counts [C] int64, first_rows [C] int64), classes in first-seen order."""
    rows = np.ascontiguousarray(rows, np.uint64)
    n, w64 = rows.shape
    masked = rows if and_mask is None else rows & np.asarray(and_mask, np.uint64)[None, :]
    wts = None if weights is None else [int(x) for x in np.asarray(weights).tolist()]
    index, first, count = {}, [], []
    for i in np.flatnonzero(masked.any(axis=1)).tolist():
        k = masked[i].tobytes()
        c = index.setdefault(k, len(first))
        if c == len(first):
            first.append(i)
            count.append(0)
        count[c] += 1 if wts is None else wts[i]
    first = np.array(first, np.int64)
    bits = masked[first] if len(first) else np.zeros((0, w64), np.uint64)
    return np.ascontiguousarray(bits), np.array(count, np.int64), first


def members(bits):
    """[C][w64] uint64 -> [C][64 * w64] bool, allele a of class c at [c][a]"""
    bits = np.ascontiguousarray(bits, np.uint64)
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little").astype(bool)


def counts_ref(bits, counts):
    """-> (per-allele sum of the counts of the classes holding the allele [A] int64, first such class or -1 [A] int64)"""
    bits = np.ascontiguousarray(bits, np.uint64)
    n, w64 = bits.shape
    if n == 0:
        return np.zeros(64 * w64, np.int64), np.full(64 * w64, -1, np.int64)
    m = members(bits)
    cnt = [int(x) for x in np.asarray(counts).tolist()]
    if max(abs(x) for x in cnt) * n >= 2 ** 63:             # a column sum can leave int64 on the way: Python ints
        tot = (m.astype(object) * np.array(cnt, object)[:, None]).sum(axis=0)
    else:
        tot = np.zeros(64 * w64, np.int64)
        for c0 in range(0, n, 512):                         # (in blocks: [C][A] int64 at once is hundreds of MB)
            tot += np.array(cnt[c0:c0 + 512], np.int64) @ m[c0:c0 + 512].astype(np.int64)
    first = np.where(m.any(axis=0), m.argmax(axis=0), -1)
    return np.array([int(x) for x in tot], np.int64), first.astype(np.int64)


def table_size(n):
    """the dedup's table rule today: T = max(1024, next power of two >= 2n)"""
    t = 1024
    while t < 2 * n:
        t <<= 1
    return t


# ---- building blocks --------------------------------------------------------------------------------------------------------------

def _pool(rng, k, w64):
    """k distinct non-zero rows"""
    p = rng.randint(0, 256, size=(max(k, 1), w64 * 8)).astype(np.uint8).view(np.uint64)[:k]
    assert len({r.tobytes() for r in p}) == k and p.any(axis=1).all()
    return p


def _assemble(pool, cls, key_of_class=None):
    """cls[i] = class of row i, -1 = an all-zero row"""
    cls = np.asarray(cls, np.int64)
    rows = np.zeros((len(cls), pool.shape[1]), np.uint64)
    live = cls >= 0
    rows[live] = pool[cls[live]]
    keys = None
    if key_of_class is not None:
        keys = np.full(len(cls), EMPTY, np.uint64)
        keys[live] = np.asarray(key_of_class, np.uint64)[cls[live]]
    return rows, keys


def _each_then_random(rng, n, k, shuffle=True):
    """n labels out of k: every label once (shuffled, or in order) as far as n reaches, the rest at random"""
    head = (rng.permutation(k) if shuffle else np.arange(k))[:n]
    return np.concatenate([head, rng.randint(0, max(k, 1), max(n - k, 0))]).astype(np.int64)


def zero_positions(n):
    """index 0, the last index, and both sides of every multiple of 1024"""
    z = {0, n - 1}
    for m in range(1024, n, 1024):
        z.update((m - 1, m + 1))
    return np.array(sorted(i for i in z if 0 <= i < n), np.int64)


def _bit(w64, word, bit):
    r = np.zeros(w64, np.uint64)
    r[word] = _U1 << np.uint64(bit)
    return r


def onebit_positions(w64):
    """(word, bit) of the single bit in which the classes of the `onebit` pool differ"""
    pos = [(0, 0), (w64 - 1, 63), (1, 33), (w64 - 3, 17)]                 # first bit, last bit, two odd-indexed words
    if w64 > 64:
        pos += [(64, 5), (w64 - 1, 0)]                                   # the second lane trip of the 64-lane loops
    if w64 > 128:
        pos += [(130, 40), (131, 41)]                                   # the second trip of the 128-bit compare
    return pos


# ---- sizes: four textures, with and without interleaved zero rows -------------------------------------------------------------------

def _texture(kind, zeros):
    def gen(n, w64, seed):
        rng = np.random.RandomState(seed)
        dead = zero_positions(n) if zeros else np.zeros(0, np.int64)
        live = np.setdiff1d(np.arange(n), dead)
        L = len(live)
        if kind == "distinct":
            k, lab = L, np.arange(L)
        elif kind == "identical":
            k, lab = min(1, L), np.zeros(L, np.int64)
        elif kind == "alternate":
            k, lab = min(2, L), np.arange(L) % 2
        else:                                               # n // 3 + 1 classes; the last live row founds one of them
            k = min(n // 3 + 1, L)
            lab = np.zeros(L, np.int64)
            if k > 1:
                lab[:L - 1] = _each_then_random(rng, L - 1, k - 1)
                lab[L - 1] = k - 1
        cls = np.full(n, -1, np.int64)
        cls[live] = lab
        rows, _ = _assemble(_pool(rng, k, w64), cls)
        return (rows, None, None, None), k
    return gen


# ---- row width: classes that differ in exactly one bit ---------------------------------------------------------------------------

def _onebit_pool(rng, w64):
    base = _pool(rng, 1, w64)[0]
    return np.stack([base] + [base ^ _bit(w64, w, b) for w, b in onebit_positions(w64)])


def _onebit(n, w64, seed):
    rng = np.random.RandomState(seed)
    pool = _onebit_pool(rng, w64)
    rows, _ = _assemble(pool, _each_then_random(rng, n, len(pool)))
    return (rows, None, None, None), min(n, len(pool))


# ---- masks -----------------------------------------------------------------------------------------------------------------------

def _split(w64):
    return 64 if w64 > 64 else w64 // 2


def _mask_high(n, w64, seed):
    """only the words from _split(w64) on survive: 40 contents with 10 distinct upper parts, 4 contents with an empty upper part"""
    rng = np.random.RandomState(seed)
    s = _split(w64)
    pool = _pool(rng, 44, w64)
    pool[:40, s:] = _pool(rng, 10, w64 - s)[np.arange(40) % 10]
    pool[40:, s:] = 0
    rows, _ = _assemble(pool, _each_then_random(rng, n, 44, shuffle=False))
    mask = np.zeros(w64, np.uint64)
    mask[s:] = np.uint64(EMPTY)
    return (rows, None, mask, None), min(n, 10)


def _mask_merge(n, w64, seed):
    """two one-bit pools; the mask erases every differing bit: each pool collapses into one class"""
    rng = np.random.RandomState(seed)
    a, b = _onebit_pool(rng, w64), _onebit_pool(rng, w64)
    pool = np.concatenate([a, b])
    mask = np.full(w64, EMPTY, np.uint64)
    for w, bit in onebit_positions(w64):
        mask[w] &= ~(_U1 << np.uint64(bit))
    assert (a[0] & mask).tobytes() != (b[0] & mask).tobytes()
    half = len(a)
    lab = np.concatenate([[0, half][:n], rng.randint(0, len(pool), max(n - 2, 0))]).astype(np.int64)
    rows, _ = _assemble(pool, lab)
    return (rows, weights_40(rng, n), mask, None), min(n, 2)


def _mask_third(n, w64, seed):
    """every third row has bits only where the mask has none"""
    rng = np.random.RandomState(seed)
    mask = np.full(w64, EMPTY, np.uint64)
    mask[:4] = 0
    keep = _pool(rng, 30, w64)
    assert len({(r & mask).tobytes() for r in keep}) == 30 and (keep & mask).any(axis=1).all()
    gone = _pool(rng, 30, w64)
    gone[:, 4:] = 0
    pool = np.concatenate([keep, gone])
    third = np.arange(n) % 3 == 1
    lab = np.zeros(n, np.int64)
    lab[~third] = _each_then_random(rng, int((~third).sum()), 30)
    lab[third] = 30 + rng.randint(0, 30, int(third.sum()))
    rows, _ = _assemble(pool, lab)
    return (rows, None, mask, None), min(int((~third).sum()), 30)


def _mask_all(n, w64, seed):
    rng = np.random.RandomState(seed)
    pool = _pool(rng, 30, w64)
    pool[:, w64 // 2:] = 0
    mask = np.zeros(w64, np.uint64)
    mask[w64 // 2:] = np.uint64(EMPTY)
    rows, _ = _assemble(pool, rng.randint(0, 30, n))
    return (rows, None, mask, None), 0


# ---- weights ---------------------------------------------------------------------------------------------------------------------

def weights_40(rng, n):
    """int64 weights: 0, 1, 2^31, 2^32, 2^40 and random values below 2^40"""
    fixed = np.array([0, 1, 1 << 31, 1 << 32, 1 << 40], np.int64)
    w = np.where(rng.rand(n) < 0.5, fixed[rng.randint(0, len(fixed), n)], rng.randint(0, 1 << 40, n).astype(np.int64))
    return w.astype(np.int64)


def _weights(n, w64, seed):
    """50 classes and zero rows; class 0 carries weight 0 only (a class all the same), class 1 weight 2^40 only"""
    rng = np.random.RandomState(seed)
    live = np.setdiff1d(np.arange(n), zero_positions(n)[1:])
    cls = np.full(n, -1, np.int64)
    cls[live] = _each_then_random(rng, len(live), 50)
    w = weights_40(rng, n)
    w[cls == 0] = 0
    w[cls == 1] = 1 << 40
    rows, _ = _assemble(_pool(rng, 50, w64), cls)
    return (rows, w, None, None), min(len(live), 50)


# ---- steered keys: probe chains ------------------------------------------------------------------------------------------------------

def _chain(kind):
    def gen(n, w64, seed):
        rng = np.random.RandomState(seed)
        T = table_size(n)
        if kind == "lds":                                   # every key starts at LDS slot 2046 of 2048; low bits at random
            k = min(700, n)
            key = (rng.randint(0, 1 << 13, k).astype(np.uint64) << np.uint64(51)) | np.uint64(2046 << 40) \
                | rng.randint(0, 1 << 40, k).astype(np.uint64)
            cls = _each_then_random(rng, n, k)
        else:                                               # all rows distinct, every key starts at table slot T - 2
            k = n
            j = np.arange(1, n + 1).astype(np.uint64)
            key = (j << np.uint64(40)) | np.uint64(T - 2) if kind == "global" else \
                (j << np.uint64(51)) | np.uint64(2046 << 40) | np.uint64(T - 2)
            cls = np.arange(n)
        assert len(set(key.tolist())) == k and EMPTY not in key.tolist()
        rows, keys = _assemble(_pool(rng, k, w64), cls, key)
        return (rows, None, None, keys), k
    return gen


# ---- forged collisions: several contents under one key, every content under exactly one key -------------------------------------------

N_KEY_GROUPS = 11


def _forged(kind, weighted=False, masked=False):
    def gen(n, w64, seed):
        rng = np.random.RandomState(seed)
        if kind == "all":                                   # every row distinct, ONE key: n - 1 rows leave the founder's slot
            rows, keys = _assemble(_pool(rng, n, w64), np.arange(n), np.full(n, 0x9E3779B97F4A7C15, np.uint64))
            total = n
        else:
            per_key = [{"three": 3, "five": 5}.get(kind, 2)] + [2] * (N_KEY_GROUPS - 1)
            bases = _pool(rng, N_KEY_GROUPS, w64)
            pool, key = [], []
            for g, m in enumerate(per_key):                 # content c of key group g: the base with one bit of the LAST 8 words flipped
                for c in range(m):
                    pool.append(bases[g] ^ (_bit(w64, w64 - 8 + (3 * c + g) % 8, (7 * c + g) % 48) if c else np.uint64(0)))
                    key.append(((g + 1) * 0x9E3779B97F4A7C15) & EMPTY)
            pool = np.stack(pool)
            total = len(pool)
            # label 1 = the minority content of key group 0: it appears once, at row 0 (`first`) or at the last row (`last`)
            others = np.array([c for c in range(total) if c != 1], np.int64)
            body = others[_each_then_random(rng, max(n - 1, 0), total - 1)]
            lab = np.concatenate([body, [1]] if kind == "last" else [[1], body])[:n].astype(np.int64)
            rows, keys = _assemble(pool, lab, key)
        mask = None
        if masked:                                          # leaves the contents distinct (the flipped bits are below bit 48)
            mask = np.full(w64, 0xFFFFFFFFFFFF5555, np.uint64)
            mask[w64 - 8:] = np.uint64(0x0000FFFFFFFFFFFF)
            assert len({(r & mask).tobytes() for r in rows}) == len({r.tobytes() for r in rows})
        wts = rng.randint(0, 6, n).astype(np.int64) if weighted else None
        return (rows, wts, mask, keys), min(n, total)
    return gen


# ---- registry ----------------------------------------------------------------------------------------------------------------------

TEXTURES = ("distinct", "identical", "random", "alternate")
GENERATORS = {"onebit": _onebit, "mask_high": _mask_high, "mask_merge": _mask_merge, "mask_third": _mask_third,
              "mask_all": _mask_all, "weights": _weights, "chain_global": _chain("global"), "chain_lds": _chain("lds"),
              "chain_both": _chain("both")}
for _t in TEXTURES:
    GENERATORS[_t] = _texture(_t, False)
    GENERATORS[_t + "_zeros"] = _texture(_t, True)
FORGED = ("first", "last", "three", "five", "all")
for _k in FORGED:
    for _w in (False, True):
        for _m in (False, True):
            GENERATORS["forged_" + _k + ("_w" if _w else "") + ("_m" if _m else "")] = _forged(_k, _w, _m)


def make_claim(name, n, w64, seed):
    """-> ((rows, weights|None, mask|None, keys|None), number of classes the texture promises)"""
    return GENERATORS[name](n, w64, seed)


def make(name, n, w64, seed):
    return GENERATORS[name](n, w64, seed)[0]
