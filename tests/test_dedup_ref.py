"""The dict reference of the class dedup (tests/dedup_ref.py) against the C oracle on every generated texture, and the generators'
own promises -- two independent references pinned to each other before either judges a kernel (tests/test_gpu_dedup_edges.py)."""
import numpy as np
import pytest

import dedup_ref as dr

SIZES = (0, 1, 257, 5000)
WIDTHS = (8, 72)


def _masked(rows, mask):
    return rows if mask is None else rows & mask[None, :]


@pytest.mark.parametrize("w64", WIDTHS)
@pytest.mark.parametrize("name", sorted(dr.GENERATORS))
def test_dict_reference_equals_c_oracle_and_textures_keep_their_promises(orc, name, w64):
    for n in SIZES:
        (rows, wts, mask, keys), claim = dr.make_claim(name, n, w64, seed=1000 + n)
        assert rows.shape == (n, w64) and rows.dtype == np.uint64
        bits, cnt, first = dr.dedup_ref(rows, wts, mask)
        ob, oc, of = orc.dedup(rows, weight=wts, and_mask=mask)
        assert np.array_equal(bits, ob) and np.array_equal(cnt, oc) and np.array_equal(first, of), (name, n)
        assert len(cnt) == claim, (name, n, len(cnt), claim)
        m = _masked(rows, mask)
        assert np.array_equal(bits, m[first]) and np.all(np.diff(first) > 0)
        assert int(cnt.sum()) == int((np.ones(n, np.int64) if wts is None else wts)[m.any(axis=1)].sum())
        if keys is not None:
            assert keys.shape == (n,) and keys.dtype == np.uint64
            zero = ~m.any(axis=1)
            assert np.all(keys[zero] == np.uint64(dr.EMPTY)) and not np.any(keys[~zero] == np.uint64(dr.EMPTY))
            key_of = {}
            for i in np.flatnonzero(~zero).tolist():
                assert key_of.setdefault(m[i].tobytes(), int(keys[i])) == int(keys[i]), (name, n, i)


def test_textures_are_what_their_names_say():
    n = 5000
    rows = dr.make("random_zeros", n, 8, 3)[0]
    z = dr.zero_positions(n)
    assert {0, 1023, 1025, 4095, 4097, n - 1} <= set(z.tolist())
    assert not rows[z].any() and rows[np.setdiff1d(np.arange(n), z)].any(axis=1).all()
    for name in ("random", "random_zeros"):                      # the last live row founds a class of its own
        rows = dr.make(name, n, 8, 3)[0]
        _, cnt, first = dr.dedup_ref(rows)
        last_live = int(np.flatnonzero(rows.any(axis=1))[-1])
        assert first[-1] == last_live and cnt[-1] == 1 and len(cnt) == n // 3 + 1
    for w64 in (8, 72, 136):                                    # one-bit pool: every class one bit away from the base
        rows = dr.make("onebit", 300, w64, 4)[0]
        bits, _, _ = dr.dedup_ref(rows)
        pos = dr.onebit_positions(w64)
        assert len(bits) == len(pos) + 1
        base = min(range(len(bits)), key=lambda c: sum(int(np.unpackbits((bits[c] ^ b).view(np.uint8)).sum()) for b in bits))
        diffs = set()
        for c in range(len(bits)):
            if c != base:
                x = bits[c] ^ bits[base]
                (w,) = np.flatnonzero(x)
                assert int(x[w]) & (int(x[w]) - 1) == 0
                diffs.add((int(w), int(x[w]).bit_length() - 1))
        assert diffs == set(pos)
    assert any(w >= 64 for w, _ in dr.onebit_positions(72)) and {130, 131} <= {w for w, _ in dr.onebit_positions(136)}
    # probe chains: where every key starts
    rows, _, _, keys = dr.make("chain_global", 1500, 8, 5)
    assert np.all(keys & np.uint64(dr.table_size(1500) - 1) == np.uint64(dr.table_size(1500) - 2)) and len(set(keys.tolist())) == 1500
    assert len(set(((keys >> np.uint64(40)) & np.uint64(2047)).tolist())) > 1000
    rows, _, _, keys = dr.make("chain_lds", 5000, 8, 5)
    assert np.all((keys >> np.uint64(40)) & np.uint64(2047) == np.uint64(2046)) and len(set(keys.tolist())) == 700
    rows, _, _, keys = dr.make("chain_both", 1200, 8, 5)
    assert np.all((keys >> np.uint64(40)) & np.uint64(2047) == np.uint64(2046))
    assert np.all(keys & np.uint64(dr.table_size(1200) - 1) == np.uint64(dr.table_size(1200) - 2))
    # forged collisions: several contents per key, one key per content; the minority content where the name says
    for kind, per0 in (("first", 2), ("last", 2), ("three", 3), ("five", 5)):
        rows, _, _, keys = dr.make("forged_" + kind, 3000, 136, 6)
        by_key = {}
        for i in range(len(rows)):
            by_key.setdefault(int(keys[i]), set()).add(rows[i].tobytes())
        assert len(by_key) == dr.N_KEY_GROUPS and sorted(len(v) for v in by_key.values()) == sorted([per0] + [2] * (dr.N_KEY_GROUPS - 1))
        for contents in by_key.values():                        # contents of one key differ only in words >= 128
            cs = [np.frombuffer(c, np.uint64) for c in contents]
            assert all(not (c ^ cs[0])[:128].any() for c in cs)
        same_key = np.flatnonzero(keys == keys[0 if kind != "last" else -1])
        odd = 0 if kind != "last" else len(rows) - 1
        if kind in ("first", "last"):
            assert sum(rows[i].tobytes() == rows[odd].tobytes() for i in same_key) == 1 and len(same_key) > 100
    rows, _, _, keys = dr.make("forged_all", 1500, 8, 7)
    assert len(set(keys.tolist())) == 1 and len({r.tobytes() for r in rows}) == 1500
    w = dr.make("weights", 5000, 8, 8)[1]
    assert {0, 1, 1 << 40} <= set(w.tolist()) and dr.dedup_ref(dr.make("weights", 5000, 8, 8)[0], w)[1].max() > 1 << 40


def test_counts_reference_equals_column_by_column_python_sums():
    rng = np.random.RandomState(2)
    for n, w64, hi in ((0, 8, 10), (1, 8, 10), (9, 8, 1 << 24), (300, 72, 1 << 44), (5, 8, 1 << 62)):
        bits = rng.randint(0, 256, size=(n, w64 * 8)).astype(np.uint8).view(np.uint64).reshape(n, w64)
        cnt = rng.randint(hi // 2, hi, n).astype(np.int64)
        if n == 5:
            bits[:, 0] |= np.uint64(1)                           # allele 0 in all five classes: the sum leaves int64 on purpose
            cnt[:] = [1 << 62, (1 << 62) - 2, -(1 << 62), -(1 << 62), 1]     # (every subset sum still fits)
        tot, first = dr.counts_ref(bits, cnt)
        for a in list(range(0, 64 * w64, 37)) + [0, 64 * w64 - 1]:
            col = [c for c in range(n) if (int(bits[c, a >> 6]) >> (a & 63)) & 1]
            assert int(tot[a]) == sum(int(cnt[c]) for c in col) and int(first[a]) == (col[0] if col else -1)
