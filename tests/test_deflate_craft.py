"""The crafted DEFLATE members of tests/deflate_craft.py against zlib alone (no GPU): every valid member inflates to the expansion of
its token list, every refused one is refused by the host reader's rule with the zlib message its row names, every member fits a BGZF
container -- and the table covers what it claims to cover: each branch of the kernel's copy_match at both sides of every boundary, the
independent batch with near and far matches, a dependent match inside a window, the T_MAX cut, the second-level pool's limits and a
symbol of 48 bits.  The conditions are worked out with the small restatements of the kernel's rules in deflate_craft (copy_branch,
batch_branch, windows, sub_table_demand); its constants are read from csrc/hgx_inflate.hip, so a retuned ring moves the cases."""
import random
import zlib

import deflate_craft as dc

RING, FLUSH, T_MAX, NEAR_MAX = dc.RING, dc.FLUSH, dc.T_MAX, dc.NEAR_MAX


def by_name(group, name):
    (c,) = [c for c in dc.cases(group) if c.name == name]
    return c


def test_writer_primitives_against_zlib():
    """The writer itself: fixed, dynamic and stored blocks of random tokens inflate (zlib) to expand(tokens); canonical codes of the
    fixed lengths are RFC 1951's; the length / distance symbol tables cover their ranges without gaps."""
    assert [dc.length_symbol(n)[0] for n in (3, 10, 11, 258)] == [257, 264, 265, 285] and dc.length_symbol(258, True) == (284, 5, 31)
    assert [dc.distance_symbol(d)[0] for d in (1, 4, 5, 24577, 32768)] == [0, 3, 4, 29, 29] and dc.distance_symbol(32768)[2] == 8191
    for n in range(3, 259):
        s, e, v = dc.length_symbol(n)
        assert dc.LEN_BASE[s - 257] + v == n and v < (1 << e) or (e == 0 and v == 0)
    codes = dc.canonical_codes(dc.FIXED_LIT)
    assert codes[0] == (int("00110000"[::-1], 2), 8) and codes[256] == (0, 7) and codes[280] == (int("11000000"[::-1], 2), 8) and codes[144][1] == 9
    rng = random.Random(3)
    for trial in range(30):
        payload, cdata = dc.random_member(rng, 20000)
        assert zlib.decompressobj(-15).decompress(cdata) == payload
    assert dc.expand([1, 2, 3, (5, 2), (3, 7)]) == bytes([1, 2, 3, 2, 3, 2, 3, 2, 2, 3, 2])
    data = bytes(rng.randrange(4) for _ in range(5000))
    assert dc.expand(dc.lz_parse(data)) == data and any(not isinstance(t, int) for t in dc.lz_parse(data))


def test_host_verdict_is_the_container_rule():
    raw = b"hello hello hello"
    cdata = dc._fixed(list(raw))
    crc = zlib.crc32(raw)
    assert dc.host_verdict(cdata, crc, len(raw)) == (True, raw, None)
    assert dc.host_verdict(cdata + b"trailing", crc, len(raw)) == (True, raw, None)           # bytes behind the final block
    assert dc.host_verdict(cdata, 12345, 0) == (True, b"", None)                               # ISIZE 0: not decoded at all
    assert dc.host_verdict(cdata, crc ^ 1, len(raw)) == (False, None, "wrong CRC")
    assert dc.host_verdict(cdata, crc, len(raw) - 1) == (False, None, "more output than ISIZE")
    assert dc.host_verdict(cdata, crc, len(raw) + 1) == (False, None, "less output than ISIZE")
    assert dc.host_verdict(cdata[:5], crc, len(raw)) == (False, None, "stream incomplete")
    assert dc.host_verdict(b"\x07", crc, len(raw)) == (False, None, "invalid block type")


def test_every_valid_case_inflates_to_its_tokens():
    valid = dc.cases(valid=True)
    assert len(valid) >= 60
    for c in valid:
        tokens = c.meta.get("tokens")
        if tokens is not None and c.isize:
            assert dc.expand(tokens) == c.payload, c
        ok, out, why = dc.host_verdict(c.cdata, c.crc, c.isize)
        assert ok and out == c.payload and why is None, (c, why)
        if c.isize:                                                            # (and zlib itself, without the container rule)
            assert zlib.decompressobj(-15).decompress(c.cdata) == c.payload, c
    c = by_name("sizes", "isize_0_stream_not_empty")
    assert zlib.decompressobj(-15).decompress(c.cdata) == dc.expand(c.meta["tokens"]) != b"" and c.payload == b""


def test_every_invalid_case_is_refused_with_its_message():
    rows = dc.cases("refused")
    assert len(rows) >= 30
    for c in rows:
        ok, out, why = dc.host_verdict(c.cdata, c.crc, c.isize)
        assert not ok and out is None and why == c.why, (c, why)
        assert c.verdict == dc.VERDICT_OF[c.why] != dc.OK, c
        assert c.isize > 0
    for c in dc.cases("truncated"):
        ok, _, why = dc.host_verdict(c.cdata, c.crc, c.isize)
        assert not ok, (c, why)
        whole = c.meta["whole"]
        assert dc.host_verdict(whole, c.crc, c.isize)[0] and c.cdata == whole[:len(c.cdata)] and len(c.cdata) in (1, 2, 3, len(whole) // 2)
    # every message of the mapping has a row, except none
    assert {c.why for c in rows} == set(dc.VERDICT_OF)
    # "wrong CRC only": the stream and the size are right
    c = by_name("refused", "crc_one_bit")
    out = zlib.decompressobj(-15).decompress(c.cdata)
    assert len(out) == c.isize and bin((zlib.crc32(out) ^ c.crc) & 0xFFFFFFFF).count("1") == 1


def test_every_member_fits_a_bgzf_container():
    for c in dc.case_table():
        assert c.isize <= 65536 and (c.payload is None or len(c.payload) <= 65536), c
        assert len(c.member()) <= 65536, c
    assert max(len(c.member()) for c in dc.case_table()) == 65536                 # (the largest stored block fills one)
    assert max(c.isize for c in dc.case_table()) == 65536


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------
def all_matches(group):
    return [m for c in dc.cases(group) for m in dc.positions(c.meta["tokens"])]


def test_far_distance_cases_lie_beyond_what_zlib_writes():
    for c in dc.cases("far_distances"):
        got = {(n, d) for _, n, d in dc.positions(c.meta["tokens"])}
        assert got == {(n, d) for n in (3, 258) for d in (32768, 32767, 32507)}
        assert all(d > 32768 - 262 for _, d in got) and len(c.payload) > 32768
    assert max(by_name("far_distances", "dynamic").meta["lit_lens"]) > 8


def test_switch_cases_cover_both_sides_of_every_boundary():
    ms = all_matches("near_far_switch")
    dists = (NEAR_MAX - 1, NEAR_MAX, NEAR_MAX + 1, RING - T_MAX, RING - 1, RING, RING + 1)
    lengths = (3, 63, 64, 65, 258)
    for d in dists:
        for n in lengths:
            here = [t for t, n2, d2 in ms if (n2, d2) == (n, d)]
            assert {t % FLUSH for t in here} >= {0, 1, FLUSH - 1}, (d, n)
            assert any(t // FLUSH != (t + n - 1) // FLUSH for t in here), ("no match across a flush boundary", d, n)
            assert any(t // RING != (t + n - 1) // RING for t in here), ("no match across the ring's wrap", d, n)
            assert all(dc.copy_branch(t, n, d) == ("near" if d <= NEAR_MAX else "far") for t in here)
    assert {dc.copy_branch(t, n, d) for t, n, d in ms} == {"near", "far"}
    # each match is its own decision: a literal on both sides
    for c in dc.cases("near_far_switch"):
        tok = c.meta["tokens"]
        assert all(isinstance(tok[i - 1], int) for i, t in enumerate(tok) if not isinstance(t, int))


def test_overlap_cases_cover_every_short_distance():
    ms = all_matches("overlap")
    assert {(n, d) for _, n, d in ms} >= {(n, d) for n in (258, 257) for d in range(1, 258)}
    assert {(n, d) for _, n, d in ms} >= {(n, n + k) for n in (3, 64, 65, 258) for k in (-1, 0, 1)}
    assert {dc.copy_branch(t, n, d) for t, n, d in ms} == {"run", "overlap", "near"}
    # the reciprocal's modulo is exact on every (i, dist) these cases use: the float expression of the kernel, in float32
    import numpy as np
    for d in range(2, 258):
        i = np.arange(258, dtype=np.float32)
        q = ((i + np.float32(0.5)) * (np.float32(1.0) / np.float32(d))).astype(np.uint32)
        assert (q == np.arange(258) // d).all(), d


def _window_view(c):
    """[(window's wpos, [(token index, my_off, length, dist, branch)])] of a window_chains case."""
    trace = c.meta["trace"]
    out = []
    for win in dc.windows(trace, c.meta["wpos0"]):
        rows = []
        for i, off, wpos in win:
            used, olen, d = trace[i]
            rows.append((i, off, olen, d, dc.batch_branch(wpos, off, olen, d) if d > 0 else "literal"))
        out.append((win[0][2] if win else None, rows))
    return out


def test_window_chain_cases_hold_what_they_claim():
    cs = {c.meta["kind"]: c for c in dc.cases("window_chains")}
    for c in cs.values():
        assert all(used <= 3 + 2 + 12 + 3 for used, _, _ in c.meta["trace"])
    # eight or more matches begin inside a 64-bit window, whatever its phase: every match is 4 bits long
    c = cs["many"]
    assert all(used == 4 for used, olen, d in c.meta["trace"] if d > 0)
    assert max(sum(1 for r in rows if r[3] > 0) for _, rows in _window_view(c)) >= 16
    # more than four independent matches in one window, near and far ones in one batch of four
    views = _window_view(cs["batch"])
    best = max(views, key=lambda v: sum(1 for r in v[1] if r[4].startswith("batch")))
    ind = [r[4] for r in best[1] if r[4].startswith("batch")]
    assert len(ind) > 4 and {"batch_near", "batch_far"} <= set(ind[:4])
    # a match whose source is another match's output of the same window; it goes the ordinary way although it is short
    views = _window_view(cs["dependent"])
    dep = [(wpos, r) for wpos, rows in views for r in rows if r[3] > 0 and r[2] <= 64 and r[1] > 0 and r[3] < r[1] + r[2] and r[3] > 3]
    assert dep and all(r[4] == "near" for _, r in dep)
    assert all(wpos + r[1] - r[3] >= wpos for wpos, r in dep)                     # (the source begins inside the window's own output)
    assert any(r[4] == "run" and r[1] > 0 for _, rows in views for r in rows) and any(r[4] == "overlap" for _, rows in views for r in rows)
    assert any(r[4].startswith("batch") for _, rows in views for r in rows)
    # a 65-byte match between 64-byte ones, near and far
    views = _window_view(cs["65"])
    for far in (False, True):
        assert any([r[2] for r in rows[k:k + 3]] == [64, 65, 64] and (rows[k][3] > NEAR_MAX) == far and
                   [r[4][:5] for r in rows[k:k + 3]] == ["batch", "far" if far else "near", "batch"][:3]
                   for _, rows in views for k in range(len(rows) - 2)), far
    # the cut
    views = _window_view(cs["tmax_eob"])
    assert len(views) == 1 and sum(r[2] for r in views[0][1]) == T_MAX == cs["tmax_eob"].meta["fill"]
    views = _window_view(cs["tmax_lit"])
    assert sum(r[2] for r in views[0][1]) == T_MAX and views[1][1][0][4] == "literal"       # the literal is cut off: it begins the next window
    views = _window_view(cs["tmax_plus_1"])
    assert cs["tmax_plus_1"].meta["fill"] == T_MAX + 1 and sum(r[2] for r in views[0][1]) < T_MAX and views[1][1][0][3] > 0
    assert views[1][1][1][4] == "literal"
    views = _window_view(cs["max"])
    trace = cs["max"].meta["trace"]
    assert all(used == 2 and olen == 258 for used, olen, d in trace if d > 0)
    assert all(sum(r[2] for r in rows) == 258 * (T_MAX // 258) for _, rows in views[:20])  # 32 matches begin in the window, three are taken


def test_code_shape_cases_hold_what_they_claim():
    P_L, P_D = dc.K["LIT_P"], dc.K["DIST_P"]
    a, b = by_name("code_shapes", "unary_15_bits"), by_name("code_shapes", "full_alphabets_pool_overflow")
    for c in (a, b, by_name("other_encoder", "bam_block0_skewed")):
        ll, dl = c.meta["lit_lens"], c.meta["dist_lens"]
        assert dc.kraft(ll) == 32768 and dc.kraft(dl) == 32768 and max(ll) == 15 and max(dl) == 15, c
    for c in (a, b):
        ll, dl = c.meta["lit_lens"], c.meta["dist_lens"]
        lf, df = dc.token_freqs(c.meta["tokens"])
        # the shortest and the longest codes are all in use
        for lens, freq in ((ll, lf), (dl, df)):
            short = min(L for L in lens if L)
            assert all(freq[s] > 0 for s, L in enumerate(lens) if L in (short, 15)), c
        # a symbol that uses all 48 bits a lane's decode allows: 15 + 5 + 15 + 13
        n, d = c.meta["uses_48_bit_symbol"]
        ls, le, _ = dc.length_symbol(n)
        ds, de, _ = dc.distance_symbol(d)
        assert (n, d) in c.meta["tokens"] and ll[ls] + le + dl[ds] + de == 48
    # (A): the long codes fit the default pool and not the small one -- second-level tables in one form, the slow path in the other
    demand = dc.sub_table_demand(a.meta["lit_lens"], a.meta["dist_lens"])
    assert dc.K["SMALL_POOL"] < min(1 << (15 - P_L), 1 << (15 - P_D)) and demand <= dc.K["SUB_CAP"], demand
    # (B): more than the default pool -- some long codes through tables and some through the slow path there, too
    demand = dc.sub_table_demand(b.meta["lit_lens"], b.meta["dist_lens"])
    assert demand > dc.K["SUB_CAP"], demand
    assert all(L for L in b.meta["lit_lens"]) and all(L for L in b.meta["dist_lens"]) and len(b.meta["lit_lens"]) == 286 and len(b.meta["dist_lens"]) == 30
    assert dc.sub_table_demand(*[by_name("other_encoder", "bam_block0_skewed").meta[k] for k in ("lit_lens", "dist_lens")]) > dc.K["SUB_CAP"]
    # header fields: a 15-bit code asks for all 19 code-length codes; eight is the least a valid header can do with, four is refused
    assert dc.dynamic_header(dc.BitWriter(), dc.trim(a.meta["lit_lens"], 257), dc.trim(a.meta["dist_lens"], 1)) == 19
    assert by_name("code_shapes", "hclen_field_4").meta["n_cl"] == 8 and by_name("refused", "four_code_length_codes").meta["n_cl"] == 4
    assert len(by_name("code_shapes", "hlit257_hdist1_no_distance_code").meta["lit_lens"]) == 257
    rl = by_name("code_shapes", "run_length_symbols")
    syms = [s for s, _ in rl.meta["rl"]]
    assert (18, 127) in rl.meta["rl"] and any(syms[i:i + 2] == [17, 16] for i in range(len(syms))) and any(syms[i:i + 2] == [18, 16] for i in range(len(syms)))
    at = 0
    crossing = False
    for s, v in rl.meta["rl"]:
        n = 1 if s < 16 else 3 + v if s == 16 else (3 if s == 17 else 11) + v
        crossing = crossing or (s == 16 and at < rl.meta["n_lit"] < at + n)
        at += n
    assert crossing and s == 16                                                   # (and the last run ends the lengths)
    tok = by_name("code_shapes", "258_as_284_plus_31").meta["tokens"]
    assert sum(1 for t in tok if not isinstance(t, int) and t[0] == 258) == 3


def test_block_structure_and_size_cases_hold_what_they_claim():
    c = by_name("block_structure", "200_blocks")
    assert len(c.meta["types"]) == 200 and all(c.meta["types"].count(k) >= 66 for k in (0, 1, 2))
    assert sorted(x.meta["phase"] for x in dc.cases("block_structure") if "phase" in x.meta) == list(range(8))
    stored = sorted({x.meta["stored_len"] for x in dc.cases("block_structure") if "stored_len" in x.meta})
    assert stored == [0, 1, T_MAX - 1, T_MAX, T_MAX + 1, dc.MAX_CDATA - 5]
    assert {x.name for x in dc.cases("block_structure")} >= {"stored_len_0", "stored_len_0_not_final", "final_fixed_block_only_eob", "trailing_bytes"}
    c = by_name("block_structure", "ends_on_last_bit")
    assert c.meta["end_bit"] == 8 * len(c.cdata)
    assert sorted(len(x.payload) for x in dc.cases("sizes")) == [0, 1, 31, 32, 33, FLUSH - 1, FLUSH, FLUSH + 1, 65535, 65536]
    # the refused "distance t + 1" rows: first symbol, far into the member, inside a window (the ordinary way), on a long code
    c = by_name("refused", "dist_too_far_inside_window")
    (win,) = [w for w in dc.windows(c.meta["trace"], c.meta["wpos0"]) if any(i == c.meta["bad_index"] for i, _, _ in w)]
    (row,) = [(off, wpos) for i, off, wpos in win if i == c.meta["bad_index"]]
    used, olen, d = c.meta["trace"][c.meta["bad_index"]]
    assert row[0] > 0 and d == row[0] + row[1] + 1 and olen <= 64 and not dc.batch_branch(row[1], row[0], olen, d).startswith("batch")
    c = by_name("refused", "dist_too_far_on_long_code")
    assert c.meta["lit_lens"][c.meta["long_symbol"]] == 15
    assert [t for t in by_name("refused", "dist_too_far_first_symbol").cdata[:1]] and dc.positions([(3, 1)]) == [(0, 3, 1)]
