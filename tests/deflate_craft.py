"""A DEFLATE *writer* for tests (RFC 1951), and the table of crafted BGZF members the device inflate (csrc/hgx_inflate.hip) is pinned
with.  zlib's deflate writes only part of what the format allows -- no distance above 32 506, never 258 as symbol 284 + 31, code
lengths from real frequencies only -- and what other writers of BAM files emit lies outside it.  Here a stream is written from a
token list (int = literal, (length, distance) = match) under explicit code-length lists, with raw control over the header fields, so
that a test says exactly which (position, length, distance), which code shape and which defect the decoder meets.

The reference for every expectation is `host_verdict`: the rule of the project's host reader (inflate_one in csrc/hgx_bam.cpp)
written with Python's zlib.  `copy_branch`, `windows` and `sub_table_demand` restate -- as small pure functions, with the constants
read out of the kernel's source -- which path of the kernel a case takes, so that the host test can show that the table covers the
paths it claims.  No GPU in this file."""
import functools
import heapq
import os
import random
import re
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "hisat-genotype_amd", "csrc", "hgx_inflate.hip")


# ---- the kernel's constants ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def kernel_constants():
    """RING, FLUSH, T_MAX, NEAR_MAX, LIT_P, DIST_P, SUB_CAP as csrc/hgx_inflate.hip defines them (#define / constexpr lines)."""
    src = open(KERNEL_SOURCE).read()
    env = {}
    for name, val in re.findall(r"^#define\s+(HGX_INF_[A-Z]+)\s+(\d+)\s*$", src, flags=re.M):
        env.setdefault(name, int(val))
    for decl in re.findall(r"^constexpr\s+(?:int|uint32_t)\s+([^;]+);", src, flags=re.M):
        for item in decl.split(","):
            m = re.match(r"\s*([A-Za-z_]+)\s*=\s*(.+?)\s*$", item)
            if not m:
                continue
            expr = re.sub(r"\(uint32_t\)|(?<=\d)u\b", "", m.group(2))
            if re.fullmatch(r"[A-Za-z_0-9+\-*/ ()]+", expr):
                try:
                    env[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(env)))
                except (NameError, SyntaxError):
                    pass
    out = {k: env[k] for k in ("RING", "FLUSH", "T_MAX", "NEAR_MAX", "LIT_P", "DIST_P", "SUB_CAP")}
    out["SMALL_POOL"] = int(re.search(r"sub_cap\s*=\s*SMALL_POOL\s*\?\s*(\d+)u", src).group(1))
    return out


K = kernel_constants()
RING, FLUSH, T_MAX, NEAR_MAX = K["RING"], K["FLUSH"], K["T_MAX"], K["NEAR_MAX"]

# verdicts (include/hgx.h, hgx_bgzf_inflate_verdicts)
OK, BAD_BLOCK_TYPE, BAD_STORED, BAD_CODE, BAD_DIST, OVERRUN, BAD_SIZE, BAD_CRC, BAD_LENGTHS, INPUT_END = range(10)
ANY_BAD = -1                                   # (truncated members only: behind the cut the reader sees bytes that may decode to anything)
# what the host reader says -> the verdict.  The zlib messages and the container rules of host_verdict.
VERDICT_OF = {
    "invalid block type": BAD_BLOCK_TYPE,
    "invalid stored block lengths": BAD_STORED,
    "invalid distance too far back": BAD_DIST,
    "invalid distance code": BAD_CODE, "invalid literal/length code": BAD_CODE,
    "too many length or distance symbols": BAD_LENGTHS, "invalid code lengths set": BAD_LENGTHS, "invalid bit length repeat": BAD_LENGTHS,
    "invalid literal/lengths set": BAD_LENGTHS, "invalid distances set": BAD_LENGTHS, "invalid code -- missing end-of-block": BAD_LENGTHS,
    "more output than ISIZE": OVERRUN, "less output than ISIZE": BAD_SIZE, "wrong CRC": BAD_CRC,
    # the stream does not end inside the member's bytes (zlib raises nothing: it waits for more input)
    "stream incomplete": INPUT_END,
}


# ---- bits, codes ------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """Bits in DEFLATE's order: a field's least significant bit first; Huffman codes are handed over already reversed."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        self.bits(0, -self.n & 7)

    def nbits(self):
        return 8 * len(self.out) + self.n

    def raw(self, data):
        assert self.n % 8 == 0
        self.out += self.acc.to_bytes(self.n >> 3, "little") + bytes(data)
        self.acc = 0
        self.n = 0

    def bytes(self):
        k = (self.n + 7) >> 3
        return bytes(self.out) + self.acc.to_bytes(k, "little")


def canonical_codes(lens):
    """[(code reversed for the stream, length) or None per symbol] of the canonical code with these lengths (RFC 1951 3.2.2).  The
    lengths are taken as they are: an over-subscribed or incomplete list gets the codes the rule gives."""
    count = [0] * 17
    for L in lens:
        count[L] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for L in range(1, 17):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    out = []
    for L in lens:
        if L == 0:
            out.append(None)
            continue
        c = nxt[L] & ((1 << L) - 1)
        nxt[L] += 1
        out.append((int(format(c, "0%db" % L)[::-1], 2), L))
    return out


def kraft(lens):
    """Sum of 2^-L in units of 2^-15 (complete: 32768)."""
    return sum(1 << (15 - L) for L in lens if L)


def huffman_lens(freqs, limit=15):
    """Code lengths of a Huffman code for the symbols with freq > 0 (at least two of them get a code, so the set is complete); a code
    deeper than `limit` flattens the frequencies and tries again."""
    freqs = list(freqs)
    used = [s for s, f in enumerate(freqs) if f > 0]
    if len(used) < 2:
        for s in range(len(freqs)):
            if s not in used:
                used.append(s)
                freqs[s] = 1
            if len(used) == 2:
                break
    while True:
        heap = [(freqs[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        lens = [0] * len(freqs)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= limit:
            return lens
        freqs = [(f + 1) // 2 + 1 if f > 0 else 0 for f in freqs]


def shape_lens(shape, order, n):
    """Code lengths for n symbols: the multiset `shape` ({length: count}) handed out along `order` (symbols, the first gets the
    shortest code); symbols not in `order` get no code."""
    lens = [0] * n
    seq = [L for L in sorted(shape) for _ in range(shape[L])]
    assert len(seq) <= len(order)
    for s, L in zip(order, seq):
        lens[s] = L
    return lens


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(length, alt258=False):
    """(symbol, extra bits, extra value); alt258: 258 as symbol 284 with extra 31, which zlib's inflate accepts and its deflate never writes."""
    assert 3 <= length <= 258
    if length == 258 and alt258:
        return 284, 5, 31
    i = max(k for k in range(29) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


_LEN_SYM = [None] * 3 + [length_symbol(n) for n in range(3, 259)]


def expand(tokens):
    """The bytes a token list means (LZ77 expansion); raw-symbol tokens have no meaning and are not allowed here."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 1 <= dist <= len(out), (length, dist, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                seg = bytes(out[-dist:])
                out += (seg * (length // dist + 1))[:length]
    return bytes(out)


def positions(tokens):
    """[(target position, length, distance)] of the matches of a token list."""
    at, out = 0, []
    for t in tokens:
        if isinstance(t, int):
            at += 1
        else:
            out.append((at, t[0], t[1]))
            at += t[0]
    return out


# ---- block emitters ---------------------------------------------------------------------------------------------------------------------
# Tokens: int = literal; (length, distance) = match; ("L", symbol) = a raw literal/length symbol without extra bits;
# ("M", length, distance symbol, extra value) = a match with a raw distance symbol; ("B", value, n) = n raw bits.
def emit_symbols(bw, tokens, lit_lens, dist_lens, alt258=False, eob=True, trace=None):
    """The symbols of a Huffman block (and its end-of-block code).  trace (a list): gets (bits used, output length, distance or 0) per token
    and (bits, 0, -1) for the end-of-block code -- what the kernel's windows are made of."""
    lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
    for t in tokens:
        b0 = bw.nbits() if trace is not None else 0
        if isinstance(t, int):
            bw.bits(*lc[t])
            olen, d = 1, 0
        elif t[0] == "L":
            bw.bits(*lc[t[1]])
            olen, d = 0, 0
        elif t[0] == "B":
            bw.bits(t[1], t[2])
            olen, d = 0, 0
        else:
            if t[0] == "M":
                _, olen, ds, dv = t
                de, d = (DIST_EXTRA[ds] if ds < 30 else 0), 0
            else:
                olen, d = t
                ds, de, dv = distance_symbol(d)
            ls, le, lv = length_symbol(olen, alt258) if alt258 else _LEN_SYM[olen]
            bw.bits(*lc[ls])
            bw.bits(lv, le)
            bw.bits(*dc[ds])
            bw.bits(dv, de)
        if trace is not None:
            trace.append((bw.nbits() - b0, olen, d))
    if eob:
        b0 = bw.nbits()
        bw.bits(*lc[256])
        if trace is not None:
            trace.append((bw.nbits() - b0, 0, -1))


def fixed_block(bw, tokens, final=True, **kw):
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    emit_symbols(bw, tokens, FIXED_LIT, FIXED_DIST, **kw)


def stored_block(bw, data, final=True, length=None, nlen=None):
    """A stored block; `length` / `nlen` override the two 16-bit fields."""
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    n = len(data) if length is None else length
    bw.bits(n, 16)
    bw.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
    bw.raw(data)


def run_length_symbols(lens):
    """A plain greedy run-length coding of the code lengths: [(symbol, extra value)]."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
            continue
        out.append((v, 0))
        i += 1
        run -= 1
        while run >= 3:
            take = min(run, 6)
            out.append((16, take - 3))
            i += take
            run -= take
    return out


RL_EXTRA = {16: 2, 17: 3, 18: 7}


def complete_cl_lens(symbols_used):
    """A complete code-length code (<= 7 bits) for the run-length symbols in use: flat, the lower symbols a bit shorter."""
    used = sorted(set(symbols_used))
    if len(used) == 1:
        used.append(0 if used[0] != 0 else 1)          # (a one-code code-length code is refused by zlib: give it a partner)
    n = len(used)
    k = n.bit_length() - 1
    r = n - (1 << k)
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k if i < n - 2 * r else k + 1
    assert kraft(lens) == 32768 and max(lens) <= 7
    return lens


def dynamic_header(bw, lit_lens, dist_lens, final=True, hlit=None, hdist=None, n_cl=None, cl_lens=None, rl=None):
    """The header of a dynamic block.  lit_lens / dist_lens: the lengths that are sent (HLIT = len(lit_lens) - 257 and HDIST = len(dist_lens)
    - 1 unless the raw 5-bit fields hlit / hdist say otherwise); rl: the run-length symbols [(symbol, extra value)] (default: greedy);
    cl_lens: the 19 lengths of the code-length code (default: a flat complete code over the symbols in use); n_cl: how many of them
    are written (HCLEN + 4; default: up to the last non-zero one in the order of RFC 1951, at least 4)."""
    if rl is None:
        rl = run_length_symbols(list(lit_lens) + list(dist_lens))
    if cl_lens is None:
        cl_lens = complete_cl_lens([s for s, _ in rl])
    if n_cl is None:
        n_cl = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
    bw.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    bw.bits(n_cl - 4, 4)
    for i in range(n_cl):
        bw.bits(cl_lens[CL_ORDER[i]], 3)
    cc = canonical_codes(cl_lens)
    for s, v in rl:
        bw.bits(*cc[s])
        bw.bits(v, RL_EXTRA.get(s, 0))
    return n_cl


def dynamic_block(bw, tokens, lit_lens, dist_lens, final=True, alt258=False, eob=True, trace=None, **header):
    dynamic_header(bw, lit_lens, dist_lens, final, **header)
    emit_symbols(bw, tokens, list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens)), alt258=alt258, eob=eob, trace=trace)


def token_freqs(tokens):
    """(literal/length symbol counts [286] with one end-of-block, distance symbol counts [30]) of a token list."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[_LEN_SYM[t[0]][0]] += 1
            df[distance_symbol(t[1])[0]] += 1
    return lf, df


def huffman_block(bw, tokens, final=True, freqs=None, **kw):
    """A dynamic block under the Huffman code of the tokens' own frequencies (or of `freqs`); no distance code where there is no match."""
    lf, df = freqs or token_freqs(tokens)
    lit_lens, dist_lens = huffman_lens(lf), (huffman_lens(df) if any(df) else [0] * 30)
    dynamic_block(bw, tokens, trim(lit_lens, 257), trim(dist_lens, 1), final=final, **kw)
    return lit_lens, dist_lens


def trim(lens, least):
    """The list without its trailing zeros (at least `least` entries: HLIT / HDIST as small as the lengths allow)."""
    n = len(lens)
    while n > least and lens[n - 1] == 0:
        n -= 1
    return list(lens[:n])


# ---- the container ----------------------------------------------------------------------------------------------------------------------
BGZF_HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
EOF_MEMBER = BGZF_HEAD + b"\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"
MAX_MEMBER = 65536                       # (BSIZE is 16 bits: member size - 1)
MAX_CDATA = MAX_MEMBER - 26


def member(cdata, crc, isize):
    """A BGZF member around cdata with the CRC-32 and ISIZE given (right or wrong)."""
    assert len(cdata) + 26 <= MAX_MEMBER, len(cdata)
    return BGZF_HEAD + struct.pack("<H", len(cdata) + 25) + bytes(cdata) + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def good_member(payload, stored=False):
    bw = BitWriter()
    if stored:
        stored_block(bw, payload)
    else:
        fixed_block(bw, list(payload))
    return member(bw.bytes(), zlib.crc32(payload), len(payload))


def host_verdict(cdata, crc, isize):
    """(ok, payload or None, message or None): the host reader's rule for one member (inflate_one in csrc/hgx_bam.cpp).  ISIZE 0 is
    accepted without decoding; otherwise a raw inflate must reach the end of the stream within ISIZE bytes of output, the output must be
    exactly ISIZE bytes with the CRC-32 given; bytes behind the final block are accepted.  The message is zlib's own where zlib
    raises one, else the container rule that failed."""
    if isize == 0:
        return True, b"", None
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(cdata), isize + 1)
    except zlib.error as e:
        return False, None, str(e).split(": ", 1)[-1]
    if len(out) > isize:
        return False, None, "more output than ISIZE"
    if not d.eof:
        return False, None, "stream incomplete"
    if len(out) < isize:
        return False, None, "less output than ISIZE"
    if zlib.crc32(out) & 0xFFFFFFFF != crc & 0xFFFFFFFF:
        return False, None, "wrong CRC"
    return True, out, None


# ---- which path of the kernel -----------------------------------------------------------------------------------------------------------
def copy_branch(t, length, dist):
    """The branch of copy_match (k_bgzf_inflate_w) a match of `length` bytes at output position t from `dist` back takes."""
    if dist >= length and dist <= NEAR_MAX:
        return "near"
    if dist == 1:
        return "run"
    if dist < length:
        return "overlap"
    return "far"


def batch_branch(wpos, my_off, length, dist):
    """A match inside a window that began at output position wpos, my_off bytes into the window's output: the independent batch
    (four at a time, reads before writes; ring or memory) or the ordinary way through copy_match."""
    if length <= 64 and my_off + length <= dist and dist <= wpos + my_off:
        return "batch_near" if dist <= NEAR_MAX else "batch_far"
    return copy_branch(wpos + my_off, length, dist)


def windows(trace, wpos=0):
    """The windows k_bgzf_inflate_w cuts a block's symbols into, when every symbol is decoded by its lane (codes within the tables):
    a window takes the symbols that START within 64 bits of its first one, stops on the end-of-block code and is cut in front of the
    symbol with which its output would pass T_MAX.  trace: emit_symbols'.  Returns [[(index in trace, my_off, wpos of the window)]]."""
    out, i = [], 0
    while i < len(trace):
        cur, off, win = 0, 0, []
        while i < len(trace) and cur < 64:
            used, olen, d = trace[i]
            if d == -1:                                 # end of block: the window ends on it
                i += 1
                cur = 64
                break
            if off + olen > T_MAX:
                break
            win.append((i, off, wpos))
            off += olen
            cur += used
            i += 1
        out.append(win)
        wpos += off
    return out


def prefix_tables(lens, P):
    """{P-bit prefix: longest code length under it} for the codes longer than P bits."""
    out = {}
    for c in canonical_codes(lens):
        if c and c[1] > P:
            pre = c[0] & ((1 << P) - 1)                  # (reversed code: its first P bits are the low ones)
            out[pre] = max(out.get(pre, 0), c[1])
    return out


def sub_table_demand(lit_lens, dist_lens):
    """Entries of the second-level pool the two codes ask for: one table of 2^(longest - P) entries per distinct P-bit prefix."""
    return (sum(1 << (L - K["LIT_P"]) for L in prefix_tables(lit_lens, K["LIT_P"]).values()) +
            sum(1 << (L - K["DIST_P"]) for L in prefix_tables(dist_lens, K["DIST_P"]).values()))


# ---- another encoder -------------------------------------------------------------------------------------------------------------------
def lz_parse(data, max_chain=4):
    """A small greedy hash-chain parser with the whole 32 768-byte window (no 262-byte margin as in zlib): a token list."""
    n, head, prev, tokens, i = len(data), {}, [-1] * len(data), [], 0
    while i < n:
        best, best_d = 0, 0
        if i + 3 <= n:
            j, chain, m = head.get(data[i:i + 3], -1), 0, min(258, n - i)
            while j >= 0 and i - j <= 32768 and chain < max_chain:
                l = 3
                while l < m and data[j + l:j + l + 16] == data[i + l:i + l + 16]:
                    l += 16
                while l < m and data[j + l] == data[i + l]:
                    l += 1
                l = min(l, m)
                if l > best or (l == best and chain == 0):
                    best, best_d = l, i - j
                j, chain = prev[j], chain + 1
        step = best if best >= 3 else 1
        tokens.append((best, best_d) if best >= 3 else data[i])
        for k in range(i, min(i + step, n - 2)):
            key = data[k:k + 3]
            prev[k] = head.get(key, -1)
            head[key] = k
        i += step
    return tokens


# ---- code shapes -------------------------------------------------------------------------------------------------------------------------
def unary_lens(symbols, n):
    """Lengths 1, 2, ..., k-1, k-1 over the given symbols in this order (Kraft-complete; 16 symbols reach 15 bits)."""
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    return lens


# every literal/length symbol and every distance symbol has a code; 15-bit codes in both; the long codes ask for more second-level
# entries than the default pool has
FULL_LIT_SHAPE = {4: 8, 6: 16, 8: 32, 10: 64, 11: 100, 12: 50, 13: 9, 14: 5, 15: 2}
FULL_DIST_SHAPE = dict([(L, 2) for L in range(2, 15)] + [(15, 4)])


def full_lens(lit_order=None, dist_order=None):
    lit_order = list(range(286)) if lit_order is None else lit_order
    dist_order = list(range(30)) if dist_order is None else dist_order
    return shape_lens(FULL_LIT_SHAPE, lit_order, 286), shape_lens(FULL_DIST_SHAPE, dist_order, 30)


def by_frequency(tokens):
    """Symbol orders (most frequent first, every symbol present) of a token list: for full_lens."""
    lf, df = token_freqs(tokens)
    return sorted(range(286), key=lambda s: (-lf[s], s)), sorted(range(30), key=lambda s: (-df[s], s))


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
class Case:
    """One member.  valid: payload is what it inflates to.  Invalid: `why` is the zlib message (or the container rule) host_verdict
    gives, `verdict` the INF_* value -- VERDICT_OF[why] unless the row says otherwise; `form_verdict`: {form: (verdict, reason)} where a
    form of the kernel reaches another check first."""

    def __init__(self, group, name, cdata, payload=None, why=None, crc=None, isize=None, verdict=None, form_verdict=None, **meta):
        self.group, self.name, self.cdata, self.payload, self.why = group, name, bytes(cdata), payload, why
        self.valid = why is None
        self.crc = (zlib.crc32(payload) if payload is not None else 0) if crc is None else crc
        self.isize = len(payload) if isize is None else isize
        self.verdict = OK if self.valid else (VERDICT_OF[why] if verdict is None else verdict)
        self.form_verdict = form_verdict or {}
        self.meta = meta

    def member(self):
        return member(self.cdata, self.crc, self.isize)

    def __repr__(self):
        return "%s/%s" % (self.group, self.name)


def _literals(rng, n, alphabet=256):
    return [rng.randrange(alphabet) for _ in range(n)]


def _fixed(tokens, **kw):
    bw = BitWriter()
    fixed_block(bw, tokens, **kw)
    return bw.bytes()


def _valid_cases():
    rng = random.Random(1951)
    cases = []

    def add(group, name, cdata, tokens=None, payload=None, **meta):
        if payload is None:
            payload = expand(tokens)
        cases.append(Case(group, name, cdata, payload, tokens=tokens, **meta))

    # -- distances zlib never writes: 32 768 literals, then matches at 32 768, 32 767 and 32 507 of lengths 3 and 258
    tokens = _literals(rng, 32768)
    for d in (32768, 32767, 32507):
        for n in (3, 258):
            tokens.append((n, d))
            tokens.append(rng.randrange(256))
    add("far_distances", "fixed", _fixed(tokens), tokens)
    bw = BitWriter()
    lit_lens, dist_lens = huffman_block(bw, tokens)
    add("far_distances", "dynamic", bw.bytes(), tokens, lit_lens=lit_lens, dist_lens=dist_lens)

    # -- the near/far switch and the ring's wrap: every distance around NEAR_MAX and RING with every length, at target positions 0, 1 and
    #    FLUSH - 1 modulo FLUSH, and where the match straddles a flush boundary / the ring's wrap; a literal between two matches
    # (RING - 258 / RING - 257: where round 4's form, k_bgzf_inflate, switches from its ring to memory)
    dists = (NEAR_MAX - 1, NEAR_MAX, NEAR_MAX + 1, RING - T_MAX, RING - 258, RING - 257, RING - 1, RING, RING + 1)
    lengths = (3, 63, 64, 65, 258)
    wanted = []
    for d in dists:
        for n in lengths:
            for mod, res in ((FLUSH, 0), (FLUSH, 1), (FLUSH, FLUSH - 1), (FLUSH, FLUSH - max(1, n // 2)), (RING, RING - max(1, n // 2))):
                wanted.append((n, d, mod, res))
    tokens, at, part = [], 0, 0

    def close_switch():
        nonlocal tokens, at, part
        if tokens:
            add("near_far_switch", "part%d" % part, _fixed(tokens), tokens)
            part += 1
        tokens, at = [], 0
    for n, d, mod, res in wanted:
        start = max(at + 1, d)
        start += (res - start) % mod
        if start + n + 1 > 60000:                     # (about 9 bits per literal: the member stays below 64 KB)
            close_switch()
            start = d + (res - d) % mod
        tokens += _literals(rng, start - at)
        tokens.append((n, d))
        at = start + n
    close_switch()

    # -- overlapping copies: every distance 1..257 with lengths 258 and 257; dist == len and len +- 1
    tokens, part = _literals(rng, 300), 0
    size = 300
    for d in range(1, 258):
        for n in (258, 257):
            if size + n + 1 > 65000:
                add("overlap", "part%d" % part, _fixed(tokens), tokens)
                part += 1
                tokens, size = _literals(rng, 300), 300
            tokens += [(n, d), rng.randrange(256)]
            size += n + 1
    add("overlap", "part%d" % part, _fixed(tokens), tokens)
    tokens = _literals(rng, 300)
    for n in (3, 64, 65, 258):
        for d in (n - 1, n, n + 1):
            tokens += [(n, d), rng.randrange(256)]
    add("overlap", "dist_eq_len", _fixed(tokens), tokens)

    # -- window chains: codes of 1-3 bits for everything in use, so that a 64-bit window holds many matches
    lit_lens = [0] * 286
    for s, L in ((276, 2), (285, 2), (257, 2), (120, 3), (256, 3)):       # lengths 59..66, 258, 3; the literal 'x'
        lit_lens[s] = L
    dist_lens = [0] * 30
    for s in (0, 2, 17, 26):                                              # distances 1, 3, 385..512, 8193..12288: 2 bits each
        dist_lens[s] = 2
    assert kraft(lit_lens) == 32768 and kraft(dist_lens) == 32768
    head = _literals(rng, 12288 + 300)

    def chain_case(name, body, **meta):
        bw = BitWriter()
        fixed_block(bw, head, final=False)
        trace = []
        dynamic_block(bw, body, trim(lit_lens, 257), trim(dist_lens, 1), trace=trace)
        add("window_chains", name, bw.bytes(), head + body, trace=trace, wpos0=len(head), **meta)
    chain_case("eight_matches", [(3, 1), (3, 3)] * 40 + [120], kind="many")
    chain_case("independent_batch", ([(64, 400), (64, 9000), (64, 385), (64, 512), (64, 8193), (64, 12288), 120] * 6), kind="batch")
    # (six overlapping matches make 396 bytes; the seventh reads from 385 back: its source is what the window itself wrote)
    chain_case("dependent_in_window", ([(66, 3)] * 6 + [(64, 385), (3, 1), (64, 9000), 120]) * 6, kind="dependent")
    chain_case("65_between_64", ([(64, 450), (65, 450), (64, 450), (64, 9500), (65, 9500), (64, 9500), 120] * 6), kind="65")
    fill = [(258, 1)] * 3 + [(66, 3), (66, 3), (59, 3), (59, 3)]                  # 40 bits that make 1024 bytes
    fill1 = [(258, 1)] * 3 + [(66, 3), (66, 3), (60, 3), (59, 3)]                 # ... and 1025
    chain_case("window_of_exactly_tmax_then_eob", fill, kind="tmax_eob", fill=sum(t[0] for t in fill))
    chain_case("window_of_tmax_then_literal", fill + [120] + fill + [120, 120], kind="tmax_lit", fill=sum(t[0] for t in fill))
    chain_case("window_of_tmax_plus_1", fill1 + [120] + fill1 + [120], kind="tmax_plus_1", fill=sum(t[0] for t in fill1))
    # 258-byte matches at 2 bits each: a window could ask for 32 of them
    lit2, dist2 = [0] * 286, [0] * 30
    lit2[285], lit2[120], lit2[256] = 1, 2, 2
    dist2[0], dist2[1] = 1, 1
    bw = BitWriter()
    fixed_block(bw, head[:100], final=False)
    body = ([(258, 1), (258, 2)] * 40 + [120]) * 2
    trace = []
    dynamic_block(bw, body, trim(lit2, 257), trim(dist2, 1), trace=trace)
    add("window_chains", "cut_maximum", bw.bytes(), head[:100] + body, trace=trace, wpos0=100, kind="max")

    # -- code shapes
    # (A) 15-bit codes in both alphabets, every code in use, the long ones within the default pool (and beyond the pool of 32)
    lit_syms = [65, 285, 257, 66, 258, 67, 265, 68, 273, 69, 256, 70, 281, 71, 284, 72]      # 1, 2, ... 14, 15, 15 bits
    dist_syms = [0, 3, 1, 8, 16, 2, 20, 24, 4, 10, 27, 12, 28, 14, 26, 29]
    la, da = unary_lens(lit_syms, 286), unary_lens(dist_syms, 30)
    body = []
    for rep in range(3):
        body += [65, 66, 67, 68, 69, 70, 71, 72] * 4
        for n, ds in ((258, 0), (3, 3), (4, 1), (11, 8), (35, 16), (131, 2), (257, 20), (162, 24), (3, 4), (258, 10)):
            body.append((n, DIST_BASE[ds]))
        body += [(257, 32768), 72, (258, 24577), 71, (36, 12289 + rep), (12, 16385 + 5000), (150, 8193 + 77), (3, 65 + 31), (4, 129 + 63)]
    pre = _literals(rng, 32768, 8)
    pre_l = [65 + v for v in pre]
    bw = BitWriter()
    dynamic_block(bw, pre_l, trim(unary_lens([65, 66, 67, 68, 69, 70, 71, 72, 256], 286), 257), [0], final=False)
    dynamic_block(bw, body, trim(la, 257), trim(da, 1))
    add("code_shapes", "unary_15_bits", bw.bytes(), pre_l + body, lit_lens=la, dist_lens=da, uses_48_bit_symbol=(257, 32768))
    # (B) every symbol of both alphabets has a code; more second-level entries than the default pool holds
    order_l = [s for s in range(286) if s not in (255, 284)] + [255, 284]            # (15 bits: the literal 255 and length symbol 284)
    order_d = [s for s in range(30) if s not in (0, 29)] + [0, 29]
    lb, db = full_lens(order_l, order_d)
    body = _literals(rng, 33000) + [255] * 3
    for s in range(257, 286):
        body += [(LEN_BASE[s - 257], 1 + s), s & 255]
    for ds in range(30):
        body += [(3 + ds, DIST_BASE[ds]), (258, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1), ds]
    body += [(257, 32768), 255, (257, 24577), (131, 32768)]
    bw = BitWriter()
    dynamic_block(bw, body, lb, db)
    add("code_shapes", "full_alphabets_pool_overflow", bw.bytes(), body, lit_lens=lb, dist_lens=db, uses_48_bit_symbol=(257, 32768))
    # header fields at their ends
    bw = BitWriter()
    l257 = unary_lens([97, 98, 256], 257)
    dynamic_block(bw, [97, 98, 97, 97], l257, [0])                              # HLIT 257, HDIST 1: no distance code, literals only
    add("code_shapes", "hlit257_hdist1_no_distance_code", bw.bytes(), [97, 98, 97, 97], lit_lens=l257, dist_lens=[0])
    bw = BitWriter()
    tok = [97] * 9 + [(5, 1), (258, 7), 98]
    dynamic_block(bw, tok, unary_lens([97, 98, 256, 259, 285], 286), unary_lens([0, 5, 29], 30))      # HLIT 286, HDIST 30
    add("code_shapes", "hlit286_hdist30", bw.bytes(), tok)
    bw = BitWriter()
    tok = [97] * 4 + [(6, 1), (3, 1), 97]
    one = [0] * 30
    one[0] = 1
    dynamic_block(bw, tok, unary_lens([97, 256, 257, 260], 261), trim(one, 1))
    add("code_shapes", "one_distance_code_of_one_bit", bw.bytes(), tok)
    bw = BitWriter()                                                            # only the end-of-block code, one bit; an empty non-final block
    eob_only = [0] * 256 + [1]
    dynamic_block(bw, [], eob_only, [0], final=False)
    fixed_block(bw, [104, 105])
    add("code_shapes", "single_eob_code_in_empty_block", bw.bytes(), [104, 105])
    # HCLEN: 19 code-length codes (symbol 15 is the last in RFC 1951's order, so a 15-bit code asks for all of them) is what the two
    # sets above send.  FOUR code-length codes name only 16, 17, 18 and 0: every length would be 0 and there is no end-of-block code --
    # that header is among the refused rows.  The shortest header that can be valid has the HCLEN FIELD 4: eight codes, 16 17 18 0 8 7
    # 9 6; no complete distance code exists over 6..9 bits and 30 symbols, so the block has literals only.
    l8 = [0] * 257
    for s in range(32, 94):
        l8[s] = 6
    l8[10] = l8[256] = 7
    for s in (94, 95, 96, 97):
        l8[s] = 8
    assert kraft(l8) == 32768
    tok = [32 + rng.randrange(66) for _ in range(80)] + [10]
    bw = BitWriter()
    n_cl = dynamic_header(bw, l8, [0], cl_lens=complete_cl_lens([16, 17, 18, 0, 8, 7, 9, 6]))
    emit_symbols(bw, tok, l8 + [0] * 31, [0] * 32)
    add("code_shapes", "hclen_field_4", bw.bytes(), tok, n_cl=n_cl)
    # the run-length symbols: a 16 that carries a literal length into the distance lengths; a 16 directly after a 17 and after an 18
    # (it repeats zero); an 18 with 138; the last run ends exactly at HLIT + HDIST
    lr = [0] * 260
    lr[0] = lr[1] = 2
    lr[256] = lr[257] = lr[258] = lr[259] = 3                                   # 2/4 + 4/8 = 1
    dr = [3, 3, 3, 3, 3, 3, 3, 3]                                               # 8/8
    # "2 2"; 17: three zeros; 16 behind it: three more; 18 + 127: 138 zeros; 18: 107 zeros; 16 behind it: three zeros -- 254 zeros, up to
    # symbol 255; then a 3 and two 16s that repeat it eleven times: across the end of the literal lengths (260) to the very last length
    rl = [(2, 0), (2, 0), (17, 0), (16, 0), (18, 127), (18, 107 - 11), (16, 0), (3, 0), (16, 3), (16, 2)]
    got = []
    for s, v in rl:
        got += [s] if s < 16 else [got[-1]] * (3 + v) if s == 16 else [0] * ((3 if s == 17 else 11) + v)
    assert got == lr + dr, (len(got), len(lr) + len(dr))
    tok = [0, 1, 1, 0, (3, 1), (5, 5), (4, 8), 0]
    bw = BitWriter()
    dynamic_block(bw, tok, lr, dr, rl=rl, cl_lens=complete_cl_lens([s for s, _ in rl]))
    add("code_shapes", "run_length_symbols", bw.bytes(), tok, rl=rl, n_lit=len(lr))
    tok = _literals(rng, 300) + [(258, 300), 7, (258, 1), (258, 257), 9]
    add("code_shapes", "258_as_284_plus_31", _fixed(tok, alt258=True), tok)

    # -- block structure
    bw, tok_all, types, size = BitWriter(), [], [], 0
    for i in range(200):
        tok = _literals(rng, rng.randrange(0, 12), 6)
        kind = i % 3
        if size > 40 and kind:
            tok.append((rng.randrange(3, 40), rng.randrange(1, 40)))
        size += sum(1 if isinstance(t, int) else t[0] for t in tok)
        if kind == 0:
            stored_block(bw, bytes(tok), final=i == 199)
        elif kind == 1:
            fixed_block(bw, tok, final=i == 199)
        else:
            huffman_block(bw, tok, final=i == 199)
        types.append(kind)
        tok_all += tok
    add("block_structure", "200_blocks", bw.bytes(), tok_all, types=types)
    phases = []
    for nine in range(8):                                                     # a 9-bit literal more moves the stored block's header by one bit
        bw = BitWriter()
        tok = [65, 66, 67] + [200] * nine
        fixed_block(bw, tok, final=False)
        phases.append((bw.nbits() + 3) % 8)
        data = bytes(_literals(rng, 50))
        stored_block(bw, data, final=False)
        fixed_block(bw, [68])
        add("block_structure", "stored_at_bit_phase_%d" % phases[-1], bw.bytes(), payload=bytes(tok) + data + b"D", phase=phases[-1])
    assert sorted(phases) == list(range(8))
    for n in (0, 1, T_MAX - 1, T_MAX, T_MAX + 1):
        for final in (False, True):
            if n and not final:
                continue
            bw = BitWriter()
            pre = _literals(rng, FLUSH - T_MAX // 2)                           # (the larger ones cross a flush boundary)
            fixed_block(bw, pre, final=False)
            data = bytes(_literals(rng, n))
            stored_block(bw, data, final=final)
            if not final:
                fixed_block(bw, [33])
            add("block_structure", "stored_len_%d%s" % (n, "" if final else "_not_final"), bw.bytes(), payload=bytes(pre) + data + (b"" if final else b"!"), stored_len=n)
    data = bytes(_literals(rng, MAX_CDATA - 5))
    bw = BitWriter()
    stored_block(bw, data)
    add("block_structure", "stored_largest", bw.bytes(), payload=data, stored_len=len(data))
    bw = BitWriter()
    stored_block(bw, b"abc", final=False)
    fixed_block(bw, [])
    add("block_structure", "final_fixed_block_only_eob", bw.bytes(), payload=b"abc")
    bw = BitWriter()
    tok = [65] * 5 + [200] * 6                                                # 3 + 5 * 8 + 6 * 9 + 7 = 104 bits
    fixed_block(bw, tok)
    assert bw.nbits() % 8 == 0
    add("block_structure", "ends_on_last_bit", bw.bytes(), tok, end_bit=bw.nbits())
    add("block_structure", "trailing_bytes", _fixed(tok) + bytes(_literals(rng, 7)), tok, trailing=7)

    # -- sizes: the pieces of the last flush and the CRC join
    for n in (1, 31, 32, 33, FLUSH - 1, FLUSH, FLUSH + 1, 65535, 65536):
        tok = _literals(rng, min(n, 20000))
        size = len(tok)
        while size < n:
            ln = min(n - size, rng.randrange(3, 259))
            if ln < 3:
                tok += _literals(rng, ln)
            else:
                tok.append((ln, rng.randrange(1, min(size, 32768) + 1)))
            size += ln
        add("sizes", "payload_%d" % n, _fixed(tok), tok)
    tok = _literals(rng, 100) + [(50, 20)]
    cases.append(Case("sizes", "isize_0_stream_not_empty", _fixed(tok), b"", crc=0, isize=0, tokens=tok))
    return cases


@functools.lru_cache(None)
def bam_payload_blocks(n_blocks=2, size=0xff00):
    """The first n_blocks * size bytes of a fixture's BAM payload (uncompressed), in blocks of `size`."""
    import tempfile
    import golden_util as gu
    from hisatgenotype_amd import bamio
    fx = gu.load("hla_mid_real")
    loc = fx["_locus"]
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "fixture.bam")
        bamio.write_bam(p, fx["sam"], [(loc.ref_allele, len(loc.backbone))])
        payload = b"".join(bamio._bgzf_blocks(open(p, "rb").read()))
    assert len(payload) >= n_blocks * size, len(payload)
    return [payload[i * size:(i + 1) * size] for i in range(n_blocks)]


def _other_encoder_cases():
    """A BAM's payload as another encoder would write it: a greedy parse over the whole 32 768-byte window, once under the fixed codes
    and once under the full skewed set (FULL_*_SHAPE, the frequent symbols the short codes)."""
    cases = []
    for i, raw in enumerate(bam_payload_blocks()):
        tokens = lz_parse(raw)
        assert expand(tokens) == raw
        cases.append(Case("other_encoder", "bam_block%d_fixed" % i, _fixed(tokens), raw, tokens=tokens))
        lit_lens, dist_lens = full_lens(*by_frequency(tokens))
        bw = BitWriter()
        dynamic_block(bw, tokens, lit_lens, dist_lens)
        cases.append(Case("other_encoder", "bam_block%d_skewed" % i, bw.bytes(), raw, tokens=tokens, lit_lens=lit_lens, dist_lens=dist_lens))
    return cases


# Chain-window code of the refused "distance t + 1 inside a window" row (the set of the window_chains group)
def _chain_lens():
    lit_lens, dist_lens = [0] * 286, [0] * 30
    for s, L in ((276, 2), (285, 2), (257, 2), (120, 3), (256, 3)):
        lit_lens[s] = L
    for s in (0, 2, 17, 26):
        dist_lens[s] = 2
    return lit_lens, dist_lens


def _invalid_cases():
    rng = random.Random(1952)
    cases = []

    def add(name, cdata, why, isize, crc=0, **kw):
        cases.append(Case("refused", name, cdata, None, why, crc=crc, isize=isize, **kw))
    lits = _literals(rng, 40)
    # block type 3, behind a good block
    bw = BitWriter()
    fixed_block(bw, lits, final=False)
    bw.bits(1, 1)
    bw.bits(3, 2)
    bw.bits(0, 13)
    add("block_type_3", bw.bytes(), "invalid block type", 40)
    # stored blocks
    bw = BitWriter()
    stored_block(bw, bytes(lits), nlen=(40 ^ 0xFFFF) ^ 0x0100)
    add("stored_nlen_wrong", bw.bytes(), "invalid stored block lengths", 40)
    bw = BitWriter()
    stored_block(bw, bytes(lits), length=140)                                # 100 bytes more than the member holds; ISIZE agrees with LEN
    add("stored_len_past_member", bw.bytes(), "stream incomplete", 140)
    # a Huffman block whose last byte is missing from the member -- and the byte that follows, the first of the CRC-32 field, happens to
    # be that byte: a reader that looks beyond the member sees a whole stream with the right size and CRC-32
    for last in range(256 * 64):
        tok = lits + [last & 255, last >> 8]
        cdata = _fixed(tok)
        if zlib.crc32(bytes(tok)) & 0xFF == cdata[-1]:
            break
    assert member(cdata[:-1], zlib.crc32(bytes(tok)), 42)[18:18 + len(cdata)] == cdata           # (the member's bytes spell the whole stream)
    add("final_block_ends_in_footer", cdata[:-1], "stream incomplete", 42, crc=zlib.crc32(bytes(tok)), whole=cdata)
    bw = BitWriter()
    stored_block(bw, bytes(lits))
    add("stored_len_past_isize", bw.bytes(), "more output than ISIZE", 39, crc=zlib.crc32(bytes(lits[:39])))
    # a distance one byte beyond the member's first byte
    add("dist_too_far_first_symbol", _fixed([(3, 1)]), "invalid distance too far back", 3)
    tok = _literals(rng, 5000) + [(10, 5001), 1, 2]
    add("dist_too_far_after_5000", _fixed(tok), "invalid distance too far back", 5012)
    lit_lens, dist_lens = _chain_lens()
    head = _literals(rng, 390)
    body = [(3, 1), (3, 3), (64, 397), (3, 1), 120]                             # the third match stands at 396 and reaches 397 back
    bw = BitWriter()
    fixed_block(bw, head, final=False)
    trace = []
    dynamic_block(bw, body, trim(lit_lens, 257), trim(dist_lens, 1), trace=trace)
    add("dist_too_far_inside_window", bw.bytes(), "invalid distance too far back", 390 + 3 + 3 + 64 + 3 + 1, trace=trace, wpos0=390, bad_index=2)
    order_l = [s for s in range(286) if s not in (255, 284)] + [255, 284]
    lb, db = full_lens(order_l)
    tok = _literals(rng, 100) + [(257, 101), 5]
    bw = BitWriter()
    dynamic_block(bw, tok, lb, db)
    add("dist_too_far_on_long_code", bw.bytes(), "invalid distance too far back", 358, lit_lens=lb, dist_lens=db, long_symbol=284)
    # symbols that have a code and no meaning
    for ds in (30, 31):
        add("fixed_distance_symbol_%d" % ds, _fixed(lits + [("M", 3, ds, 0), 7]), "invalid distance code", 44)
    for ls in (286, 287):
        add("fixed_length_symbol_%d" % ls, _fixed(lits + [("L", ls), 7]), "invalid literal/length code", 44)
    # bits that are no code: the other bit of a one-code set; any bits where there is no distance code
    one = [1]
    bw = BitWriter()
    dynamic_block(bw, [97] * 4 + [("L", 257), ("B", 1, 1), 97], unary_lens([97, 256, 257, 260], 261), one)
    add("one_code_distance_set_other_bit", bw.bytes(), "invalid distance code", 8)
    bw = BitWriter()
    fixed_block(bw, lits, final=False)
    dynamic_block(bw, [("B", 1, 1), ("B", 0, 7)], [0] * 256 + [1], [0])
    add("one_code_literal_set_other_bit", bw.bytes(), "invalid literal/length code", 40)
    bw = BitWriter()
    dynamic_block(bw, [97] * 4 + [("L", 257), ("B", 0, 8), 97], unary_lens([97, 256, 257, 260], 261), [0])
    add("match_without_distance_code", bw.bytes(), "invalid distance code", 8)
    # header fields beyond their range
    good_l, good_d = unary_lens([97, 98, 256, 257], 286), unary_lens([0, 1, 2], 30)
    for n_lit in (287, 288):
        bw = BitWriter()
        dynamic_block(bw, [97, 98, 97], good_l + [0] * (n_lit - 286), good_d, hlit=n_lit - 257)
        add("hlit_%d" % n_lit, bw.bytes(), "too many length or distance symbols", 3)
    for n_dist in (31, 32):
        bw = BitWriter()
        dynamic_block(bw, [97, 98, 97], good_l, good_d + [0] * (n_dist - 30), hdist=n_dist - 1)
        add("hdist_%d" % n_dist, bw.bytes(), "too many length or distance symbols", 3)
    # over-subscribed and incomplete sets of lengths, in each of the three alphabets
    gl, gd = trim(good_l, 257), trim(good_d, 1)
    for name, cl in (("over_subscribed", {0: 1, 1: 1, 2: 1, 3: 2}), ("incomplete", {0: 2, 1: 2, 2: 2, 3: 3})):
        cl_lens = [0] * 19
        for s, L in cl.items():
            cl_lens[s] = L
        bw = BitWriter()
        dynamic_block(bw, [97], gl, gd, cl_lens=cl_lens, rl=[(v, 0) for v in gl + gd])
        add("code_length_code_" + name, bw.bytes(), "invalid code lengths set", 1)
    for name, lens in (("over_subscribed", {97: 1, 98: 1, 256: 1}), ("incomplete", {97: 2, 256: 2})):
        ll = [0] * 257
        for s, L in lens.items():
            ll[s] = L
        bw = BitWriter()
        dynamic_block(bw, [97], ll, gd)
        add("literal_set_" + name, bw.bytes(), "invalid literal/lengths set", 1)
    for name, lens in (("over_subscribed", [1, 1, 1]), ("incomplete", [2, 2])):
        bw = BitWriter()
        dynamic_block(bw, [97], gl, lens)
        add("distance_set_" + name, bw.bytes(), "invalid distances set", 1)
    # the run-length symbols
    rl_good = run_length_symbols(gl + gd)
    cl_all = complete_cl_lens([s for s, _ in rl_good] + [16, 18])
    bw = BitWriter()
    dynamic_block(bw, [97], gl, gd, rl=[(16, 0)] + rl_good, cl_lens=cl_all)
    add("repeat_16_first", bw.bytes(), "invalid bit length repeat", 1)
    bw = BitWriter()
    dynamic_block(bw, [97], gl, gd, rl=rl_good[:-1] + [(18, 127)], cl_lens=cl_all)
    add("repeat_past_hlit_hdist", bw.bytes(), "invalid bit length repeat", 1)
    no_eob = list(gl)
    no_eob[256], no_eob[99] = 0, gl[256]
    bw = BitWriter()
    dynamic_block(bw, [97], no_eob, gd, eob=False)
    add("no_end_of_block_code", bw.bytes(), "invalid code -- missing end-of-block", 1)
    # four code-length codes (HCLEN field 0) name 16, 17, 18 and 0 only: every length is zero
    cl4 = [0] * 19
    cl4[0] = cl4[18] = 1
    bw = BitWriter()
    n_cl = dynamic_header(bw, [0] * 257, [0], cl_lens=cl4, n_cl=4, rl=[(18, 127), (18, 120 - 11)])
    bw.bits(0, 16)
    add("four_code_length_codes", bw.bytes(), "invalid code -- missing end-of-block", 1, n_cl=n_cl)
    # sizes: ISIZE, CRC-32
    tok = _literals(rng, 500)
    add("one_byte_more_than_isize", _fixed(tok), "more output than ISIZE", 499, crc=zlib.crc32(bytes(tok[:499])))
    add("one_byte_less_than_isize", _fixed(tok), "less output than ISIZE", 501, crc=zlib.crc32(bytes(tok)))
    tok2 = tok + [(258, 7)]
    add("match_crosses_isize_by_one", _fixed(tok2), "more output than ISIZE", 757, crc=zlib.crc32(expand(tok2)[:757]))
    add("crc_one_bit", _fixed(tok), "wrong CRC", 500, crc=zlib.crc32(bytes(tok)) ^ 0x00010000)
    return cases


def _truncated_cases():
    """A valid member of each block type cut after 1, 2, 3 and half of its bytes, ISIZE and CRC-32 kept: what the reader sees behind
    the cut may decode to anything, so only `refused` is expected."""
    rng = random.Random(1953)
    tok = _literals(rng, 600, 20) + [(100, 300), 3, (258, 1)]
    payload = expand(tok)
    streams = {"fixed": _fixed(tok)}
    bw = BitWriter()
    stored_block(bw, payload)
    streams["stored"] = bw.bytes()
    bw = BitWriter()
    huffman_block(bw, tok)
    streams["dynamic"] = bw.bytes()
    cases = []
    for kind, cdata in streams.items():
        for keep in (1, 2, 3, len(cdata) // 2):
            cases.append(Case("truncated", "%s_cut_at_%d" % (kind, keep), cdata[:keep], None, "stream incomplete", crc=zlib.crc32(payload), isize=len(payload),
                              verdict=ANY_BAD, whole=cdata))
    return cases


@functools.lru_cache(None)
def case_table():
    """Every crafted member: the valid groups, the refused rows and the truncated members."""
    return tuple(_valid_cases() + _other_encoder_cases() + _invalid_cases() + _truncated_cases())


def cases(group=None, valid=None):
    return [c for c in case_table() if (group is None or c.group == group) and (valid is None or c.valid == valid)]


# ---- random members (tools/fuzz_inflate.py) ---------------------------------------------------------------------------------------------
def random_member(rng, max_payload=60000):
    """(payload, cdata): a random token list -- literals over a random alphabet, matches at distances up to 32 768 -- in one to four
    blocks of random type; the dynamic ones under random complete sets of code lengths (a Huffman code of random weights)."""
    tokens, size, blocks = [], 0, []
    bw = BitWriter()
    n_blocks = rng.randrange(1, 5)
    target = rng.choice([0, 1, 50, 3000, 40000, max_payload])
    for b in range(n_blocks):
        tok, alphabet = [], rng.choice([1, 2, 4, 20, 256])
        goal = rng.randrange(0, target // n_blocks + 1) if target else 0
        made = 0
        while made < goal:
            if size + made == 0 or rng.random() < 0.5:
                n = min(goal - made, rng.randrange(1, 40))
                tok += [rng.randrange(alphabet) for _ in range(n)]
                made += n
            else:
                ln = min(rng.choice([3, 4, 10, 63, 64, 65, 257, 258]), max(3, goal - made))
                d = rng.choice([1, 2, 3, ln - 1, ln, ln + 1, 300, NEAR_MAX, NEAR_MAX + 1, RING, 20000, 32768, rng.randrange(1, 32769)])
                tok.append((ln, min(max(d, 1), size + made)))
                made += ln
        final = b == n_blocks - 1
        kind = rng.randrange(3)
        if kind == 0 and all(isinstance(t, int) for t in tok):
            stored_block(bw, bytes(tok), final=final)
        elif kind == 1:
            fixed_block(bw, tok, final=final, alt258=rng.random() < 0.3)
        else:
            lf, df = token_freqs(tok)
            if rng.random() < 0.5:                                              # codes for symbols that never come, too
                lf = [f + (rng.random() < 0.5) for f in lf]
                df = [f + (rng.random() < 0.5) for f in df]
            skew = rng.choice([0.0, 1.0, 4.0])                                  # random weights: flat ... a long tail of 15-bit codes
            lf = [f and 1 + int(f * 1000 * rng.random() ** skew) for f in lf]
            df = [f and 1 + int(f * 1000 * rng.random() ** skew) for f in df]
            huffman_block(bw, tok, final=final, freqs=(lf, df))
        tokens += tok
        size += made
    return expand(tokens), bw.bytes()
