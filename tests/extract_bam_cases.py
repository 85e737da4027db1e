"""Shared by tests/test_gpu_extract_bam.py and tests/test_extract_bam_host.py: BAM builders and the comparison of
Extractor.feed_bam with the yardstick -- the lines `samtools view` prints for the same records through Extractor.feed (the text
route) and through the spec (tests/extract_ref.py)."""
import os
import struct
import tempfile
import zlib

import extract_ref
from hisatgenotype_amd import bamio, capi, engine, extract

REFS = [(c, 100000000) for c in ["1", "2", "6", "7", "18", "22", "X"]]
# what a BAM cannot hold: a record with fewer than 11 columns, a tag value that is no integer (bamio refuses both)
NOT_IN_BAM = {"error_short_line", "error_tag_value"}
SEQ_CODES = "=ACMGRSVTWYHKDBN"
DECLINE = {"RECORD": 3, "VALUE": 4, "TYPE": 6, "NAMES": 9, "INFLATE": 11, "CHAIN": 12}


def fixture(name):
    """The fixture as a BAM can hold it, with its regions, families and expected {(family index, mate): text}."""
    fx = extract_ref.load(name)
    if name == "reverse_with_n":
        # BAM's 4-bit codes have no lower case: acgt are stored as N, so the expectation is the spec's on that text
        fx = dict(fx, sam=fx["sam"].replace("acgt", "NNNN"))
    dbl = list(fx["args"]["database_list"])
    regions = extract_ref.region_table(fx["locus"], dbl)
    a = fx["args"]
    texts, exc = extract_ref.extract(fx["sam"], regions, dbl, a["aligner"], a["paired"], a["simulation"], a["fastq"])
    expect = {(dbl.index(f), m): t for (f, m), t in texts.items()}
    assert (exc.__name__ if exc else None) == fx["exception"]
    return fx, regions, dbl, expect


def bam_names():
    return [n for n in extract_ref.fixture_names() if n not in NOT_IN_BAM and not extract_ref.load(n)["pre_existing"]]


def inflate_all(bgzf):
    return b"".join(bamio._bgzf_blocks(bgzf))


def bgzf(raw, block_size=0xff00, cuts=()):
    """`raw` as BGZF blocks of block_size bytes, with a block boundary at every offset in `cuts` as well.  -> (bytes, the file
    offsets at which the blocks end)."""
    edges = sorted(set(list(range(0, len(raw), block_size)) + [c for c in cuts if 0 < c < len(raw)] + [len(raw)]))
    out, ends = bytearray(), {}
    for b, e in zip(edges[:-1], edges[1:]):
        for p in range(b, e, 0xff00):
            piece = raw[p:min(p + 0xff00, e)]
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            cdata = comp.compress(piece) + comp.flush()
            out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata +
                    struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece)))
        ends[e] = len(out)
    out += bamio._BGZF_EOF
    return bytes(out), ends


def sam_to_bam(sam, block_size=0xff00, refs=REFS):
    """bamio.write_bam's file for SAM text.  -> bytes"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.bam")
        bamio.write_bam(path, sam, refs, block_size=block_size)
        with open(path, "rb") as f:
            return f.read()


def bam_lines(data):
    """The lines `samtools view` prints for a BAM's bytes (bamio.read_bam), newline-joined."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.bam")
        with open(path, "wb") as f:
            f.write(data)
        lines = bamio.read_bam(path)
    return "".join(l + "\n" for l in lines)


def header(refs=REFS):
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs).encode()
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def record(qname, flag, rid, pos0, seq="ACGT", qual=None, aux=b"", codes=None):
    """One BAM record with its block_size word (no CIGAR, no mate fields).  qname: bytes; seq "*": l_seq 0; qual None: 'I's,
    "*": 0xff-filled; codes: the 4-bit base codes instead of seq."""
    if codes is None:
        codes = [] if seq == "*" else [SEQ_CODES.index(c) for c in seq]
    n = len(codes)
    padded = list(codes) + [0]
    packed = bytes((padded[i] << 4) | padded[i + 1] for i in range(0, n, 2))
    q = bytes([0xff] * n) if qual == "*" else bytes([40] * n) if qual is None else bytes(ord(c) - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", rid, pos0, len(qname) + 1, 0, 4680, 0, flag, n, -1, -1, 0) + qname + b"\0" + packed + q + aux
    return struct.pack("<i", len(body)) + body


def line(qname, flag, rid, pos0, seq="ACGT", qual=None, tags=(), codes=None, refs=REFS):
    """The line `samtools view` prints for record(...) with the same arguments (tags: the printed fields).  -> bytes"""
    if codes is not None:
        seq = "".join(SEQ_CODES[c] for c in codes) or "*"
    n = 0 if seq == "*" else len(seq)
    q = "*" if (qual == "*" or n == 0) else "I" * n if qual is None else qual
    cols = [qname, b"%d" % flag, refs[rid][0].encode() if 0 <= rid < len(refs) else b"*", b"%d" % (pos0 + 1), b"0", b"*", b"*", b"0", b"0",
            seq.encode(), q.encode()] + [t if isinstance(t, bytes) else t.encode() for t in tags]
    return b"\t".join(cols) + b"\n"


def aux_int(tag, t, v):
    return tag.encode() + t.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[t], v)


def run(feed_name, regions, families, a, data, sizes, front=None):
    """Feed `data` through Extractor.<feed_name> in blocks of the given sizes (cycled), taking after every block.
    -> ({(family, mate): bytes}, stats, exception or None, the library's message)."""
    with engine.test_switches(**({"front": front} if front else {})):
        ex = extract.Extractor(regions, families, a["aligner"], a["paired"], a["simulation"], a["fastq"])
        out = {(f, m): [] for f in range(len(families)) for m in range(2 if a["paired"] else 1)}
        exc, msg = None, ""
        p, k = 0, 0
        try:
            try:
                while True:
                    n = sizes[k % len(sizes)]
                    getattr(ex, feed_name)(data[p:p + n], last=p + n >= len(data))
                    p += n
                    k += 1
                    for key in out:
                        out[key].append(ex.take(*key))
                    if p >= len(data):
                        break
            except (ValueError, AssertionError, SystemExit, IndexError, TypeError, capi.HgxError) as e:
                exc = e
                msg = capi.lib().hgx_last_error().decode(errors="replace")
                for key in out:
                    out[key].append(ex.take(*key))
            return {key: b"".join(v) for key, v in out.items()}, ex.stats(), exc, msg
        finally:
            ex.close()


def kind(exc):
    return type(exc).__name__ if exc is not None else None


def spec(text, regions, families, a):
    texts, exc = extract_ref.extract(text, regions, families, a["aligner"], a["paired"], a["simulation"], a["fastq"])
    return {(families.index(f), m): t.encode() for (f, m), t in texts.items()}, (exc.__name__ if exc else None)


# ---- records assembled here: aux encodings, reference ids, base codes and damage that bamio.write_bam cannot produce -------------
CASE_REGIONS = [("fa", "6", 1000, 2000), ("fb", "6", 1500, 3000), ("fb", "7", 100, 200), ("fa", "7", 150, 400), ("fb", "7", 10000, 20000)]
CASE_FAMILIES = ["fa", "fb"]
ARGS = {"aligner": "hisat2", "paired": True, "simulation": False, "fastq": True}
NH1 = (aux_int("NH", "C", 1), ("NH:i:1",))


def pair(qname, rid, pos0, aux=NH1[0], tags=NH1[1], flag1=0x43, flag2=0x83, **kw):
    """Both mates of a read with the same aux data.  -> [(record, line)] * 2"""
    return [(record(qname, f, rid, pos0, aux=aux, **kw), line(qname, f, rid, pos0, tags=tags, **kw)) for f in (flag1, flag2)]


def single(qname, flag, rid, pos0, aux=NH1[0], tags=NH1[1], **kw):
    return [(record(qname, flag, rid, pos0, aux=aux, **kw), line(qname, flag, rid, pos0, tags=tags, **kw))]


def _aux_cases():
    ok = []
    for k, t in enumerate("cCsSiI"):                                     # NH of every integer type; behind Z, H and B tags
        ok += pair(b"nh_%s" % t.encode(), 2, 1100 + k, aux_int("NH", t, 1), ("NH:i:1",))
        ok += pair(b"nh2_%s" % t.encode(), 2, 1100 + k, aux_int("NH", t, 2), ("NH:i:2",))
    ok += pair(b"neg", 2, 1100, aux_int("NH", "c", -1) + aux_int("AS", "s", -300), ("NH:i:-1", "AS:i:-300"))
    ok += pair(b"behind_z", 2, 1600, b"YTZCP\0" + aux_int("NH", "C", 1), ("YT:Z:CP", "NH:i:1"))
    ok += pair(b"behind_h", 2, 1600, b"XHH1AE3\0" + aux_int("NH", "C", 1), ("XH:H:1AE3", "NH:i:1"))
    for st, fmt, vals in (("c", "<3b", (-1, 2, 3)), ("C", "<3B", (1, 2, 255)), ("s", "<3h", (-300, 2, 3)), ("S", "<3H", (1, 2, 65535)),
                          ("i", "<3i", (-70000, 2, 3)), ("I", "<3I", (1, 2, 4000000000)), ("f", "<3f", (1.5, 2.0, -0.25))):
        arr = b"ZBB" + st.encode() + struct.pack("<I", 3) + struct.pack(fmt, *vals)
        txt = "ZB:B:%s,%s" % (st, ",".join(("%g" % v) if st == "f" else str(v) for v in vals))
        ok += pair(b"behind_b" + st.encode(), 3, 160, arr + aux_int("NH", "C", 1), (txt, "NH:i:1"))
    ok += pair(b"dup_last_1", 2, 1100, aux_int("NH", "C", 2) + aux_int("NH", "C", 1), ("NH:i:2", "NH:i:1"))
    ok += pair(b"dup_last_2", 2, 1100, aux_int("NH", "C", 1) + aux_int("NH", "C", 2), ("NH:i:1", "NH:i:2"))
    bt = []
    for k, t in enumerate("cCsSiI"):                                     # bowtie2: AS > XS on the first left record
        bt += pair(b"as_%s" % t.encode(), 2, 1100, aux_int("AS", t, 5) + aux_int("XS", t, 3), ("AS:i:5", "XS:i:3"))
        bt += pair(b"xs_%s" % t.encode(), 2, 1100, aux_int("AS", t, 3) + aux_int("XS", t, 5), ("AS:i:3", "XS:i:5"))
    pad = pair(b"before", 2, 1100) + pair(b"before2", 3, 160)
    return [
        dict(name="aux_types", recs=ok),
        dict(name="aux_bowtie2", recs=bt, args=dict(ARGS, aligner="bowtie2")),
        dict(name="bowtie2_as_only", recs=pad + pair(b"r", 2, 1100, aux_int("AS", "c", 5), ("AS:i:5",)), args=dict(ARGS, aligner="bowtie2"),
             decline="TYPE", exc="TypeError"),
        dict(name="as_float", recs=pad + pair(b"r", 2, 1100, b"ASf" + struct.pack("<f", 1.5), ("AS:f:1.5",)), decline="VALUE", exc="ValueError"),
        # (int("1") is fine: the device leaves a Z-typed NH to the host route, which reads what the text holds, as the reference does)
        dict(name="nh_z_digit", recs=pad + pair(b"r", 2, 1100, b"NHZ1\0", ("NH:Z:1",)), decline="VALUE"),
        dict(name="nh_z_word", recs=pad + pair(b"r", 2, 1100, b"NHZone\0", ("NH:Z:one",)), decline="VALUE", exc="ValueError"),
        dict(name="nh_too_wide", recs=pad + pair(b"r", 2, 1100, aux_int("NH", "I", 4000000000), ("NH:i:4000000000",)) + pair(b"after", 2, 1100),
             decline="VALUE"),
        dict(name="z_blank", recs=pad + pair(b"r", 2, 1100, b"XXZa b\0" + NH1[0], ("XX:Z:a b", "NH:i:1")) + pair(b"after", 2, 1100), decline="RECORD"),
        dict(name="qname_high_byte", recs=pad + pair(b"r\x80x", 2, 1100) + pair(b"after", 2, 1100), decline="RECORD", ascii=False),
        dict(name="tag_past_record", recs=pad + pair(b"r", 2, 1100, b"NHi\x01\x00", ()), decline="RECORD", error="malformed BAM record"),
        dict(name="unknown_aux_type", recs=pad + pair(b"r", 2, 1100, b"NHq\x01", ()), decline="RECORD", error="malformed BAM record"),
    ]


def _ref_cases():
    recs = []
    recs += pair(b"unmapped", -1, -1, flag1=0x4d, flag2=0x8d)
    recs += pair(b"no_ref_mapped", -1, 1100)                                                # refID -1 without flag 4: '*' names no chromosome
    recs += pair(b"absent_chrom", 6, 1100)                                                  # X: not in the region table
    recs += pair(b"first_region_wins", 2, 1600)                                             # 6:1600 lies in fa's and in fb's region
    recs += pair(b"second_only", 2, 2500) + pair(b"chr7_fb", 3, 120) + pair(b"chr7_both", 3, 160) + pair(b"chr7_far", 3, 15000)
    recs += pair(b"edge_left", 2, 1000) + pair(b"edge_right", 2, 2000 + 999) + pair(b"edge_out", 2, 3000)
    return [
        dict(name="references", recs=recs),
        dict(name="ref_id_beyond_table", recs=recs + pair(b"bad", len(REFS), 1100) + pair(b"after", 2, 1100), decline="RECORD"),
    ]


def _base_cases():
    import random
    rnd = random.Random(5)
    recs = []
    # 150, 250: the workload's read lengths; 1023 .. 1025: k_ext_emit stages 1024 bytes a round and writes 256 bytes a round
    for n in (0, 1, 2, 63, 64, 65, 150, 250, 1023, 1024, 1025, 4097, 5000):
        seq = "".join(rnd.choice("ACGTN") for _ in range(n)) or "*"
        qual = None if n == 0 else "".join(chr(33 + rnd.randrange(0, 60)) for _ in range(n))
        for k, (f1, f2) in enumerate(((0x43, 0x83), (0x53, 0x93), (0x43, 0x93))):
            recs += pair(b"len%d_%d" % (n, k), 2, 1100, flag1=f1, flag2=f2, seq=seq, qual=qual)
    # Either side of the first length L at which k_ext_emit stops staging a read in LDS (csrc/hgx_extract.hip: staged = span <=
    # EXT_SRC_MAX = 4096 and pad + total <= EXT_IMG_MAX = 4608), for a name of 8 bytes and l bases.  a = the source's offset in
    # its 16-byte granule (0 .. 15) and pad = the destination's in its dword (0 .. 3) depend on where a piece pattern puts the
    # record, so every length from the least L - 1 to the greatest L is here: L - 1 and L are among them whatever a and pad are.
    #   BAM, FASTQ:  total = 2 l + 14, span = a + ceil(l / 2) + l < 4096 there; pad + 2 l + 14 > 4608  <=>  L = 2298 - ceil(pad / 2)
    #                (pad 0: 2298, pad 1 and 2: 2297, pad 3: 2296): 2295 .. 2298
    #   BAM, FASTA:  total = l + 11, span = a + ceil(l / 2) < 4096 there; pad + l + 11 > 4608  <=>  L = 4598 - pad: 4594 .. 4598
    #   SAM text, FASTQ (SEQ, a tab, QUAL): span = a + 2 l + 1 > 4096  <=>  L = 2048 - floor(a / 2), a = 0 .. 15: 2040 .. 2048
    #                (total = 2 l + 14 <= 4110 there)
    for n in list(range(2040, 2049)) + list(range(2295, 2299)) + list(range(4594, 4599)):
        seq = "".join(rnd.choice("ACGTN") for _ in range(n))
        qual = "".join(chr(33 + rnd.randrange(0, 60)) for _ in range(n))
        recs += pair(b"edge%04d" % n, 2, 1100, flag1=0x43, flag2=0x93, seq=seq, qual=qual)
    recs += pair(b"codes", 2, 1100, flag1=0x53, flag2=0x83, codes=list(range(16)))
    recs += pair(b"codes_odd", 2, 1100, flag1=0x53, flag2=0x93, codes=list(range(16)) + [3])
    for n in (1, 7, 100):
        recs += pair(b"noqual%d" % n, 2, 1100, flag1=0x53, flag2=0x83, seq="ACGTTGCAAC" * 10 if n == 100 else "ACGTTGC"[:n], qual="*")
    for name in (b"a", b"ab", b"abc", b"abcd", b"x", b"xy", b"xyz"):                        # destinations at every dword offset
        recs += pair(name, 2, 1100, seq="ACGTA"[:1 + len(name)])
    un_recs = []
    for n in (0, 1, 64, 65):
        seq = "".join(rnd.choice("ACGT") for _ in range(n)) or "*"
        un_recs += single(b"u%d" % n, 0x10 if n & 1 else 0, 2, 1100, seq=seq) + single(b"u%d_b" % n, 0, 3, 160, seq=seq)
    return [
        dict(name="bases_fastq", recs=recs),
        dict(name="bases_fasta", recs=recs, args=dict(ARGS, fastq=False)),
        dict(name="bases_unpaired", recs=un_recs, args=dict(ARGS, paired=False)),
        dict(name="names_simulation", recs=pair(b"r1|a", 2, 1100) + pair(b"r1|b", 3, 160) + pair(b"r2|a", 2, 1100),
             args=dict(ARGS, simulation=True)),
    ]


def _damage_cases():
    recs = []
    for k in range(60):
        recs += pair(b"read%03d" % k, 2, 1100 + k)
    raw = header() + b"".join(r for r, _ in recs)
    good, _ = bgzf(raw, 1500)
    # a flipped byte inside the deflate data of the third block
    ends = []
    off = 0
    while off < len(good):
        ends.append(off)
        off += struct.unpack_from("<H", good, off + 16)[0] + 1
    flipped = bytearray(good)
    flipped[ends[2] + 18 + 40] ^= 0x55
    cut_at = len(raw) - len(recs[-1][0]) // 2                            # inside the last record
    complete = len(raw) - len(recs[-1][0])
    return [
        dict(name="flipped_deflate_byte", data=bytes(flipped), recs=recs, decline="INFLATE", error=r"corrupt BGZF block \(inflate / CRC32 / ISIZE mismatch\)"),
        dict(name="truncated_mid_record", data=bgzf(raw[:cut_at], 1500)[0], recs=recs, error="truncated BAM record at offset %d$" % complete),
    ]


CASES = _aux_cases() + _ref_cases() + _base_cases() + _damage_cases()


def check_case(case, front, piece_lists):
    """feed_bam on the case's BAM in every piece pattern == the case's lines through the text route (same front) == the spec."""
    a = case.get("args", ARGS)
    text = b"".join(l for _, l in case["recs"])
    data = case.get("data") or bgzf(header() + b"".join(r for r, _ in case["recs"]), case.get("block_size", 700))[0]
    want, _, want_exc, _ = run("feed", CASE_REGIONS, CASE_FAMILIES, a, text, [len(text)], front=front)
    if case.get("error") is None:
        assert kind(want_exc) == case.get("exc"), case["name"]
        if case.get("ascii", True):
            s_out, s_exc = spec(text.decode(), CASE_REGIONS, CASE_FAMILIES, a)
            assert s_exc == case.get("exc") and s_out == want, case["name"]
    for sizes in piece_lists:
        got, st, exc, msg = run("feed_bam", CASE_REGIONS, CASE_FAMILIES, a, data, sizes, front=front)
        where = (case["name"], sizes, st, msg)
        if case.get("error") is not None:
            import re
            assert isinstance(exc, capi.HgxError) and re.search(case["error"], msg), where
            assert all(want[k].startswith(got[k]) for k in got), where         # what was written before the error is the text route's
        else:
            assert kind(exc) == kind(want_exc), where
            assert got == want, where
        if front == "device":
            if case.get("decline"):
                assert st["chunks_host"] >= 1 and st["decline"] == DECLINE[case["decline"]], where
            elif case.get("error") is None:
                assert st["route"] == 2 and st["chunks_host"] == 0, where
        else:
            assert st["route"] == 0 and st["chunks_device"] == 0, where
        if case.get("error") is None and exc is None:
            assert st["records"] == len(case["recs"]), where


# ---- hgx_extract_file (Extractor.feed_file) on a BAM file -------------------------------------------------------------------------
def run_file(regions, families, a, data, front, piece=None, tmp=None):
    """Extractor.feed_file on a file holding `data`.  -> ({(family, mate): bytes}, stats, exception or None, the library's message)"""
    sw = {"front": front}
    if piece is not None:
        sw["extract_bam_piece"] = str(piece)
    with tempfile.TemporaryDirectory() as d, engine.test_switches(**sw):
        path = os.path.join(d, "records.bam")
        with open(path, "wb") as f:
            f.write(data)
        ex = extract.Extractor(regions, families, a["aligner"], a["paired"], a["simulation"], a["fastq"])
        exc, msg = None, ""
        try:
            try:
                ex.feed_file(path)
            except (ValueError, AssertionError, SystemExit, IndexError, TypeError, capi.HgxError) as e:
                exc = e
                msg = capi.lib().hgx_last_error().decode(errors="replace")
            out = {(f, m): ex.take(f, m) for f in range(len(families)) for m in range(2 if a["paired"] else 1)}
            return out, ex.stats(), exc, msg
        finally:
            ex.close()


def check_file_entry(front):
    """hgx_extract_file reads a BAM in blocks of extract_bam_piece through hgx_extract_feed_bam: fixtures with and without the
    switch, a file whose size is a multiple of the piece, a bgzipped SAM text (the one-piece text path), damaged files."""
    import re
    for name in bam_names():
        fx, regions, fams, expect = fixture(name)
        a = fx["args"]
        data = sam_to_bam(fx["sam"], 1000)
        n_rec = sum(1 for l in fx["sam"].splitlines() if l and not l.startswith("@"))
        pieces = [None, max(len(data) // 5, 1), len(data)] + [len(data) // d for d in range(2, 40) if len(data) % d == 0][:1]
        for piece in pieces:
            got, st, exc, msg = run_file(regions, fams, a, data, front, piece)
            where = (name, piece, st, msg)
            assert kind(exc) == fx["exception"], where
            assert {k: v.decode() for k, v in got.items()} == expect, where
            if exc is None:
                assert st["records"] == n_rec, where
                if front == "device":
                    assert st["route"] == 2 and st["chunks_host"] == 0, where
                    if piece == len(data) // 5 and n_rec > 100:
                        assert st["chunks_device"] > 1, where
                else:
                    assert st["route"] == 0 and st["chunks_device"] == 0, where
    # a bgzipped SAM text is no BAM: the reader inflates it in one piece and its lines are the stream
    fx, regions, fams, expect = fixture("big_random")
    got, st, exc, msg = run_file(regions, fams, fx["args"], bgzf(fx["sam"].encode(), 0xff00)[0], front, 1000)
    assert exc is None and {k: v.decode() for k, v in got.items()} == expect, (st, msg)
    assert st["route"] == (2 if front == "device" else 0)
    for case in CASES:
        if case.get("data") is None:
            continue
        for piece in (None, 700):
            got, st, exc, msg = run_file(CASE_REGIONS, CASE_FAMILIES, ARGS, case["data"], front, piece)
            assert isinstance(exc, capi.HgxError) and exc.code == -6 and re.search(case["error"], msg), (case["name"], piece, msg)
