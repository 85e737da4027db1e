"""The BAM index (.bai, SAM specification section 5.2) in plain Python: the binning scheme, the writer's rule, the parser and the query.

The library's index code (csrc/hgx_bai.cpp) is held to this file: hgx_bam_index_build must write exactly `build`'s bytes, and a region
read through an index must give what the full read gives.  test_bai_ref.py pins this file itself by brute force.

The writer's rule (one definite byte string per coordinate-sorted BAM):
  * a record's virtual offset is (file offset of the block << 16 | offset in the block's payload) for the FIRST block whose payload
    reaches beyond the record's first byte; the end of the stream is (file size << 16);
  * placed = refID >= 0 and pos >= 0; bin = reg2bin(pos, pos + max(reference span of the CIGAR, 1)), span 0 with the unmapped flag;
  * the chunks of a (reference, bin) are the maximal runs of consecutive records with that pair, each [first record's offset, offset
    of the record behind the run), bins ascending, no pseudo-bin;
  * ioffset[w] = the smallest offset of a record overlapping 16 kb window w; windows without one take the previous window's value
    (0 in front of the first); n_intv = last overlapped window + 1;
  * n_no_coor (the records that are not placed) at the end.
"""
import struct
import zlib

PSEUDO_BIN = 37450
MAX_POS = 1 << 29


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def blocks(data):
    """[(file offset, payload)] of a BGZF file's blocks."""
    out, off = [], 0
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04", off
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        p, bsize = off + 12, None
        while p + 4 <= off + 12 + xlen:
            slen = struct.unpack_from("<H", data, p + 2)[0]
            if data[p:p + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", data, p + 4)[0]
            p += 4 + slen
        cdata = data[off + 12 + xlen:off + bsize + 1 - 8]
        payload = zlib.decompress(cdata, -15) if cdata else b""
        assert len(payload) == struct.unpack_from("<I", data, off + bsize + 1 - 4)[0]
        out.append((off, payload))
        off += bsize + 1
    return out


def read(bam_path):
    """-> (refs [(name, length)], records, end): records = dicts with voff, ref, pos, end (exclusive), flag, rname, size (bytes with the
    length word) in file order; `end` = the virtual offset of the stream's end."""
    with open(bam_path, "rb") as f:
        data = f.read()
    blks = blocks(data)
    raw = b"".join(p for _, p in blks)
    starts, at = [], 0                       # (stream offset of the block's first byte, length, file offset) of non-empty blocks
    for off, p in blks:
        if p:
            starts.append((at, len(p), off))
        at += len(p)

    def voff(s, hint=[0]):
        k = hint[0]
        if k >= len(starts) or starts[k][0] > s:
            k = 0
        while k < len(starts) and starts[k][0] + starts[k][1] <= s:
            k += 1
        hint[0] = k
        return (len(data) << 16) if k == len(starts) else (starts[k][2] << 16) | (s - starts[k][0])

    assert raw[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        refs.append((raw[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
        p += 4 + l_name + 4
    recs = []
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        ref, pos, l_rn, _mq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", raw, p + 4)
        span = 0
        if not flag & 4:
            for k in range(n_cig):
                v = struct.unpack_from("<I", raw, p + 36 + l_rn + 4 * k)[0]
                if (v & 15) in (0, 2, 3, 7, 8):
                    span += v >> 4
        recs.append({"voff": voff(p), "ref": ref, "pos": pos, "end": pos + max(span, 1), "flag": flag, "rname": refs[ref][0] if ref >= 0 else "*",
                     "size": 4 + bs, "qname": raw[p + 36:p + 36 + l_rn - 1].decode()})
        p += 4 + bs
    assert p == len(raw)
    return refs, recs, len(data) << 16


def build(bam_path):
    """The index of a coordinate-sorted BAM by the rule in this module's docstring."""
    refs, recs, v_end = read(bam_path)
    per_ref = [{"bins": {}, "ioffset": {}} for _ in refs]
    n_no_coor, prev = 0, None
    for k, r in enumerate(recs):
        nxt = recs[k + 1]["voff"] if k + 1 < len(recs) else v_end
        if r["ref"] < 0 or r["pos"] < 0:
            n_no_coor += 1
            prev = None
            continue
        assert n_no_coor == 0 and r["end"] <= MAX_POS
        key = (r["ref"], reg2bin(r["pos"], r["end"]))
        R = per_ref[r["ref"]]
        if key == prev:
            R["bins"][key[1]][-1][1] = nxt
        else:
            R["bins"].setdefault(key[1], []).append([r["voff"], nxt])
        prev = key
        for w in range(r["pos"] >> 14, ((r["end"] - 1) >> 14) + 1):
            R["ioffset"].setdefault(w, r["voff"])
    out = bytearray(b"BAI\x01" + struct.pack("<i", len(refs)))
    for R in per_ref:
        out += struct.pack("<i", len(R["bins"]))
        for b in sorted(R["bins"]):
            out += struct.pack("<Ii", b, len(R["bins"][b]))
            for beg, end in R["bins"][b]:
                out += struct.pack("<QQ", beg, end)
        n_intv = max(R["ioffset"]) + 1 if R["ioffset"] else 0
        out += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = R["ioffset"].get(w, last)
            out += struct.pack("<Q", last)
    return bytes(out + struct.pack("<Q", n_no_coor))


def parse(data):
    """-> {'refs': [{'bins': {bin: [(beg, end)]}, 'ioffset': [...]}], 'n_no_coor': int or None}; ValueError for anything wrong."""
    def take(fmt, at):
        if at + struct.calcsize(fmt) > len(data):
            raise ValueError("truncated index")
        return struct.unpack_from(fmt, data, at), at + struct.calcsize(fmt)
    if data[:4] != b"BAI\x01":
        raise ValueError("not a BAM index")
    (n_ref,), at = take("<i", 4)
    if n_ref < 0:
        raise ValueError("negative count")
    refs = []
    for _ in range(n_ref):
        (n_bin,), at = take("<i", at)
        if n_bin < 0:
            raise ValueError("negative count")
        bins = {}
        for _ in range(n_bin):
            (b, n_chunk), at = take("<Ii", at)
            if n_chunk < 0:
                raise ValueError("negative count")
            chunks = []
            for _ in range(n_chunk):
                (beg, end), at = take("<QQ", at)
                if b != PSEUDO_BIN and beg > end:
                    raise ValueError("chunk ends before it begins")
                chunks.append((beg, end))
            bins.setdefault(b, []).extend(chunks)
        (n_intv,), at = take("<i", at)
        if n_intv < 0:
            raise ValueError("negative count")
        iv = []
        for _ in range(n_intv):
            (v,), at = take("<Q", at)
            iv.append(v)
        refs.append({"bins": bins, "ioffset": iv})
    n_no_coor = None
    if len(data) - at >= 8:
        (n_no_coor,), at = take("<Q", at)
    elif len(data) != at:
        raise ValueError("truncated index")
    return {"refs": refs, "n_no_coor": n_no_coor}


def query(index, ref, beg, end):
    """The chunks that may hold records of reference `ref` overlapping [beg, end), sorted."""
    if not 0 <= ref < len(index["refs"]) or end <= beg:
        return []
    R = index["refs"][ref]
    w = beg >> 14
    min_off = R["ioffset"][w] if w < len(R["ioffset"]) else 0
    out = []
    for b in reg2bins(beg, end):
        if b != PSEUDO_BIN:
            out.extend(c for c in R["bins"].get(b, []) if c[1] > min_off)
    return sorted(out)


def records_in(bam_path, chunks):
    """The records (as `read` gives them) whose first byte lies inside one of the chunks, each once, in file order."""
    _, recs, _ = read(bam_path)
    return [r for r in recs if any(beg <= r["voff"] < end for beg, end in chunks)]


def dump(index):
    """parse's structure back as bytes (bins ascending; n_no_coor None = left out)."""
    out = bytearray(b"BAI\x01" + struct.pack("<i", len(index["refs"])))
    for R in index["refs"]:
        out += struct.pack("<i", len(R["bins"]))
        for b in sorted(R["bins"]):
            out += struct.pack("<Ii", b, len(R["bins"][b]))
            for beg, end in R["bins"][b]:
                out += struct.pack("<QQ", beg, end)
        out += struct.pack("<i", len(R["ioffset"])) + b"".join(struct.pack("<Q", v) for v in R["ioffset"])
    if index["n_no_coor"] is not None:
        out += struct.pack("<Q", index["n_no_coor"])
    return bytes(out)


def with_pseudo_bin(data):
    """The same index with htslib's metadata bin 37450 in every reference that has bins (two "chunks": the reference's offset range,
    then the mapped / unmapped counts -- not offsets, and not in order)."""
    ix = parse(data)
    for R in ix["refs"]:
        if R["bins"]:
            lo = min(c[0] for cs in R["bins"].values() for c in cs)
            hi = max(c[1] for cs in R["bins"].values() for c in cs)
            R["bins"][PSEUDO_BIN] = [(lo, hi), ((1 << 40) + len(R["bins"]), 0)]
    return dump(ix)


def with_zero_linear(data):
    """The same index with every linear offset 0 (a lower bound that says nothing)."""
    ix = parse(data)
    for R in ix["refs"]:
        R["ioffset"] = [0] * len(R["ioffset"])
    return dump(ix)


def without_no_coor(data):
    ix = parse(data)
    ix["n_no_coor"] = None
    return dump(ix)
