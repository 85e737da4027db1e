"""The read table of the "hgx" aligner in plain Python: what parse_reads / load_reads of
csrc/hgx_align_host.cpp make of one or two inflated FASTA / FASTQ texts, and which of those inputs the kernels of
csrc/hgx_reads.hip take.  Nothing here is shared with either implementation.

records(texts, fastq)       [(name, seq, qual | None)] in the aligner's order (read 2k + i = record k of input i), or ReadsError
                            with the kind of the loader's message
device_takes(texts, fastq)  the decline code the kernels must report, 0 = they make the table
"""
MAX_READ = 1024
TILE = 4096
GATE = 512 << 10
MAX_BYTES = (1 << 32) - 64
(GATE_CODE, SWITCH, EMPTY_LINE, MARKER, TRUNCATED, QUAL_LEN, LOWER, COUNT, READ_LEN, SIZE) = range(1, 11)

# kind -> words of the loader's message (hgx_last_error)
MESSAGES = {"format": "neither FASTA nor FASTQ", "truncated": "truncated FASTQ record", "count": "reads in the first file",
            "read_len": "the aligner takes up to"}


class ReadsError(ValueError):
    def __init__(self, kind):
        super().__init__(MESSAGES[kind])
        self.kind = kind


def _parse(t, fastq):
    """The records of one text, by the loader's line walk: a line ends at '\\n' (or the text's end) and loses one trailing '\\r';
    empty lines BETWEEN records are skipped; a FASTQ record is the next four lines whatever they hold; a FASTA record's bases
    are the lines up to the next non-empty line that starts with '>', joined."""
    n, k = len(t), 0

    def line():
        nonlocal k
        if k >= n:
            return None
        b = k
        e = t.find(b"\n", k)
        if e < 0:
            e = n
        k = e + 1
        if e > b and t[e - 1:e] == b"\r":
            e -= 1
        return b, e

    if fastq is None:
        fastq = t[:1] == b"@"
    recs = []
    cur = line()
    while cur is not None:
        b, e = cur
        if e == b:
            cur = line()
            continue
        if t[b:b + 1] != (b"@" if fastq else b">"):
            raise ReadsError("format")
        q = b + 1
        while q < e and t[q] not in (0x20, 0x09):
            q += 1
        name = t[b + 1:q]
        if fastq:
            s, p, ql = line(), line(), line()
            if s is None or p is None or ql is None or ql[1] - ql[0] != s[1] - s[0]:
                raise ReadsError("truncated")
            recs.append((name, t[s[0]:s[1]].upper(), t[ql[0]:ql[1]]))
            cur = line()
        else:
            parts = []
            while True:
                cur = line()
                if cur is None or (cur[1] > cur[0] and t[cur[0]:cur[0] + 1] == b">"):
                    break
                parts.append(t[cur[0]:cur[1]])
            recs.append((name, b"".join(parts).upper(), None))
    return recs


def records(texts, fastq=None):
    per = [_parse(bytes(t), fastq) for t in texts]
    if len(per) == 2 and len(per[0]) != len(per[1]):
        raise ReadsError("count")
    out = []
    for k in range(len(per[0])):
        for recs in per:
            if len(recs[k][1]) > MAX_READ:
                raise ReadsError("read_len")
            out.append(recs[k])
    return out


def device_takes(texts, fastq=None, front="device", max_bytes=MAX_BYTES):
    """The kernels see the text by POSITION: line l of a FASTQ text belongs to record l // 4 (FASTA: l // 2), the way the loader
    sees it when no line is empty and no FASTA record spans lines.  Every rule that the positional view breaks, or that would need
    the bases re-packed, is a decline; where several apply, the smallest code.  front: "device", "host", or None = the gate."""
    if front == "host":
        return SWITCH
    total = sum(len(t) for t in texts)
    if total + 64 >= max_bytes:              # (input 2 is padded to a multiple of 64: the rule counts the most it can be)
        return SIZE
    if front is None and total < GATE:
        return GATE_CODE
    codes, n_rec, longest = [], [], 0
    for t in texts:
        t = bytes(t)
        fq = (t[:1] == b"@") if fastq is None else bool(fastq)
        lines = t.split(b"\n")
        if lines[-1] == b"":                     # (behind the last '\n' there is no line; a last line without one is a line)
            lines.pop()
        lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
        if any(len(l) == 0 for l in lines):
            codes.append(EMPTY_LINE)
        per = 4 if fq else 2
        if len(lines) % per:
            codes.append(TRUNCATED)
        n_rec.append(len(lines) // per)
        for r in range(n_rec[-1]):
            head, seq = lines[per * r], lines[per * r + 1]
            if head and head[:1] != (b"@" if fq else b">"):
                codes.append(MARKER)
            if fq and len(lines[per * r + 3]) != len(seq):
                codes.append(QUAL_LEN)
            if not fq and seq[:1] == b">":
                codes.append(MARKER)
            if any(0x61 <= c <= 0x7a for c in seq):
                codes.append(LOWER)
            longest = max(longest, len(seq))
    if len(texts) == 2 and n_rec[0] != n_rec[1]:
        codes.append(COUNT)
    if longest > MAX_READ:
        codes.append(READ_LEN)
    return min(codes) if codes else 0
