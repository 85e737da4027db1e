"""Named inputs of the device read table (csrc/hgx_reads.hip), shared by tests/test_reads_table_ref.py (CPU: the
statement against the host loader) and tests/test_gpu_reads_table.py (the kernels against the statement).

cases() = {name: Case}: texts (one or two inflated FASTA / FASTQ texts), fastq (None / True / False as Reads.from_text takes it),
front (the test switch the GPU test sets: "device", "host", or None = no switch, the gate decides), takes (the decline code the
kernels must report, written down by hand per case: 0 = they make the table) and error (None, or the kind of the loader's message
where the statement raises).  T = align.READS_TILE.  The one code without a case is SIZE: 4 GB of text is no test input.
"""
import collections
import random

from hisatgenotype_amd import align
import reads_table_ref as ref

T = align.READS_TILE
Case = collections.namedtuple("Case", "texts fastq front takes error")


def _seq(rng, n):
    return "".join(rng.choice("ACGTN") for _ in range(n))


def _qual(rng, n):
    return "".join(chr(rng.randrange(35, 74)) for _ in range(n))       # '#' .. 'I' ('+' and '@' among them, anywhere in a line)


def _fastq(recs, eol="\n", name_eol=None, last_eol=True):
    name_eol = eol if name_eol is None else name_eol
    t = "".join("@%s%s%s%s+%s%s%s" % (n, name_eol, s, eol, eol, q, eol) for n, s, q in recs)
    return (t if last_eol else t[:len(t) - len(eol)]).encode()


def _fasta(recs, eol="\n"):
    return "".join(">%s%s%s%s" % (n, eol, s, eol) for n, s in recs).encode()


def _recs(seed, n, length=lambda k: 50, prefix="r"):
    rng = random.Random(seed)
    return [("%s%d" % (prefix, k), _seq(rng, length(k)), _qual(rng, length(k))) for k in range(n)]


def _fastq_of_size(seed, total):
    """A FASTQ text of exactly `total` bytes that ends with '\\n': 50-base records (name + 106 bytes each), the last one's name
    stretched to fit."""
    rng = random.Random(seed)
    out, size, k = [], 0, 0
    while total - size >= 240:
        out.append(("s%d" % k, _seq(rng, 50), _qual(rng, 50)))
        size += len(out[-1][0]) + 106
        k += 1
    out.append(("L" * (total - size - 106), _seq(rng, 50), _qual(rng, 50)))
    text = _fastq(out)
    assert len(text) == total and 1 <= len(out[-1][0]) <= 255
    return text


_CASES = {}


def cases():
    if _CASES:
        return _CASES
    c = _CASES

    def ok(name, texts, fastq=None):
        c[name] = Case(texts, fastq, "device", 0, None)

    def declines(name, texts, code, error=None, fastq=None, front="device"):
        c[name] = Case(texts, fastq, front, code, error)

    # record counts at the lane, wavefront and workgroup edges of the record pass (256 lanes per workgroup, one lane more than records)
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257):
        ok("count-%d" % n, [_fastq(_recs(100 + n, n))])
    # text sizes at the tile edge: one tile less a byte, one tile, one tile and a byte
    for d in (-1, 0, 1):
        ok("bytes-T%+d" % d, [_fastq_of_size(200 + d, T + d)])
    # a '\n' as the last byte of a tile (offset T - 1) and as the first byte of the next (offset T), records behind it
    more = _fastq(_recs(210, 40, prefix="m"))
    ok("newline-last-of-tile", [_fastq_of_size(211, T) + more])
    ok("newline-first-of-tile", [_fastq_of_size(212, T + 1) + more])
    assert c["newline-last-of-tile"].texts[0][T - 1:T] == b"\n" and c["newline-first-of-tile"].texts[0][T:T + 1] == b"\n"
    # one record whose four lines start in four different tiles: a long comment on the name line and on the '+' line
    rng = random.Random(220)
    s, q = _seq(rng, 1024), _qual(rng, 1024)
    span = ("@span " + "c" * 7494 + "\n" + s + "\n+" + "p" * 4000 + "\n" + q + "\n").encode()
    starts = [0, span.index(b"\n") + 1, span.index(b"\n+") + 1, span.rindex(b"\n", 0, len(span) - 1) + 1]
    assert [x // T for x in starts] == [0, 1, 2, 3]
    ok("four-tiles", [span + _fastq(_recs(221, 3))])
    # the longest read the aligner takes, and (T >= 1 024: no line is longer than a tile) three reads of 341 bases in a row
    ok("read-1024", [_fastq(_recs(230, 2) + [("long", _seq(rng, 1024), _qual(rng, 1024))] + _recs(231, 2, prefix="b"))])
    ok("reads-3x341", [_fastq(_recs(232, 3, lambda k: 341))])
    # read lengths 1 .. 130: sequence and quality offsets take every residue mod 16
    ok("lengths-1-130", [_fastq(_recs(240, 130, lambda k: k + 1))])
    ok("no-final-newline", [_fastq(_recs(250, 5), last_eol=False)])
    ok("crlf", [_fastq(_recs(251, 70), eol="\r\n")])
    ok("crlf-no-final-newline", [_fastq(_recs(252, 3), eol="\r\n", last_eol=False)])
    ok("crlf-on-names-only", [_fastq(_recs(253, 70), name_eol="\r\n")])
    r = _recs(260, 6)
    ok("names", [_fastq([("n0 a comment", r[0][1], r[0][2]), ("n1\ttab comment", r[1][1], r[1][2]), ("", r[2][1], r[2][2]),
                         ("N" * 255, r[3][1], r[3][2]), (" blank first", r[4][1], r[4][2]), ("n5|x/1", r[5][1], r[5][2])])])
    ok("quality-starts-with-at-and-plus", [_fastq([("qa", r[0][1], "@" + r[0][2][1:]), ("qp", r[1][1], "+" + r[1][2][1:]),
                                                    ("qb", r[2][1], r[2][2][:-1] + "@")])])
    ok("fasta", [_fasta([(n, s) for n, s, _ in _recs(270, 70)])])
    ok("fasta-crlf-no-final-newline", [_fasta([(n, s) for n, s, _ in _recs(271, 3)], eol="\r\n")[:-2]])
    ok("fasta-forced", [_fasta([(n, s) for n, s, _ in _recs(272, 3)])], fastq=False)
    ok("two-fastq", [_fastq(_recs(280, 70, lambda k: 40 + k % 7)), _fastq(_recs(281, 70, lambda k: 90 - k % 11, prefix="m"))])
    ok("two-fasta", [_fasta([(n, s) for n, s, _ in _recs(282, 5)]), _fasta([(n, s) for n, s, _ in _recs(283, 5)])])
    ok("two-empty", [b"", b""])
    ok("fastq-and-fasta", [_fastq(_recs(284, 4)), _fasta([(n, s) for n, s, _ in _recs(285, 4)])])      # (each input by its first byte)

    # ---- one input per decline code ------------------------------------------------------------------------------------
    small = _fastq(_recs(300, 10))
    declines("gate", [small], ref.GATE_CODE, front=None)
    declines("switch", [small], ref.SWITCH, front="host")
    r = _recs(301, 4)
    declines("empty-line-between-records", [_fastq(r[:2]) + b"\n" + _fastq(r[2:])], ref.EMPTY_LINE)
    declines("empty-line-trailing", [_fastq(r) + b"\n"], ref.EMPTY_LINE)
    declines("empty-line-leading", [b"\n" + _fastq(r)], ref.EMPTY_LINE, fastq=True)      # (told: the first byte is no '@')
    declines("empty-line-cr-only", [_fastq(r) + b"\r\n"], ref.EMPTY_LINE)
    declines("empty-read", [b"@e\n\n+\n\n" + _fastq(r)], ref.EMPTY_LINE)
    declines("marker", [_fastq(r[:2]) + b"x" + _fastq(r[2:])[1:]], ref.MARKER, "format")
    declines("marker-forced-fastq-on-fasta", [_fasta([(n, s) for n, s, _ in r])], ref.MARKER, "format", fastq=True)
    declines("marker-multi-line-fasta", [b"".join((">%s\n%s\n%s\n" % (n, s[:30], s[30:])).encode() for n, s, _ in r)], ref.MARKER)
    declines("marker-fasta-header-behind-header", [b">a\n>b\nACGT\n>c\nAC\n"], ref.MARKER)
    declines("truncated", [_fastq(r)[:-(len(r[3][2]) + 1)]], ref.TRUNCATED, "truncated")            # the last record lacks its fourth line
    declines("truncated-fasta", [_fasta([(n, s) for n, s, _ in r]) + b">z\n"], ref.TRUNCATED)
    declines("quality-length", [_fastq([r[0], (r[1][0], r[1][1], r[1][2][:-1]), r[2]])], ref.QUAL_LEN, "truncated")
    declines("lower", [_fastq([r[0], (r[1][0], r[1][1][:20] + "g" + r[1][1][21:], r[1][2]), r[2]])], ref.LOWER)
    declines("lower-z-and-a", [_fasta([("z", "ACGTz"), ("a", "aACGT")])], ref.LOWER)
    declines("lower-last-byte-of-the-text", [_fasta([("x", "ACGTACGTAC"), ("y", "ACGTACGTACGTt")])[:-1]], ref.LOWER)
    pre = b">b16 pad\n"                                                     # 9 bytes: base k of the read stands at offset 9 + k
    declines("lower-at-a-16-byte-boundary", [pre + b"ACGTACG" + b"c" + b"ACGTACGTACGTACGT\n"], ref.LOWER)
    assert c["lower-at-a-16-byte-boundary"].texts[0][16:17] == b"c"
    declines("lower-before-a-16-byte-boundary", [pre + b"ACGTAC" + b"t" + b"GACGTACGTACGTACGT\n"], ref.LOWER)
    declines("count", [_fastq(r), _fastq(r[:3])], ref.COUNT, "count")
    declines("read-length", [_fastq(r[:2] + [("big", _seq(rng, 1025), _qual(rng, 1025))])], ref.READ_LEN, "read_len")
    # several rules at once: the smallest code
    declines("empty-line-and-lower", [_fasta([("x", "ACgT")]) + b"\n"], ref.EMPTY_LINE)
    declines("not-in-a-z", [_fasta([("x", "AC`{T")])], 0)                    # ('`' and '{' stand beside a-z)
    return c
