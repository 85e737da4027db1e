"""Shared by tests/test_gpu_linear_edges.py and tests/test_linear_cases_host.py: builders of SAM lines and BAM records in the
shapes real aligners write, the case table of the linear route's edges, and the comparison of a case with the plain statement
(tests/linear_ref.py).  The expectation of a SAM case is the statement on its text, of a BAM case the statement on the lines
`samtools view` prints for its records."""
import functools
import os
import random
import re
import struct

import extract_bam_cases as X
import linear_ref
from hisatgenotype_amd import synth

DECLINE = {"UNKNOWN_NAME": 3, "AS": 4, "RECORD": 5}         # HGX_LIN_DECLINE_* (csrc/hgx_linear.hpp)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8191, 8193)      # around the scan's tile (SCAN_TILE = 4096) and its 4-entry loads
SHAPES = ("lines", "kept", "groups", "classes")


# ---- loci ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def locus(kind):
    """"str": the small locus every case uses unless it needs more; "hla": 300 alleles; "th01": names of six and seven bytes."""
    if kind == "hla":
        return synth.make_hla_like_locus(n_alleles=300, n_vars=200, seed=21)
    return synth.make_str_like_locus(seed=3) if kind == "str" else synth.make_str_like_locus(gene="TH01", seed=3)


@functools.lru_cache(None)
def alleles(kind):
    """The names a record can be kept on, in the locus' order."""
    return tuple(a for a in locus(kind).allele_names if "BACKBONE" not in a)


@functools.lru_cache(None)
def strange_names(kind):
    """RNAMEs beside the locus' own: another gene, names the gene filter or the BACKBONE scan skip, unknown in-gene names."""
    g, a = locus(kind).gene, alleles(kind)[0]
    return dict(other="ZZ9*1", short=g[:-1] or "*", tiny=g[:3] or "*", gene=g, bb_start=g + "BACKBONE", bb_mid=g + "*xBACKBONEy",
                bb_end=g + "*endBACKBONE", bb_alone="BACKBONE*1", last_byte=a[:-1] + ("a" if a[-1] != "a" else "b"), prefix=a[:-1],
                longer=a + "0")


@functools.lru_cache(None)
def refs(kind):
    """The reference table of a case's BAM: the locus' names, then strange_names."""
    names = list(locus(kind).allele_names)
    names += [n for n in dict.fromkeys(strange_names(kind).values()) if n not in names and n != "*"]
    return tuple((n, 100000) for n in names)


# ---- tags: (name, type, value) -> the printed column and the aux bytes ---------------------------------------------------------------
INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
INT_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (I32_MIN, I32_MAX), "I": (0, 2 ** 32 - 1)}


def int_type(v):
    """The type samtools picks for an integer: the smallest that holds it."""
    return next((t for t in ("C", "c", "S", "s", "I", "i") if INT_RANGE[t][0] <= v <= INT_RANGE[t][1]), "i")     # (none: text only)


def T(name, t, v=None):
    """A tag.  T("AS", 5): an integer of the smallest type.  T("AS", "s", 5): of that type.  Z / H / A: v is the text; f: a float;
    B: v = (subtype, values)."""
    if v is None:
        t, v = int_type(t), t
    return (name, t, v)


def tag_text(tag):
    name, t, v = tag
    if t in "cCsSiI":
        return "%s:i:%d" % (name, v)
    if t == "f":
        return "%s:f:%g" % (name, v)
    if t == "B":
        sub, vals = v
        return "%s:B:%s" % (name, ",".join([sub] + [("%g" % x) if sub == "f" else str(x) for x in vals]))
    return "%s:%s:%s" % (name, t, v)


def tag_aux(tag):
    name, t, v = tag
    head = name.encode() + t.encode()
    if t in INT_FMT:
        return head + struct.pack(INT_FMT[t], v)
    if t == "A":
        return head + v.encode()
    if t == "B":
        sub, vals = v
        return head + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(INT_FMT[sub], x) for x in vals)
    return head + v.encode() + b"\0"


def bowtie2_tags(v):
    return [T("AS", v), T("XS", v - 5), T("XN", 0), T("XM", 1), T("XO", 0), T("XG", 0), T("NM", 1), T("MD", "Z", "10A9"), T("YS", -3),
            T("YT", "Z", "CP")]


def hisat2_tags(v):
    return [T("NM", 1), T("MD", "Z", "10A9"), T("YS", -3), T("YT", "Z", "CP"), T("XS", "A", "+"), T("NH", 3), T("AS", v), T("ZS", v - 2)]


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def sam_line(qname, flag, rname, tags=(), sep="\t", seq="ACGTACGTACGTACGTACGT"):
    """One SAM line (no line end).  flag: anything str() prints; tags: printed columns or T() tuples; seq "*": an empty SEQ."""
    n = 0 if seq == "*" else len(seq)
    cols = [qname, str(flag), rname, "1", "60", "%dM" % n if n else "*", "*", "0", "0", seq, "I" * n if n else "*"]
    return sep.join(cols + [t if isinstance(t, str) else tag_text(t) for t in tags])


CIGARS = {0: [], 1: [(20, "M")], 3: [(2, "S"), (16, "M"), (2, "S")]}


def bam_record(kind, qname, flag, rname, tags=(), aux=None, printed=None, n_cigar=1, l_seq=20):
    """One BAM record of the locus' BAM and the line `samtools view` prints for it.  -> (record, line)
    extract_bam_cases.record writes the fixed fields, the name, the bases and the aux data; the CIGAR of n_cigar operations is
    spliced in behind the name here.  rname None: refID -1.  aux / printed: the aux bytes and the printed columns where tags
    (T() tuples) cannot say them (damaged records)."""
    q = qname if isinstance(qname, bytes) else qname.encode()
    table = refs(kind)
    rid = -1 if rname is None else [n for n, _ in table].index(rname)
    seq = ("ACGTN" * 4)[:l_seq] or "*"
    aux = b"".join(tag_aux(t) for t in tags) if aux is None else aux
    printed = [tag_text(t) for t in tags] if printed is None else printed
    body = bytearray(X.record(q, flag, rid, 0, seq=seq, aux=aux)[4:])
    ops = CIGARS[n_cigar]
    at = 32 + len(q) + 1
    body[at:at] = b"".join(struct.pack("<I", (n << 4) | "MIDNSHP=X".index(op)) for n, op in ops)
    struct.pack_into("<H", body, 12, len(ops))
    cols = X.line(q, flag, rid, 0, seq=seq, tags=printed, refs=table).split(b"\t")
    cols[5] = "".join("%d%s" % o for o in ops).encode() or b"*"
    return struct.pack("<i", len(body)) + bytes(body), b"\t".join(cols)


class Rec:
    """A record both formats can hold."""
    def __init__(self, qname, flag, rname, tags=(), **bam_kw):
        self.qname, self.flag, self.rname, self.tags, self.bam_kw = qname, flag, rname, list(tags), bam_kw

    def sam(self):
        return sam_line(self.qname, self.flag, self.rname or "*", self.tags)

    def bam(self, kind):
        return bam_record(kind, self.qname, self.flag, self.rname, self.tags, **self.bam_kw)


def group(kind, qname, scores, first=0, tags=None):
    """Records of one read on consecutive alleles (from alleles(kind)[first] on) with the given AS values.  tags: AS value -> tag
    list (default: AS and NM)."""
    a = alleles(kind)
    tags = tags or (lambda v: [T("AS", v), T("NM", 0)])
    return [Rec(qname, 0 if j == 0 else 256, a[(first + j) % len(a)], tags(v)) for j, v in enumerate(scores)]


def both(name, family, recs, kind="str", aligner="hisat2", **kw):
    """The same records as a SAM-text case and as a BAM case."""
    return [dict(name=name + "[sam]", family=family, locus=kind, aligner=aligner, sam="".join(r.sam() + "\n" for r in recs), **kw),
            dict(name=name + "[bam]", family=family, locus=kind, aligner=aligner, bam=[r.bam(kind) for r in recs], **kw)]


def sam_case(name, family, text, kind="str", aligner="hisat2", **kw):
    return dict(name=name + "[sam]", family=family, locus=kind, aligner=aligner, sam=text, **kw)


def bam_case(name, family, pairs, kind="str", aligner="hisat2", **kw):
    return dict(name=name + "[bam]", family=family, locus=kind, aligner=aligner, bam=pairs, **kw)


def padding(kind="str", n=4, tag="pad"):
    """A few plain groups in front of (or behind) what a case is about: a decline has to come from the record it is about."""
    return [r for g in range(n) for r in group(kind, "%s%d" % (tag, g), [3, 1, 3][:1 + g % 3], first=g)]


# ---- 1. tag sets ---------------------------------------------------------------------------------------------------------------------
def _tag_cases():
    F = "tags"
    recs = padding()
    recs += group("str", "bt2", [-12, -20, -6], 0, bowtie2_tags) + group("str", "bt2b", [-6, -6, -12], 3, bowtie2_tags)
    recs += group("str", "ht2", [5, 3, 7], 1, hisat2_tags) + group("str", "ht2b", [7, 9, 8], 4, hisat2_tags)
    # two AS columns that disagree: the last one counts (by the first ones every record would join)
    recs += group("str", "twice", [5, 3, 7], 2, lambda v: [T("AS", 50), T("NM", 0), T("AS", v), T("YT", "Z", "UU")])
    recs += padding(n=2, tag="tail")
    out = both("aligner_tag_sets", F, recs)
    a = alleles("str")
    pad = "".join(r.sam() + "\n" for r in padding())
    # what int() takes beside plain digits (AS +3, FLAG +0, FLAG -1: every bit set, so skipped), and SEQ of odd and of no length
    plus = [sam_line("plus", "+0", a[0], ["AS:i:+3"]), sam_line("plus", -1, a[3], ["AS:i:90"]), sam_line("plus", 256, a[1], ["AS:i:2"], seq="ACGTA"),
            sam_line("plus", 256, a[2], ["AS:i:+4"], seq="*")]
    out.append(sam_case("plus_signs_negative_flag_and_seq_lengths", F, pad + "".join(l + "\n" for l in plus) + pad))
    out.append(sam_case("as_then_asx", F, pad + sam_line("z", 0, a[0], ["AS:i:4", "ASX:i:7"]) + "\n" + pad, decline="AS", exc=ValueError))
    out.append(sam_case("as_bare", F, pad + sam_line("z", 0, a[0], ["NM:i:0", "AS"]) + "\n" + pad, decline="AS", exc=ValueError))
    return out


# ---- 2. whitespace and line ends (SAM text only) ---------------------------------------------------------------------------------------
def _whitespace_cases():
    F = "whitespace"
    a = alleles("str")
    seps = [" ", "  \t", "\t \t ", "\t\t", " \t"]
    lines = []
    for g in range(6):
        for j, v in enumerate([5, 3, 7]):
            lines.append(sam_line("w%d" % g, 0 if j == 0 else 256, a[(g + j) % len(a)], hisat2_tags(v + g), sep=seps[(g + j) % len(seps)]))
    eleven = sam_line("w2", 4, "*")                                   # eleven columns, and exactly three: skipped, so no AS is asked of them
    three = "w3\t4\t*"
    assert len(eleven.split()) == 11 and len(three.split()) == 3
    mixed = lines[:7] + [eleven] + lines[7:10] + [three] + lines[10:]
    text = "".join(l + ("\n\n" if k % 4 == 1 else "\n\n\n" if k % 4 == 3 else "\n") for k, l in enumerate(mixed))
    out = [sam_case("mixed_blanks_and_blank_lines", F, "\n" + text)]
    out.append(sam_case("crlf_no_final_newline", F, "\r\n".join(lines[:9] + [eleven] + lines[9:])))
    out.append(sam_case("crlf_final_newline", F, "".join(l + "\r\n" for l in lines)))
    out.append(sam_case("lf_no_final_newline", F, "\n".join(lines)))
    pad = "".join(r.sam() + "\n" for r in padding())
    kept11 = sam_line("z", 0, a[0])
    kept3 = "z\t0\t%s" % a[0]
    assert len(kept11.split()) == 11
    out.append(sam_case("kept_line_of_eleven_columns", F, pad + kept11 + "\n" + pad, decline="AS", exc=AssertionError))
    out.append(sam_case("kept_line_of_three_columns", F, pad + kept3 + "\n" + pad, decline="AS", exc=AssertionError))
    return out


# ---- 3. names -------------------------------------------------------------------------------------------------------------------------
def _name_cases():
    F = "names"
    s = strange_names("str")
    recs = padding()
    # records the filters skip, each inside a group it would change if it were kept (it carries the group's id and the best AS)
    for k, key in enumerate(("short", "tiny", "other", "bb_start", "bb_mid", "bb_end", "bb_alone")):
        g = group("str", "n_" + key, [5, 3, 7], k)
        recs += g[:1] + [Rec("n_" + key, 256, s[key], [T("AS", 90), T("NM", 0)])] + g[1:]
    recs += padding(n=2, tag="tail")
    out = both("skipped_names", F, recs)
    # locus names of seven bytes or fewer (the BACKBONE scan needs eight) are kept like any other
    assert all(len(n) <= 7 for n in alleles("th01"))
    out += both("kept_names_of_seven_bytes_or_fewer", F, padding("th01") + group("th01", "s7", [5, 3, 7, 7], 5) + padding("th01", 2, "tail"), kind="th01")
    for key in ("gene", "last_byte", "prefix", "longer"):             # in-gene names the locus does not have
        bad = [Rec("z", 0, s[key], [T("AS", 0), T("NM", 0)])]
        out += both("unknown_name_" + key, F, padding() + bad + padding(n=2, tag="tail"), decline="UNKNOWN_NAME")
    return out


# ---- 4. read ids ----------------------------------------------------------------------------------------------------------------------
def _id_cases():
    F = "ids"
    s = strange_names("str")
    long_a, long_b = "q" * 253 + "a", "q" * 253 + "b"
    recs = []
    for k, q in enumerate(["r1", "r10", "r100", "r10", "r1", "ab", "ac", "x", "y", long_a, long_b, long_a, "x"]):
        recs += group("str", q, [5, 3, 7][:2 + k % 2], k)
    # one group: the filters `continue` before the read id is looked at
    g = group("str", "one", [5, 5, 3, 6], 2)
    recs += g[:2] + [Rec("unm", 4, None), Rec("elsewhere", 0, s["other"], [T("AS", 9)]), Rec("bb", 0, locus("str").allele_names[0], [T("AS", 9)])] + g[2:]
    recs += group("str", "r1", [1, 1], 5)
    return both("prefixes_lengths_and_returning_ids", F, recs)


# ---- 5. AS order and range -------------------------------------------------------------------------------------------------------------
def _as_cases():
    F = "as"
    recs = padding()
    for k, scores in enumerate([[1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [2, 2, 2, 2, 2], [-9, 4, 4, -9, 5], [3, -1, 3, 2, 4, 4, 0]]):
        recs += group("str", "o%d" % k, scores, k)
    for k, scores in enumerate([[I32_MIN, I32_MAX, I32_MIN], [I32_MAX, I32_MIN, I32_MAX], [I32_MIN, I32_MIN, I32_MIN + 1],
                                [I32_MAX - 1, I32_MAX, I32_MAX - 1], [I32_MIN, -1, 0]]):
        recs += group("str", "lim%d" % k, scores, k + 1, lambda v: [T("AS", "i", v), T("NM", 0)])
    out = both("order_and_int32_limits", F, recs)
    # BAM: every integer type at both ends of its range, between a Z and an A tag
    recs = padding()
    for k, t in enumerate("cCsSiI"):
        lo, hi = INT_RANGE[t][0], min(INT_RANGE[t][1], I32_MAX)
        wrap = lambda v, t=t: [T("MD", "Z", "20"), T("AS", t, v), T("XS", "A", "+")]
        recs += group("str", "t%s_up" % t, [lo, hi, lo], k, wrap) + group("str", "t%s_down" % t, [hi, lo, hi], k + 3, wrap)
    out.append(bam_case("integer_types_at_their_ends", F, [r.bam("str") for r in recs]))
    a = alleles("str")
    pad = padding()
    for name, v in (("as_2_pow_31", 2 ** 31), ("as_below_int32", -2 ** 31 - 1), ("as_4e9", 4000000000)):
        g = group("str", "wide", [0, v, 7], 2)
        out.append(sam_case(name, F, "".join(r.sam() + "\n" for r in pad + g + pad), decline="AS"))
    for name, v in (("as_I_2_pow_31", 2 ** 31), ("as_I_max", 2 ** 32 - 1)):
        g = group("str", "wide", [0, v, 7], 2, lambda x: [T("AS", "I" if x > 7 else "C", x)])
        out.append(bam_case(name, F, [r.bam("str") for r in pad + g + pad], decline="AS"))
    # AS 0, 4000000000, 7 on alleles a, b, c: the class is a-b (read through int32 it would be a-c)
    g = [Rec("wide", 0, a[0], [T("AS", "C", 0)]), Rec("wide", 256, a[1], [T("AS", "I", 4000000000)]), Rec("wide", 256, a[2], [T("AS", "C", 7)])]
    out.append(bam_case("as_I_4e9_group_of_three", F, [r.bam("str") for r in g], decline="AS"))
    return out


# ---- 6. the BAM aux walk ---------------------------------------------------------------------------------------------------------------
def _aux_cases():
    F = "aux"
    a = alleles("str")
    others = [T("XA", "A", "+"), T("XF", "f", 1.5), T("XZ", "Z", "10A9"), T("XH", "H", "1AE3")]
    vals = {"c": (-1, 2, 3), "C": (1, 2, 255), "s": (-300, 2, 3), "S": (1, 2, 65535), "i": (-70000, 2, 3), "I": (1, 2, 4000000000), "f": (1.5, 2.0, -0.25)}
    for sub in "cCsSiIf":
        others += [T("XB", "B", (sub, ())), T("XB", "B", (sub, vals[sub]))]
    recs = padding()
    for k, o in enumerate(others):                                     # AS behind the tag, in front of it, between two of it
        shapes = [lambda v: [o, T("AS", v)], lambda v: [T("AS", v), o], lambda v: [o, T("AS", v), o]]
        recs += [Rec("aux%d" % k, 0 if j == 0 else 256, a[(k + j) % len(a)], shapes[j](v)) for j, v in enumerate([5, 3, 7])]
    recs += group("str", "two_types", [5, 3, 300], 1, lambda v: [T("AS", "c", 100), T("NM", 0), T("AS", "S" if v > 255 else "C", v)])
    recs += group("str", "two_types_b", [5, 3, 7], 2, lambda v: [T("AS", "i", 100000), T("AS", "c", v)])
    for k, n_cigar in enumerate((0, 1, 3)):
        for j, l_seq in enumerate((0, 5, 20)):
            g = group("str", "cig%d_seq%d" % (n_cigar, l_seq), [5, 3, 7], k + j, hisat2_tags)
            for r in g:
                r.bam_kw = dict(n_cigar=n_cigar, l_seq=l_seq)
            recs += g
    recs += group("str", "q", [5, 3, 7], 4, bowtie2_tags) + group("str", "q" * 253 + "z", [5, 3, 7], 5, bowtie2_tags)    # l_read_name 2, 255
    g = group("str", "no_ref", [5, 3, 7], 6)
    recs += g[:1] + [Rec("no_ref", 256, None, [T("AS", 90)]), Rec("no_ref", 256, locus("str").allele_names[0], [T("AS", 90)])] + g[1:]
    recs += padding(n=2, tag="tail")
    pairs = [r.bam("str") for r in recs]
    out = [bam_case("tags_around_as_cigar_seq_and_names", F, pairs, block_size=700)]
    pad = [r.bam("str") for r in padding()]
    one = lambda tags, **kw: [Rec("z", 0, a[0], tags).bam("str")] if tags is not None else [bam_record("str", "z", 0, a[0], **kw)]
    out.append(bam_case("as_int_then_as_z", F, pad + one([T("AS", 5), T("AS", "Z", "x")]) + pad, decline="AS", exc=ValueError))
    out.append(bam_case("as_float_alone", F, pad + one([T("AS", "f", 1.5)]) + pad, decline="AS", exc=ValueError))
    # whitespace inside a tag moves the columns the reference splits on: here it makes a second AS column, which then counts
    g = group("str", "blank", [5, 3, 7], 1)
    g[1].tags += [T("XX", "Z", "a AS:i:50")]
    out.append(bam_case("z_tag_holding_a_blank", F, pad + [r.bam("str") for r in g] + pad, decline="RECORD"))
    g = group("str", "blank", [5, 3, 7], 1, lambda v: [T("XA", "A", " "), T("AS", v)])
    out.append(bam_case("a_tag_blank", F, pad + [r.bam("str") for r in g] + pad, decline="RECORD"))
    bad = "malformed BAM record"
    out.append(bam_case("aux_past_the_block", F, pad + one(None, aux=tag_aux(T("AS", 5)) + b"NMi\x01\x00", printed=["AS:i:5"]) + pad, decline="RECORD", error=bad))
    out.append(bam_case("aux_unknown_type", F, pad + one(None, aux=tag_aux(T("AS", 5)) + b"XQq\x01", printed=["AS:i:5"]) + pad, decline="RECORD", error=bad))
    out.append(bam_case("b_array_past_the_block", F, pad + one(None, aux=tag_aux(T("AS", 5)) + b"XBBs" + struct.pack("<I", 100) + b"\1\0\2\0\3\0",
                                                               printed=["AS:i:5"]) + pad, decline="RECORD", error=bad))
    return out


# ---- 7. the group kernel ---------------------------------------------------------------------------------------------------------------
def _group_cases():
    F = "groups"
    n_str = len(alleles("str"))
    assert n_str >= 11
    out = []
    distinct = lambda q, n, first=0: group("str", q, [4] * n, first)
    twelve = group("str", "twelve", [4] * 12, 0)                      # twelve records, nine distinct names
    for j in (9, 10, 11):
        twelve[j].rname = twelve[j - 9].rname
    mid = padding(n=2)
    for n in (9, 10, 11):
        mid += distinct("mid%d" % n, n, n) + group("str", "sep%d" % n, [2, 2], n)
    mid += twelve + group("str", "end", [1], 3)
    out += both("bowtie2_9_10_11_names_in_the_middle", F, mid, aligner="bowtie2")
    for n in (9, 10, 11):
        out += both("bowtie2_%d_names_last" % n, F, padding(n=3) + distinct("last", n, 1), aligner="bowtie2")
    out += both("bowtie2_twelve_records_nine_names_last", F, padding(n=3) + twelve, aligner="bowtie2")
    # one group of 1000 records over 300 names, all AS equal: names descending, ascending, shuffled
    names = sorted(alleles("hla"))
    order = [names[k % len(names)] for k in range(1000)]
    big = padding("hla", 2)
    for q, seq in (("down", sorted(order, reverse=True)), ("up", sorted(order)), ("mixed", random.Random(11).sample(order, len(order)))):
        big += [Rec(q, 0 if j == 0 else 256, n, [T("AS", -3)]) for j, n in enumerate(seq)] + group("hla", "sep_" + q, [1, 1], 7)
    out += both("group_of_1000_records", F, big, kind="hla")
    out += both("single_group", F, group("str", "only", [5, 3, 7], 0))
    out += both("single_kept_record", F, [Rec("u", 4, None)] + group("str", "only", [5], 0) + [Rec("o", 0, strange_names("str")["other"], [T("AS", 1)])])
    out += both("no_kept_record", F, [Rec("u", 4, None), Rec("o", 0, strange_names("str")["other"], [T("AS", 1)]),
                                      Rec("b", 0, locus("str").allele_names[0], [T("AS", 1)]), Rec("u2", 4, alleles("str")[0])])
    out.append(sam_case("no_line", F, ""))
    for name, last in (("unmapped", Rec("u", 4, None)), ("on_another_gene", Rec("o", 0, strange_names("str")["other"], [T("AS", 1)])),
                       ("on_backbone", Rec("b", 0, locus("str").allele_names[0], [T("AS", 1)]))):
        for aligner in ("hisat2", "bowtie2"):
            out += both("last_line_%s_%s" % (name, aligner), F, padding(n=5) + [last], aligner=aligner)
    return out


# ---- 8. sizes --------------------------------------------------------------------------------------------------------------------------
def sized_sam(shape, s):
    """SAM text over the 300-allele locus that puts ONE of the route's four scanned sizes at s (the route scans, in this order,
    the keep flag of every line, the head flag of every kept record, the first flag of every group and the length of every class):
      "lines"    s kept lines, each a group of its own, with 37 lines the filters skip (unmapped, another gene, BACKBONE in turn)
                 spread evenly among them (the j-th in front of kept line j * s // 37): the first scan runs over s + 37 keep flags
                 with zeros among them and leaves s kept records;
      "kept"     groups of 1, 2, 3, 1, 2, 3, ... records, the last one cut so that exactly s records are kept; there is no other
                 line, so here the line count, the first scan's size, is s as well;
      "groups"   exactly s groups of 1 to 3 records (their sizes drawn at random);
      "classes"  exactly s groups of two records each, every group on another pair of names (pairs in lexicographic order of the
                 name indices), so s groups make s distinct classes.
    The ids are distinct, AS differs within a group so that some records do not join."""
    a = alleles("hla")
    rng = random.Random(1000 * SHAPES.index(shape) + s)
    lines = []
    if shape == "lines":
        skip = [sam_line("u", 4, "*"), sam_line("o", 0, "ZZ9*1", ["AS:i:1"]), sam_line("b", 0, locus("hla").allele_names[0], ["AS:i:1"])]
        n_skip = 0
        for k in range(s):
            for j in range(37):                                       # the j-th skipped line stands in front of kept line j * s // 37
                if (j * s) // 37 == k:
                    lines.append(skip[n_skip % 3])
                    n_skip += 1
            lines.append(sam_line("r%d" % k, 0, a[rng.randrange(len(a))], ["AS:i:%d" % rng.randint(-40, 0)]))
        assert n_skip == 37
    elif shape in ("kept", "groups"):
        g = 0
        while (len(lines) if shape == "kept" else g) < s:
            k = 1 + g % 3 if shape == "kept" else rng.randint(1, 3)
            if shape == "kept":
                k = min(k, s - len(lines))
            base = rng.randint(-40, 0)
            lines += [sam_line("r%d" % g, 0 if j == 0 else 256, a[rng.randrange(len(a))], ["AS:i:%d" % (base + rng.choice([0, 0, 1, -1]))])
                      for j in range(k)]
            g += 1
    else:
        x, y = 0, 1
        for g in range(s):
            lines += [sam_line("r%d" % g, 0, a[x], ["AS:i:0"]), sam_line("r%d" % g, 256, a[y], ["AS:i:%d" % (g % 2)])]
            y += 1
            if y == len(a):
                x, y = x + 1, x + 2
    return "".join(l + "\n" for l in lines)


def sized_counts(text):
    """(lines, kept records, groups, classes) of a sized_sam text, by the statement's rules."""
    gene = locus("hla").gene
    lines = linear_ref.records(text)
    kept = [l.split() for l in lines]
    kept = [c for c in kept if not int(c[1]) & 4 and c[2].startswith(gene) and "BACKBONE" not in c[2]]
    groups = sum(1 for k, c in enumerate(kept) if k == 0 or kept[k - 1][0] != c[0])
    return len(lines), len(kept), groups, len(linear_ref.gene_counts_and_classes(lines, gene, "hisat2")[1])


FAMILIES = ("tags", "whitespace", "names", "ids", "as", "aux", "groups")


@functools.lru_cache(None)
def cases():
    out = _tag_cases() + _whitespace_cases() + _name_cases() + _id_cases() + _as_cases() + _aux_cases() + _group_cases()
    assert len({c["name"] for c in out}) == len(out) and {c["family"] for c in out} == set(FAMILIES)
    return out


# ---- a case against the statement ------------------------------------------------------------------------------------------------------
def case_lines(case):
    """The lines the reference's loop reads for the case."""
    if "sam" in case:
        return linear_ref.records(case["sam"])
    return linear_ref.records(b"".join(l for _, l in case["bam"]))


def statement(case):
    """(counts, classes) as ordered lists, or the exception type the statement raises."""
    try:
        c, k = linear_ref.gene_counts_and_classes(case_lines(case), locus(case["locus"]).gene, case["aligner"])
    except (ValueError, AssertionError) as e:
        return type(e)
    return list(c.items()), list(k.items())


def assert_nothing_to_decline(case):
    """A case that is to stay on the device holds nothing the kernels decline by their own rules: a line of fewer than three
    columns, a FLAG that is no integer, an unknown in-gene name, a kept record without an integer AS inside int32, whitespace
    inside a BAM tag."""
    gene = locus(case["locus"]).gene
    known = set(locus(case["locus"]).allele_names)
    for l in case_lines(case):
        cols = l.split()
        assert len(cols) >= 3, (case["name"], l)
        if int(cols[1]) & 4 or not cols[2].startswith(gene) or "BACKBONE" in cols[2]:
            continue
        assert cols[2] in known, (case["name"], cols[2])
        tag = [x for x in cols[11:] if x.startswith("AS")]
        assert tag and I32_MIN <= int(tag[-1][5:]) <= I32_MAX, (case["name"], l)
    if "bam" in case:                                                 # (a blank inside a tag would show as a column too many)
        assert all(len(l.split(b"\t")) == len(l.split()) for _, l in case["bam"]), case["name"]


def run(case, pl, front, tmp_dir):
    """The case through typing.linear_counts under the given front.  -> ((counts, classes) or the exception, (route, decline))"""
    import importlib
    from hisatgenotype_amd import engine
    ht = importlib.import_module("hisatgenotype_amd.typing")
    path = None
    if "bam" in case:
        path = os.path.join(str(tmp_dir), re.sub(r"\W", "_", case["name"]) + ".bam")
        with open(path, "wb") as f:
            f.write(X.bgzf(X.header(refs(case["locus"])) + b"".join(r for r, _ in case["bam"]), case.get("block_size", 0xff00))[0])
    with engine.test_switches(front=front):
        try:
            res = ht.linear_counts(pl, case.get("sam"), case["aligner"], alignment_file=path)
            got = (list(res.counts.items()), list(res.classes.items()))
        except (ValueError, AssertionError) as e:
            got = e
        return got, engine.front_last()


def check(case, pl, front, tmp_dir):
    """The case's result, exception or message under `front` is the statement's; on the device front the call also reports the
    route the case names: (2, 0), or (0, its decline code)."""
    want = statement(case) if not case.get("error") else None        # (damage the statement cannot see)
    assert (want if isinstance(want, type) else None) == case.get("exc"), (case["name"], want)
    got, route = run(case, pl, front, tmp_dir)
    if case.get("error"):
        assert isinstance(got, ValueError) and re.search(case["error"], str(got)), (case["name"], got)
    elif isinstance(want, type):
        assert type(got) is want, (case["name"], got)
    else:
        assert got == want, (case["name"], got, want)
    if front == "device":
        assert route == ((0, DECLINE[case["decline"]]) if case.get("decline") else (2, 0)), (case["name"], route)
    else:
        assert route == (0, 2), (case["name"], route)                  # HGX_LIN_DECLINE_FORCED
    return route
