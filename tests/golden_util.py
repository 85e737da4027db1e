"""Helpers to read the golden fixtures recorded from the real reference (tests/golden/make_golden.py)."""
import functools
import gzip
import json
import os

import numpy as np

from hisatgenotype_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = ["hla_small_pair", "hla_small_single", "hla_errors_filters", "hla_mid_real", "hla_keep_low",
       "hla_single_end", "hla_novel_sample", "hla_insertions", "hla_7000", "codis_like", "codis_d18s51"]
SMALL = [n for n in ALL if n != "hla_7000"]
LEAN = ["hla_7000_10k", "codis_10k"]      # BASELINE configs[0] at full size: SAM, EM calls (with their class dicts) and report only

# Long and odd-length reads and the device front end's fixed scratch limits (csrc/hgx_front_core.hpp: FE_MAX_*), kept out of ALL so
# that no downstream test changes: 2x251; eight lengths around the decode kernel's staging limits in one stream; a 2x301 sample dense
# enough to outgrow FE_MAX_CMP; three families of single reads that cross FE_MAX_CMP / FE_MAX_OPS / FE_MAX_ZS one step at a time.
LONG = ["hla_long_251", "hla_len_edges", "hla_dense_301", "hla_cap_cmp", "hla_cap_ops", "hla_cap_zs"]
LONG_TAKEN = ["hla_long_251", "hla_len_edges"]             # the device front end takes these whole
LONG_FAMILIES = {"hla_cap_cmp": "cmp", "hla_cap_ops": "ops", "hla_cap_zs": "zs"}   # one single-end read per line; the limit each family crosses
FE_MAX_CMP, FE_MAX_OPS, FE_MAX_ZS, FE_E_CAP = 64, 24, 48, 106   # csrc/hgx_front_core.hpp (the decline code as front_last reports it)


def family_members(fx):
    """A cap family line by line: (read name, that line as a stream of its own, index of its record in fx["records"], entries of
    the reference's cmp_list2, CIGAR ops, Zs items).  The counts are the reference's own (the recorded list) and the input's (the SAM
    line), not the code's."""
    import re
    lines = [l for l in fx["sam"].split("\n") if l]
    assert len(lines) == len(fx["records"]), "the reference dropped a family member"
    out = []
    for k, l in enumerate(lines):
        f = l.split("\t")
        zs = [t[5:] for t in f[11:] if t.startswith("Zs:Z:")]
        out.append((f[0], l + "\n", k, len(fx["records"][k]["cmp"]), len(re.findall(r"\d+[A-Z=]", f[5])), len(zs[0].split(",")) if zs else 0))
    return out


def member_taken(kind, n_cmp, n_ops, n_zs):
    """Only the family's own limit may separate its members: the other counts stay below theirs."""
    assert (kind == "cmp" or n_cmp <= FE_MAX_CMP) and (kind == "ops" or n_ops <= FE_MAX_OPS) and (kind == "zs" or n_zs <= FE_MAX_ZS)
    return {"cmp": n_cmp <= FE_MAX_CMP, "ops": n_ops <= FE_MAX_OPS, "zs": n_zs <= FE_MAX_ZS}[kind]


def junk_nibble_bam(src, dst):
    """Copy a BAM with the UNUSED low nibble of every odd-length record's last SEQ byte set to a value that changes from record to
    record (writers leave it 0; nothing says they must).  Returns the number of records changed."""
    import struct
    import zlib
    from hisatgenotype_amd import bamio
    raw = bytearray(b"".join(bamio._bgzf_blocks(open(src, "rb").read())))
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 4 + l_name + 4
    n = 0
    while p < len(raw):
        size, = struct.unpack_from("<i", raw, p)
        l_rn, n_cig, l_seq = raw[p + 12], struct.unpack_from("<H", raw, p + 16)[0], struct.unpack_from("<i", raw, p + 20)[0]
        if l_seq & 1:
            raw[p + 36 + l_rn + 4 * n_cig + l_seq // 2] |= 1 + n % 15
            n += 1
        p += 4 + size
    with open(dst, "wb") as fo:
        for i in range(0, len(raw), 0xff00):
            blk = bytes(raw[i:i + 0xff00])
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            cdata = comp.compress(blk) + comp.flush()
            fo.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata +
                     struct.pack("<II", zlib.crc32(blk) & 0xffffffff, len(blk)))
        fo.write(bamio._BGZF_EOF)
    return n


@functools.lru_cache(maxsize=None)
def load(name):
    with gzip.open(os.path.join(GOLDEN_DIR, name + ".json.gz"), "rb") as f:
        fx = json.loads(f.read().decode())
    if fx["locus"] is not None:
        loc = synth.Locus.from_json(fx["locus"])
    else:
        loc = synth.make_hla_like_locus(**fx["locus_params"])
        assert loc.allele_names == fx["allele_names"], "generator drifted from the recorded fixture"
    fx["_locus"] = loc
    return fx


def class_key(fx, cid):
    """Decode a recorded class id back to the reference's '-'.join(sorted(names)) key."""
    bits = int(fx["classes"][cid], 16)
    names = fx["allele_names"]
    out = []
    i = 0
    while bits:
        if bits & 1:
            out.append(names[i])
        bits >>= 1
        i += 1
    return "-".join(sorted(out))


def class_bits(fx, cid, n_alleles):
    """Recorded class as a bitset over scored alleles (Gene_names minus the backbone at index 0)."""
    bits = int(fx["classes"][cid], 16) >> 1
    w64 = (n_alleles + 63) // 64
    out = np.zeros(w64, dtype=np.uint64)
    for w in range(w64):
        out[w] = (bits >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def parse_ht(ht, var_index):
    """'left-id-..-right' -> (left, right, [var indices; -1 for nv ids])."""
    f = ht.split("-")
    ids = [var_index.get(v, -1) if v.startswith("hv") else -1 for v in f[1:-1]]
    return int(f[0]), int(f[-1]), ids
