"""The alignment reader (csrc/hgx_bam.cpp with hgx_bai.cpp, hgx_bgzf.cpp) as a stand-alone host program under AddressSanitizer and
UBSan (no GPU, not through python's process): builds tools/reader_host_check.cpp, writes the input files of every route the reader
has -- the hand-overs to the device front end's callbacks, the host BAM and SAM paths, region lists on each, damaged files, the
many-task reader -- and prints the program's record of what the reader gave back and told its callbacks.

Usage: tools/reader_host_check.py [--plain] [--no-big] [-o dump.txt]
  --plain   build without the sanitizers;  --no-big   leave the 64 MB text out;  -o   write the dump there instead of stdout
Two dumps of two versions of the reader must be identical: `diff` them.  tests/test_reader_host.py builds the same program and holds
parts of the dump to the project's Python statements of the formats."""
import os
import struct
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hisat-genotype_amd", "csrc")
UNITS = ("hgx_bam", "hgx_bai", "hgx_bgzf", "hgx_host")
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_REGIONS = 8                                   # hgx.h: HGX_MAX_REGIONS


def build(exe, sanitize=True, objects=False):
    """`objects`: link the library's own objects of the reader's units (they are fresh after the library was built) instead of
    compiling the units again."""
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-g", "-O1", "-pthread"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tools", "reader_host_check.cpp")]
    cmd += [os.path.join(CSRC, u + (".o" if objects else ".cpp")) for u in UNITS]
    subprocess.check_call(cmd + ["-lz", "-ldl", "-o", exe])
    return exe


def bgzf(data, block=0xff00, eof=True):
    """`data` as BGZF blocks of `block` payload bytes."""
    from hisatgenotype_amd import bamio
    out = bytearray()
    for o in range(0, len(data), block):
        raw = bytes(data[o:o + block])
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(raw) + c.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw))
    return bytes(out) + (bamio._BGZF_EOF if eof else b"")


def inflated(path):
    from hisatgenotype_amd import bamio
    with open(path, "rb") as f:
        return b"".join(bamio._bgzf_blocks(f.read()))


def decoy_stream():
    """The inflated BAM of test_bam_record_chain_walked_in_ranges_is_exact: a record whose B:C tag holds a chain of plausible records."""
    def rec(qname, pos0, tags=b""):
        body = struct.pack("<iiBBHHHiiii", 0, pos0, len(qname) + 1, 60, 4681, 1, 0, 4, -1, -1, 0) + qname.encode() + b"\0"
        body += struct.pack("<I", (4 << 4) | 0) + bytes([0x12, 0x48]) + bytes([30, 30, 30, 30]) + tags
        return struct.pack("<i", len(body)) + body
    fake = rec("decoy", 7)
    tag = b"XBBC" + struct.pack("<I", 120 * len(fake)) + fake * 120
    recs = [rec("a%d" % k, 10 + k) for k in range(3)] + [rec("big", 50, tag)] + [rec("z%d" % k, 90 + k) for k in range(3)]
    return b"BAM\x01" + struct.pack("<iii", 0, 1, 5) + b"chr1\0" + struct.pack("<i", 1000) + b"".join(recs)


def region_sets():
    """name -> region list, for the fixture of tests/bai_cases.py (references 6, 7, 8)."""
    import bai_cases
    g = bai_cases.region_grid()
    left = bai_cases.locus_span()[0]
    return {"none": None, "whole": ["7"], "span": ["6:%d-%d" % (left + 100, left + 700)], "overlapping": g["two, overlapping"], "unknown": ["nope"],
            "inverted": ["6:2000-1000"], "too many": ["6:%d-%d" % (left + 1 + 300 * k, left + 250 + 300 * k) for k in range(MAX_REGIONS)] + ["7:1-3000"]}


# route name -> the case's fields (the file, what the caller offers, what its callbacks answer)
ROUTES = {
    "index, splice taken": dict(path="fx.bam", sw="bai:force", keep=1, walk=1, min=1, splice=0),
    "index, splice refused": dict(path="fx.bam", sw="bai:force", keep=1, walk=1, min=1, splice=1),
    "index, no defer_walk": dict(path="fx.bam", sw="bai:force", keep=1, walk=0, min=1, splice=0),
    "bgzf, inflate taken": dict(path="fx.bam", keep=1, walk=1, min=1, inflate=0, early=1, on_raw=1),
    "bgzf, inflate refused": dict(path="fx.bam", keep=1, walk=1, min=1, inflate=1, early=1, on_raw=1),
    "bgzf, host walk": dict(path="fx.bam", keep=1),
    "bgzf, host text": dict(path="fx.bam", keep=0),
    "raw bam, handed over": dict(path="raw.bam", keep=1, walk=1, min=1, on_raw=1),
    "raw bam, host walk": dict(path="raw.bam", keep=1),
    "sam text, host": dict(path="fx.sam", keep=1),
    "sam text, handed over": dict(path="fx.sam", keep=1, text=1, min=1, on_raw=1),
}


def write_cases(d, big=True):
    """Writes the input files into directory `d` and returns the manifest's path."""
    import bai_cases
    import bai_ref
    from hisatgenotype_amd import bamio, synth
    cases = []

    def case(name, **kw):
        regions = kw.pop("regions", None)
        if regions is not None:
            kw["regions"] = ";".join(regions)
        cases.append("\t".join(["case=" + name] + ["%s=%s" % (k, v) for k, v in kw.items()]))

    def put(name, data):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data if isinstance(data, bytes) else data.encode())

    # ---- files -------------------------------------------------------------------------------------------------------------------
    fx = bai_cases.write_fixture(d, 700, name="fx.bam")                       # coordinate-sorted, three references, 700-byte blocks
    put("fx.bam.bai", bai_ref.build(fx))
    stream = inflated(fx)
    put("raw.bam", stream)
    lines = list(bai_cases.sam_lines())
    put("fx_plain.sam", "\n".join(lines) + "\n")
    put("fx.sam", "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bai_cases.REFS) + "\n".join(lines) + "\n")
    put("fx.sam.gz", bgzf(("\n".join(lines) + "\n").encode()))
    loc = bai_cases.the_locus()
    grouped = synth.simulate_sam_fast(loc, synth.pick_sample(loc, 7), 300, err_rate=0.003, seed=11)         # name-grouped, as an aligner writes
    bamio.write_bam_native(os.path.join(d, "grp.bam"), grouped, [(loc.ref_allele, len(loc.backbone))])
    put("grp.sam", grouped)
    rows = [l for l in grouped.split("\n") if l]
    put("crlf.sam", "@HD\tVN:1.0\r\n" + "\r\n".join(rows[:40]) + "\r\n\r\n@CO\tin between\r\n" + "\r\n".join(rows[40:80]))       # (no final newline)
    put("decoy.bam", bgzf(decoy_stream(), 3000))
    put("other.bin", bgzf(b"not a BAM at all\n" * 50))
    # ---- every route under every region list ----------------------------------------------------------------------------------------
    for rname, route in ROUTES.items():
        for sname, regs in region_sets().items():
            kw = dict(route, nt=3)
            if "splice" in kw and sname == "span":
                kw["dump_parts"] = "parts_%d.bin" % len(cases)
            if kw.get("walk") or kw.get("text"):
                kw["dump_raw"] = "raw_%d.bin" % len(cases)
            case("%s / %s" % (rname, sname), regions=regs, **kw)
    case("index that names no block", regions=["8"], **dict(ROUTES["index, splice taken"], nt=2))
    case("index, nothing there", regions=["6:130001-130100"], **dict(ROUTES["index, splice refused"], nt=2))
    case("index switched off", regions=["7"], path="fx.bam", sw="bai:off", keep=1, nt=2)
    case("index, small file", regions=["7"], path="fx.bam", keep=1, walk=1, min=1, splice=0, nt=2)
    case("bgzf, below the gate", path="fx.bam", keep=1, walk=1, min=1 << 30, inflate=0, early=1, nt=2)
    case("bgzipped sam text", path="fx.sam.gz", keep=1, walk=1, min=1, inflate=0, early=1, on_raw=1, nt=2)
    case("bgzf that is no bam", path="other.bin", keep=1, walk=1, min=1, inflate=0, early=1, nt=2)
    case("name-grouped bam, file order", path="grp.bam", keep=1, order=1, nt=2)
    # ---- host BAM -------------------------------------------------------------------------------------------------------------------
    for keep in (1, 0):
        case("grouped bam keep_binary=%d" % keep, path="grp.bam", keep=keep, nt=3)
    for nt in (1, 2, 3, 7):
        for f in ("fx.bam", "decoy.bam"):
            case("chain in ranges, %s, %d threads" % (f, nt), path=f, keep=0, nt=nt, sw="bam_chain_min:0")
        case("chain in ranges, region, %d threads" % nt, path="fx.bam", keep=1, nt=nt, sw="bam_chain_min:0", regions=region_sets()["overlapping"])
    # ---- host SAM -------------------------------------------------------------------------------------------------------------------
    case("sam, header lines, CRLF, no final newline", path="crlf.sam", keep=0, nt=3)
    case("sam, grouped", path="grp.sam", keep=0, nt=1)
    case("sam above 4 MB", path="big4.sam", grow="fx_plain.sam:%d" % (5 << 20), nt=3)
    case("sam above 4 MB, regions", path="big4.sam", grow="fx_plain.sam:%d" % (5 << 20), nt=5, regions=region_sets()["overlapping"])
    for nt in (1, 3, 13):
        case("sam above 8 MB, %d threads" % nt, path="big8.sam", grow="fx_plain.sam:%d" % (9 << 20), nt=nt)
    case("sam above 8 MB, regions, on_raw", path="big8.sam", grow="fx_plain.sam:%d" % (9 << 20), nt=3, on_raw=1, regions=region_sets()["span"])
    case("sam above 8 MB, handed over", path="big8.sam", grow="fx_plain.sam:%d" % (9 << 20), nt=3, on_raw=1, keep=1, text=1, min=1)
    if big:
        for ph in ("1", "3", None):
            kw = dict(path="big64.sam", grow="fx_plain.sam:%d" % (65 << 20), nt=4, on_raw=1)
            if ph:
                kw["env"] = "HGX_READ_PHASES:" + ph
            case("sam above 64 MB, phases %s" % (ph or "as built"), **kw)
    # ---- damaged files -----------------------------------------------------------------------------------------------------------------
    l_text = struct.unpack_from("<i", stream, 4)[0]
    body0 = 12 + l_text
    for _ in bai_cases.REFS:
        body0 += 8 + struct.unpack_from("<i", stream, body0)[0]
    cuts = {"inside the magic": 3, "inside the header's length": 10, "inside the header text": 8 + l_text // 2, "inside the reference list": 12 + l_text + 9,
            "inside a record": body0 + 100, "inside a record's block_size": len(stream) - 2, "behind the header": body0}
    for k, (what, at) in enumerate(cuts.items()):
        put("cut%d.bam" % k, bgzf(stream[:at], 700))
        put("cut%d.raw" % k, stream[:at])
        case("bgzf bam cut %s" % what, path="cut%d.bam" % k, keep=1, nt=2)
        case("bgzf bam cut %s, offered to the device" % what, path="cut%d.bam" % k, keep=1, walk=1, min=1, inflate=0, early=1, nt=2)
        case("raw bam cut %s" % what, path="cut%d.raw" % k, keep=0, nt=2)
    with open(fx, "rb") as f:
        whole = bytearray(f.read())
    hit, off = bytearray(whole), 0
    while off < len(whole) // 2:                                               # a payload byte of a block in the middle
        off += struct.unpack_from("<H", whole, off + 16)[0] + 1
    hit[off + 18 + 5] ^= 0x55
    put("damaged.bam", bytes(hit))
    put("damaged.bam.bai", bai_ref.build(fx))
    case("damaged payload", path="damaged.bam", keep=1, nt=3)
    case("damaged payload, through the index", path="damaged.bam", keep=1, nt=3, sw="bai:force", regions=["6", "7"])
    put("halfblock.bam", bytes(whole[:len(whole) // 2]))
    case("file cut inside a block", path="halfblock.bam", keep=1, nt=2)
    case("file cut inside a block, offered to the device", path="halfblock.bam", keep=1, walk=1, min=1, inflate=0, early=1, nt=2)
    put("empty.sam", b"")
    case("empty file", path="empty.sam", keep=0, nt=2)
    case("missing file", path="nowhere.bam", keep=1, nt=2)
    case("missing file, regions", path="nowhere.bam", keep=1, nt=2, sw="bai:force", regions=["6"])
    # ---- the many-task reader ------------------------------------------------------------------------------------------------------------
    left = bai_cases.locus_span()[0]
    case("tasks: index, whole file, no bam", tasks="fx.bam@6:%d-%d,grp.bam@,other.bin@" % (left + 100, left + 700), sw="bai:force", nt=3)
    case("tasks: too many regions, unknown file", tasks="fx.bam@%s,nowhere.bam@" % ";".join(region_sets()["too many"]), sw="bai:force", nt=2)
    manifest = os.path.join(d, "cases.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(cases) + "\n")
    return manifest


def run(exe, d, manifest):
    return subprocess.run([exe, os.path.basename(manifest)], cwd=d, check=True, stdout=subprocess.PIPE).stdout.decode()


def parse(dump):
    """case name -> its lines."""
    out, cur = {}, None
    for line in dump.split("\n"):
        if line.startswith("== case "):
            cur = out.setdefault(line[8:], [])
        elif cur is not None and line:
            cur.append(line)
    return out


if __name__ == "__main__":
    import tempfile
    import hisatgenotype_amd  # noqa: F401
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(os.path.join(tmp, "reader_host_check"), sanitize="--plain" not in sys.argv)
        text = run(exe, tmp, write_cases(tmp, big="--no-big" not in sys.argv))
    if "-o" in sys.argv:
        with open(sys.argv[sys.argv.index("-o") + 1], "w") as fo:
            fo.write(text)
    else:
        sys.stdout.write(text)
