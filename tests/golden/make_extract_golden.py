#!/usr/bin/env python3
"""Record the extract_* fixtures from the REAL reference's extract_reads (hisatgenotype_typing_process.py:1330-1784).

    python tests/golden/make_extract_golden.py [name ...]

The reference is run under Python 3 through make_golden.setup_reference(), with stub `hisat2` / `bowtie2` executables of our own
on PATH that print the scenario's SAM, and placeholder index files for check_base.  The reference does not wait for its `gzip`
children: the recorder polls until every output passes `gzip -t` with a stable size.  A fixture holds data only: the SAM text,
the .locus text, the arguments, {file name: decompressed text}, the returned fname_list and the exception type, if any."""
import gc
import gzip
import json
import os
import random
import shutil
import stat
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

LOCUS = "".join("\t".join(r) + "\n" for r in [
    ("HLA", "A*BACKBONE", "6", "1000", "2000", "1000", "+"),
    ("HLA", "B*BACKBONE", "6", "1500", "2500", "1000", "+"),          # overlaps HLA-A: one family, the first region breaks
    ("CODIS", "TH01*BACKBONE", "6", "1800", "2200", "400", "+"),      # another family inside HLA-A/B: never reached at 1800-1999
    ("HLA", "C*BACKBONE", "6", "5000", "6000", "1000", "-"),
    ("CODIS", "D18S51*BACKBONE", "18", "300", "900", "600", "+"),
    ("CYP", "CYP2D6*BACKBONE", "22", "100", "700", "600", "-"),
])


def rec(name, flag, chrom, pos, seq, qual=None, tags=()):
    qual = qual if qual is not None else "".join(chr(33 + (7 * i + len(seq)) % 40) for i in range(len(seq)))
    return "\t".join([name, str(flag), chrom, str(pos), "60", "%dM" % len(seq), "=", "0", "0", seq, qual] + list(tags)) + "\n"


def rseq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


HEADER = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:6\tLN:100000\n@PG\tID:hisat2\n"


def pair(rng, name, c1, p1, c2, p2, nh1=1, nh2=1, f1=0x43, f2=0x83, n=20):
    t1 = ("AS:i:-3", "ZS:i:-9", "NH:i:%d" % nh1) if nh1 is not None else ("YT:Z:UP",)
    t2 = ("AS:i:0", "NH:i:%d" % nh2, "YT:Z:CP") if nh2 is not None else ("YT:Z:UP",)
    return rec(name, f1, c1, p1, rseq(rng, n), tags=t1) + rec(name, f2, c2, p2, rseq(rng, n), tags=t2)


def scenarios():
    S = {}
    base = dict(database_list=[], aligner="hisat2", paired=True, simulation=False, fastq=True)

    def add(name, sam, **kw):
        a = dict(base)
        a.update(kw)
        S[name] = dict(sam=sam, args=a)

    rng = random.Random(11)
    add("hisat2_mixed_nh", HEADER +
        pair(rng, "m1", "6", 1201, "6", 1401) + pair(rng, "m2", "6", 1201, "6", 9000, nh1=2, nh2=2) +
        pair(rng, "m3", "6", 9000, "6", 9200) + pair(rng, "m4", "6", 5500, "6", 5600, nh1=3, nh2=1) +
        pair(rng, "m5", "22", 150, "22", 9000, nh1=1, nh2=4) + pair(rng, "m6", "7", 1500, "7", 1600))
    add("right_mate_quirk",
        pair(rng, "q1", "6", 9000, "6", 1300, nh1=5, nh2=5) +                      # right mate in a region, NH != 1: a hit by read2_first
        pair(rng, "q2", "6", 1300, "6", 9000, nh1=5, nh2=5) +                      # the left mate alone: no hit
        "".join([rec("q3", 0x43, "6", 9000, rseq(rng, 20), tags=("NH:i:2",)),
                 rec("q3", 0x83, "6", 9100, rseq(rng, 20), tags=("NH:i:2",)),
                 rec("q3", 0x183, "18", 400, rseq(rng, 20), tags=("NH:i:2",))]) +  # a second right record: read2_first is gone
        pair(rng, "q4", "18", 9000, "18", 400, nh1=None, nh2=None))                 # no NH at all
    add("right_mate_last_wins",
        "".join([rec("w1", 0x43, "6", 1100, "ACGTACGTAA", tags=("NH:i:1",)),
                 rec("w1", 0x143, "6", 7000, "TTTTTTTTTT", tags=("NH:i:1",)),       # a second left record: read 1 stays
                 rec("w1", 0x83, "6", 1150, "CCCCCCCCCA", tags=("NH:i:1",)),
                 rec("w1", 0x193, "6", 7100, "GGGGGGGGAT", tags=("NH:i:1",)),       # reverse, and the last right record
                 ]) + pair(rng, "w2", "6", 1100, "6", 1200))
    add("reverse_with_n",
        rec("n1", 0x53, "6", 1100, "ACGTNNacgtRYACGT", tags=("NH:i:1",)) + rec("n1", 0xa3, "6", 1200, "NNNNACGTTGCAAC", tags=("NH:i:1",)) +
        rec("n2", 0x63, "6", 1100, "A", tags=("NH:i:1",)) + rec("n2", 0x93, "6", 1200, "C", tags=("NH:i:1",)))
    add("two_families", pair(rng, "t1", "6", 1100, "18", 500) + pair(rng, "t2", "22", 101, "6", 5001) + pair(rng, "t3", "18", 301, "18", 899))
    add("overlap_break", pair(rng, "o1", "6", 1600, "6", 1700) + pair(rng, "o2", "6", 1900, "6", 2100) + pair(rng, "o3", "6", 2300, "6", 2450))
    add("half_open", pair(rng, "h1", "6", 1000, "6", 9000) + pair(rng, "h2", "6", 1001, "6", 9000) + pair(rng, "h3", "6", 2500, "6", 9000) +
        pair(rng, "h4", "6", 2501, "6", 9000) + pair(rng, "h5", "18", 900, "18", 901) + pair(rng, "h6", "18", 9000, "18", 300))
    add("unmapped_mates",
        rec("u1", 77, "*", 0, rseq(rng, 15), tags=("YT:Z:UP",)) + rec("u1", 141, "*", 0, rseq(rng, 15), tags=("YT:Z:UP",)) +
        rec("u2", 73, "6", 1100, rseq(rng, 15), tags=("NH:i:1",)) + rec("u2", 133, "6", 1100, rseq(rng, 15), tags=("YT:Z:UP",)) +
        rec("u3", 69, "6", 1100, rseq(rng, 15), tags=("YT:Z:UP",)) + rec("u3", 137, "6", 1100, rseq(rng, 15), tags=("NH:i:1",)) +
        rec("u4", 69, "6", 1100, rseq(rng, 15), tags=("NH:i:1",)) + rec("u4", 141, "*", 0, rseq(rng, 15)))
    add("name_again", pair(rng, "a1", "6", 1100, "6", 1200) + pair(rng, "a2", "6", 9000, "6", 9100) + pair(rng, "a1", "6", 1100, "6", 1200) +
        pair(rng, "a1x", "18", 400, "18", 500))
    add("unpaired", rec("s1", 0, "6", 1100, rseq(rng, 18), tags=("NH:i:1",)) + rec("s2", 16, "18", 400, rseq(rng, 18), tags=("NH:i:1",)) +
        rec("s2", 256, "6", 1100, rseq(rng, 18), tags=("NH:i:1",)) + rec("s3", 4, "*", 0, rseq(rng, 18)) +
        rec("s4", 0, "6", 1100, rseq(rng, 18), tags=("NH:i:2",)) + rec("s5", 16, "22", 200, rseq(rng, 18), tags=("NH:i:1",)),
        paired=False)
    add("fasta_out", pair(rng, "f1", "6", 1100, "6", 1200, f2=0x93) + pair(rng, "f2", "6", 9100, "6", 9200) + pair(rng, "f3", "22", 200, "22", 300),
        fastq=False)
    add("simulation_names",
        rec("0|L_6_1100", 0x43, "6", 1100, rseq(rng, 20), tags=("NH:i:1",)) + rec("0|R_6_1200", 0x83, "6", 1200, rseq(rng, 20), tags=("NH:i:1",)) +
        rec("1|L_x", 0x43, "6", 9000, rseq(rng, 20), tags=("NH:i:1",)) + rec("1|R_y", 0x83, "6", 9100, rseq(rng, 20), tags=("NH:i:1",)) +
        rec("10|L_x", 0x43, "18", 400, rseq(rng, 20), tags=("NH:i:1",)) + rec("10|R_z", 0x93, "18", 500, rseq(rng, 20), tags=("NH:i:1",)),
        simulation=True)
    add("database_filter", pair(rng, "d1", "6", 1100, "18", 500) + pair(rng, "d2", "18", 400, "18", 500) + pair(rng, "d3", "22", 200, "22", 300),
        database_list=["codis", "other"])
    add("database_append", pair(rng, "d1", "6", 1100, "18", 500) + pair(rng, "d3", "22", 200, "22", 300))

    def bt(name, flag, chrom, pos, AS, XS):
        tags = (["AS:i:%d" % AS] if AS is not None else []) + (["XS:i:%d" % XS] if XS is not None else []) + ["YT:Z:CP"]
        return rec(name, flag, chrom, pos, rseq(rng, 16), tags=tags)
    add("bowtie2_as_xs",
        bt("b1", 0x43, "6", 1100, -2, -10) + bt("b1", 0x83, "6", 9000, -2, -10) +          # AS > XS on the left record
        bt("b2", 0x43, "6", 1100, -5, -5) + bt("b2", 0x83, "6", 9000, 0, -9) +             # AS == XS: no hit; right outside
        bt("b3", 0x43, "6", 9000, -5, -5) + bt("b3", 0x83, "18", 400, -7, -1) +            # the right mate by read2_first
        bt("b4", 0x43, "6", 9000, 0, -1) + bt("b4", 0x143, "22", 200, 0, -9) + bt("b4", 0x83, "6", 9000, 0, 0) +   # read1_first is gone
        bt("b5", 77, "*", 0, None, None) + bt("b5", 141, "*", 0, None, None) +
        bt("b6", 0x43, "22", 9000, None, None) + bt("b6", 0x83, "22", 200, None, 3),         # neither AS nor XS: "" > "" is False
        aligner="bowtie2")
    ok = pair(rng, "e0", "6", 1100, "6", 1200)
    short = "\t".join(["e1", "67", "6", "1100", "60", "10M", "=", "0", "0", "ACGTACGTAC"]) + "\n"
    add("error_short_line", ok + short + pair(rng, "e2", "6", 1100, "6", 1200))
    add("error_no_mate_flag", ok + rec("e1", 0x1, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)) + pair(rng, "e2", "6", 1100, "6", 1200))
    add("error_names_differ", rec("e0", 0x43, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)) + rec("e1", 0x83, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)))
    add("error_no_read2", ok + rec("e1", 0x43, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)) + pair(rng, "e2", "6", 1100, "6", 1200))
    add("error_no_read1", ok + rec("e1", 0x83, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)) + pair(rng, "e2", "6", 1100, "6", 1200))
    add("error_bowtie2_no_xs", bt("e0", 0x43, "6", 1100, -2, -10) + bt("e0", 0x83, "6", 9000, -2, -10) +
        bt("e1", 0x43, "6", 1100, -2, None) + bt("e1", 0x83, "6", 1200, -2, -9), aligner="bowtie2")
    add("error_tag_value", ok + rec("e1", 0x43, "6", 1100, rseq(rng, 12), tags=("NH:i:x",)) + rec("e1", 0x83, "6", 1100, rseq(rng, 12), tags=("NH:i:1",)))
    add("omit_existing", pair(rng, "x1", "6", 1100, "18", 500), pre_existing=True)

    # the device route's case: a few thousand groups, most outside every region
    rng = random.Random(2024)
    chroms = ["1", "2", "6", "18", "22", "X"]
    parts = [HEADER]
    for g in range(1800):
        name = "r%05d" % g
        u = rng.random()
        if u < 0.12:
            c, p = rng.choice([("6", rng.randint(900, 2600)), ("6", rng.randint(4900, 6100)), ("18", rng.randint(250, 950)), ("22", rng.randint(50, 750))])
        else:
            c, p = rng.choice(chroms), rng.randint(7000, 90000)
        c2, p2 = (c, p + rng.randint(20, 300)) if rng.random() < 0.9 else (rng.choice(chroms), rng.randint(1, 9000))
        nh1, nh2 = rng.choice([1, 1, 1, 2, 5]), rng.choice([1, 1, 1, 2])
        f1 = 0x43 | (0x10 if rng.random() < 0.5 else 0)
        f2 = 0x83 | (0x10 if rng.random() < 0.5 else 0)
        n = rng.randint(12, 28)
        q = "I" * n
        if rng.random() < 0.05:
            parts.append(rec(name, 77, "*", 0, rseq(rng, n, "ACGTN"), q, ("YT:Z:UP",)) + rec(name, 141, "*", 0, rseq(rng, n), q, ("YT:Z:UP",)))
            continue
        parts.append(rec(name, f1, c, p, rseq(rng, n, "ACGTN" if rng.random() < 0.1 else "ACGT"), q, ("AS:i:0", "NH:i:%d" % nh1)))
        if nh1 > 1 and rng.random() < 0.5:
            parts.append(rec(name, f1 | 0x100, rng.choice(chroms), rng.randint(1, 9000), rseq(rng, n), q, ("AS:i:-6", "NH:i:%d" % nh1)))
        parts.append(rec(name, f2, c2, p2, rseq(rng, n), q, ("AS:i:0", "NH:i:%d" % nh2)))
        if nh2 > 1 and rng.random() < 0.5:
            parts.append(rec(name, f2 | 0x100, rng.choice(chroms), rng.randint(1, 9000), rseq(rng, n), q, ("AS:i:-6", "NH:i:%d" % nh2)))
    add("big_random", "".join(parts))
    return S


def make_stubs(tmp):
    bindir = os.path.join(tmp, "bin")
    for name in ("hisat2", "bowtie2"):
        p = os.path.join(bindir, name)
        with open(p, "w") as f:
            f.write("#!/bin/sh\ncat \"$HGX_STUB_SAM\"\n")
        os.chmod(p, os.stat(p).st_mode | stat.S_IEXEC)


def make_index(ix_dir, base, locus_text):
    os.makedirs(ix_dir, exist_ok=True)
    full = os.path.join(ix_dir, base)
    for e in ("fa", "snp", "haplotype", "link", "coord", "clnsig"):
        open("%s.%s" % (full, e), "w").close()
    for i in range(8):
        open("%s.%d.ht2" % (full, i + 1), "w").close()
    for i in range(4):
        open("%s.%d.bt2" % (full, i + 1), "w").close()
    for i in range(2):
        open("%s.rev.%d.bt2" % (full, i + 1), "w").close()
    with open(full + ".locus", "w") as f:
        f.write(locus_text)


def wait_for_gzip(out_dir):
    """The reference leaves its gzip children running: wait until every output is a complete .gz of stable size."""
    last = None
    for _ in range(600):
        names = sorted(os.listdir(out_dir))
        sizes = [os.path.getsize(os.path.join(out_dir, n)) for n in names]
        ok = all(subprocess.call(["gzip", "-t", os.path.join(out_dir, n)], stderr=subprocess.DEVNULL) == 0 for n in names)
        if ok and sizes == last:
            return names
        last = sizes
        time.sleep(0.1)
    raise RuntimeError("gzip children did not finish in %s" % out_dir)


def record(name, sc, tmp, process):
    a = sc["args"]
    work = os.path.join(tmp, "run_" + name)
    ix_dir, out_dir, read_dir = os.path.join(work, "ix"), os.path.join(work, "out"), os.path.join(work, "reads")
    os.makedirs(read_dir)
    os.makedirs(out_dir)
    make_index(ix_dir, "genotype_genome", LOCUS)
    sam_path = os.path.join(work, "stub.sam")
    with open(sam_path, "w") as f:
        f.write(sc["sam"])
    os.environ["HGX_STUB_SAM"] = sam_path
    ext = "fq" if a["fastq"] else "fa"
    if a["paired"]:
        read_fname = [os.path.join(read_dir, "sample_1." + ext), os.path.join(read_dir, "sample_2." + ext)]
        base = "sample_1." + ext
    else:
        read_fname = [os.path.join(read_dir, "sample." + ext)]
        base = "sample"
    for p in read_fname:
        open(p, "w").close()
    dbl = list(a["database_list"])
    pre = {}
    if a.get("pre_existing"):
        for fam in ("hla", "codis", "cyp"):
            for m in (1, 2):
                fn = "%s-%s-extracted-%d.fq.gz" % (base, fam, m)
                pre[fn] = "@kept\nAC\n+\nII\n"
                with gzip.open(os.path.join(out_dir, fn), "wt") as f:
                    f.write(pre[fn])
    exc, fname_list = None, None
    try:
        fname_list = process.extract_reads("genotype_genome", ix_dir, dbl, read_dir, out_dir, ext, read_fname, a["fastq"], a["paired"],
                                           a["simulation"], 1, 1, sys.maxsize, [0, 1], a["aligner"], 0, False)
    except BaseException as e:      # SystemExit included
        exc = type(e).__name__
        del e
    gc.collect()                    # an exception leaves the gzip pipes open in the dead frame: Popen.__del__ parks a running child
    for child in list(getattr(subprocess, "_active", None) or []):      # in subprocess._active with its pipes; the interpreter's exit
        if child.stdin and not child.stdin.closed:                     # would flush and close them, as is done here
            child.stdin.close()
    names = wait_for_gzip(out_dir)
    files = {}
    for n in names:
        with gzip.open(os.path.join(out_dir, n), "rt") as f:
            files[n] = f.read()
    args = {k: v for k, v in a.items() if k != "pre_existing"}
    fx = dict(name=name, sam=sc["sam"], locus=LOCUS, base=base, args=args, files=files, fname_list=fname_list,
              database_list_after=dbl, exception=exc, pre_existing=pre)
    with gzip.GzipFile(os.path.join(HERE, "extract_%s.json.gz" % name), "wb", mtime=0) as f:
        f.write(json.dumps(fx, sort_keys=True).encode())
    print("%-24s exception=%-16s files=%s" % (name, exc, {n: len(t) for n, t in files.items()}))


def main():
    tmp = make_golden.setup_reference()
    make_stubs(tmp)
    import hisatgenotype_typing_process as process
    S = scenarios()
    try:
        for name in (sys.argv[1:] or sorted(S)):
            record(name, S[name], tmp, process)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
