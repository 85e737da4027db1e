"""The spec of read extraction (typing_process.py:1630-1745) as plain Python, in the manner of tests/linear_ref.py: what the
library's host and device routes have to give, and what the fixtures recorded from the real reference pin."""
import gzip
import json
import os

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
EXC = {"ValueError": ValueError, "AssertionError": AssertionError, "SystemExit": SystemExit, "IndexError": IndexError,
       "TypeError": TypeError, "NotImplementedError": NotImplementedError}


def fixture_names():
    return sorted(f[len("extract_"):-len(".json.gz")] for f in os.listdir(GOLDEN_DIR)
                  if f.startswith("extract_") and f.endswith(".json.gz"))


def load(name):
    with gzip.open(os.path.join(GOLDEN_DIR, "extract_%s.json.gz" % name), "rb") as f:
        return json.loads(f.read().decode())


def region_table(locus_text, database_list):
    """[(family lower, chromosome, left, right)] in file order; database_list is extended in place."""
    filtered = len(database_list) > 0
    out, seen = [], set()
    for line in locus_text.splitlines():
        family, allele_name, chrom, left, right = line.strip().split()[:5]
        if filtered and family.lower() not in database_list:
            continue
        key = "%s-%s" % (family, allele_name.split('*')[0])
        assert key not in seen
        seen.add(key)
        out.append((family.lower(), chrom, int(left), int(right)))
        if family.lower() not in database_list:
            database_list.append(family.lower())
    return out


def revcomp(seq):
    return "".join(COMP.get(c, c) for c in reversed(seq))


def extract(sam_text, regions, families, aligner, paired, simulation, fastq):
    """-> ({(family, mate): text}, exception class or None).  The text holds what was written before the exception."""
    out = {(f, m): [] for f in families for m in range(2 if paired else 1)}
    by_chrom = {}
    for fam, chrom, left, right in regions:
        by_chrom.setdefault(chrom, []).append((fam, left, right))

    def key(name):
        return name.split('|')[0] if simulation else name

    def write(fams, name, read1, read2):
        for fam in fams:
            for m, read in enumerate([read1, read2] if paired else [read1]):
                seq, qual = read[0], read[1]                       # IndexError on an empty list, as the reference
                out[(fam, m)].append(("@%s\n%s\n+\n%s\n" % (name, seq, qual)) if fastq else (">%s\n%s\n" % (name, seq)))

    state = {"prev": "", "fams": [], "r1": [], "r2": [], "r1f": True, "r2f": True, "chk": True}

    def run():
        st = state
        for line in sam_text.split("\n")[:-1] if sam_text.endswith("\n") else sam_text.split("\n"):
            if line.startswith('@'):
                continue
            cols = line.strip().split()
            name, flag, chrom, pos, _, _, _, _, _, seq, qual = cols[:11]
            flag, pos = int(flag), int(pos) - 1
            tag = {"AS": "", "XS": "", "NH": ""}
            for col in cols[11:]:
                if col[:2] in tag:
                    tag[col[:2]] = int(col[5:])
            if st["chk"] and st["prev"] != "":
                st["chk"] = False
                if name != st["prev"] and not simulation and paired:
                    raise SystemExit(1)
            if key(name) != key(st["prev"]):
                write(st["fams"], st["prev"], st["r1"], st["r2"])
                st.update(prev=name, fams=[], r1=[], r2=[], r1f=True, r2f=True)
            left_rec = bool(flag & 0x40) or not paired
            if flag & 0x4 == 0:
                hit = aligner == "hisat2" and tag["NH"] == 1
                if not hit:
                    if left_rec:
                        hit = aligner == "bowtie2" and tag["AS"] > tag["XS"] and st["r1f"]     # TypeError: "" against an int
                    else:
                        hit = st["r2f"]
                if hit:
                    for fam, left, right in by_chrom.get(chrom, []):
                        if left <= pos < right:
                            if fam not in st["fams"]:
                                st["fams"].append(fam)
                            break
            read = [revcomp(seq), qual[::-1]] if flag & 0x10 else [seq, qual]
            if left_rec:
                st["r1f"] = False
                if not st["r1"]:
                    st["r1"] = read
            else:
                assert flag & 0x80
                st["r2f"] = False
                st["r2"] = read
        write(st["fams"], st["prev"], st["r1"], st["r2"])

    exc = None
    try:
        run()
    except (ValueError, AssertionError, SystemExit, IndexError, TypeError) as e:
        exc = type(e)
    return {k: "".join(v) for k, v in out.items()}, exc


def file_name(base, family, mate, paired):
    return "%s-%s-extracted-%d.fq.gz" % (base, family, mate + 1) if paired else "%s-%s-extracted.fq.gz" % (base, family)


def expected_files(fx):
    """{file name: text} the spec gives for a fixture's recorded input, and the exception class."""
    a = fx["args"]
    dbl = list(a["database_list"])
    regions = region_table(fx["locus"], dbl)
    texts, exc = extract(fx["sam"], regions, dbl, a["aligner"], a["paired"], a["simulation"], a["fastq"])
    return {file_name(fx["base"], f, m, a["paired"]): t for (f, m), t in texts.items()}, exc, dbl
