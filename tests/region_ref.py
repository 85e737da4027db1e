"""A samtools region LIST, stated in plain Python: "region after region, duplicates kept".

`samtools view F r1 r2 ...` (typing_core.py:436-444 names two regions in genotype-genome mode: `chr:left-right` and the gene's
backbone) prints, for every region in the order given, the records that overlap it, in file order; a record that overlaps several
regions comes out once per region.  The reference pipes that through `sort -k1,1 -s`: a STABLE sort by read name over that list.

Per region the rule is the one of one region:
  * the region string read as a whole reference name keeps every record on that reference, and that reading stands beside its
    `name:left-right` reading (1-based, inclusive; `name:left`, `name:-right`; commas may group digits);
  * a record spans [pos0, end0]: the reference bases its CIGAR consumes (M D N = X), ONE base for an unmapped record (flag 0x4) or
    an empty CIGAR;
  * a record without a reference (RNAME `*`, refID -1) belongs to no region;
  * names are compared with the file's own header: a region naming a reference the file does not have keeps nothing.
Works over SAM record lines (str).  bamio.read_bam, the native host reader and the device front end's kernels are held to this
(tests/test_region_ref.py, tests/test_gpu_region_lists.py)."""
import re

_SPAN = re.compile(r"^([0-9,]*)(?:(-)([0-9,]*))?$")
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
OPEN_END = 1 << 62


def parse(region):
    """-> (whole, name or None, left0, right0)."""
    whole, name, left0, right0 = region, None, 0, OPEN_END
    cut = region.rfind(":")
    if cut > 0:
        m = _SPAN.match(region[cut + 1:])
        if m:
            lo, hi = m.group(1).replace(",", ""), (m.group(3) or "").replace(",", "")
            lo_ok = (lo != "") == (m.group(1) != "")             # (commas alone are no number)
            hi_ok = (hi != "") == ((m.group(3) or "") != "")
            if (lo or hi) and lo_ok and hi_ok:
                name = region[:cut]
                left0 = max(int(lo) - 1, 0) if lo else 0
                right0 = int(hi) - 1 if hi else OPEN_END
    return whole, name, left0, right0


def as_list(regions):
    """A list of strings, or one string with newlines -> list of non-empty strings; None / "" -> None (nothing is filtered)."""
    if regions is None or regions == "":
        return None
    if isinstance(regions, str):
        regions = regions.split("\n")
    return [r for r in regions if r]


def span(line):
    """(rname, pos0, end0) of a SAM record line."""
    f = line.split("\t")
    flag, rname, pos0, cigar = int(f[1]), f[2], int(f[3]) - 1, f[5]
    reflen = 0
    if not (flag & 4) and cigar != "*":
        reflen = sum(int(n) for n, op in _CIGAR.findall(cigar) if op in "MDN=X")
    return rname, pos0, pos0 + max(reflen, 1) - 1


def hit(region, line):
    rname, pos0, end0 = span(line)
    if rname == "*":
        return False
    whole, name, left0, right0 = parse(region)
    if rname == whole:
        return True
    return name is not None and rname == name and end0 >= left0 and pos0 <= right0


def mask(lines, regions):
    """Per record the list of region indices that keep it."""
    regs = as_list(regions)
    return [[g for g, r in enumerate(regs) if hit(r, l)] for l in lines]


def kept(lines, regions):
    """The records `samtools view F regions...` prints, in its order: region after region, file order inside, duplicates kept."""
    regs = as_list(regions)
    if regs is None:
        return list(lines)
    return [l for r in regs for l in lines if hit(r, l)]


def kept_counts(lines, regions):
    """Records per region."""
    regs = as_list(regions)
    return [sum(1 for l in lines if hit(r, l)) for r in regs]


def name_sorted(lines):
    """`sort -k1,1 -s` under LC_ALL=C: stable, bytewise by the first field."""
    return sorted(lines, key=lambda l: l.split("\t", 1)[0].encode())
