"""The routing of an alignment set, stated in plain Python: for a list of BAM files and one samtools region string per locus slot,
the records every (slot, file) keeps, in file order.  A record belongs to a slot when `samtools view file region` prints it
(typing_core.py:436-444): its reference is the region's whole name, or the region's `name` with the record's span
[pos0, end0] overlapping [left0, right0]; the span comes from the CIGAR (M D N = X), one base for an unmapped record or an empty
CIGAR.  An empty region string filters nothing.  A region is read against every file's own header, so files may list their
references in any order.  Built on bamio.read_bam / bamio.region_hit; tests/test_gpu_alignment_set.py holds the device routing
(engine.AlignmentSet.route) to it."""
from hisatgenotype_amd import bamio


def record_span(line):
    """(rname, pos0, end0) of one SAM line as the region test sees it."""
    f = line.split("\t")
    flag, rname, pos0, cigar = int(f[1]), f[2], int(f[3]) - 1, f[5]
    reflen = 0 if (flag & 4) or cigar == "*" else bamio.cigar_reflen(cigar)
    return rname, pos0, pos0 + max(reflen, 1) - 1


def keeps(region, line):
    """Does the slot with samtools region string `region` keep this record?"""
    if not region:
        return True
    rname, pos0, end0 = record_span(line)
    if rname == "*":                                   # no reference (refID -1): no region holds it
        return False
    return bamio.region_hit(bamio.parse_region(region), rname, pos0, end0)


def route(paths, regions):
    """[slot][file] -> the kept records (SAM lines) in file order."""
    files = [bamio.read_bam(str(p)) for p in paths]
    return [[[l for l in lines if keeps(region, l)] for lines in files] for region in regions]


def kept_counts(paths, regions):
    """[slot][file] -> number of kept records: what engine.AlignmentSet.kept reports."""
    return [[len(v) for v in row] for row in route(paths, regions)]
