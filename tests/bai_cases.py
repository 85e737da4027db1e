"""Fixtures of the BAM-index tests (test_bai_ref.py, test_bam_index.py, test_gpu_bam_index.py): a genotype-genome sample as
test_gpu_region_lists.py makes it -- the reads of a synthetic HLA-like locus on chromosome coordinates -- placed ACROSS a 16 kb window
boundary of chromosome "6", with decoy records before, inside the gaps around and after the locus and on a second reference, a
reference without records, and one spliced record whose N operation spans three windows.  Sorted by coordinate and written with
bamio.write_bam at block sizes of 300, 700 and 0xff00 bytes: records straddle blocks, chunks begin at offset 0 of a block and inside one."""
import functools
import os
import random

from hisatgenotype_amd import bamio, locus as hl, synth

W = 1 << 14                                  # the linear index's window
LEFT = W - 1500                              # the locus' first base on chromosome 6 (0-based): the backbone crosses position W
REFS = [("6", 200000), ("7", 50000), ("8", 1000)]
BLOCK_SIZES = (300, 700, 0xff00)
SPLICED_AT = 5 * W - 100                     # the spliced record: 50M, 40 000 N, 50M -- windows 4 .. 7


@functools.lru_cache(maxsize=None)
def the_locus():
    return synth.make_hla_like_locus(gene="A", n_alleles=600, length=3569, n_vars=1300, seed=300, var_id_base=0)


@functools.lru_cache(maxsize=None)
def packed():
    return hl.PackedLocus.from_synth(the_locus())


def locus_span():
    return LEFT, LEFT + len(the_locus().backbone) - 1          # 0-based, inclusive


def _decoy(name, ref, pos1, cigar="50M", flag=0, n=50):
    rng = random.Random(name)                # (bases that do not deflate to nothing: the decoys are most of the file, as in a genome BAM)
    return "\t".join([name, str(flag), ref, str(pos1), "60", cigar, "*", "0", "0", "".join(rng.choice("ACGT") for _ in range(n)),
                      "".join(chr(33 + rng.randrange(40)) for _ in range(n)), "NM:i:0", "MD:Z:%d" % n, "NH:i:1"])


@functools.lru_cache(maxsize=None)
def sam_lines(n_pairs=600):
    """The sample's records, sorted by (reference, position)."""
    loc = the_locus()
    sam = synth.simulate_sam_fast(loc, synth.pick_sample(loc, 40), n_pairs, err_rate=0.003, seed=50)
    rows = []
    for l in sam.split("\n"):
        if l:
            f = l.split("\t")
            f[0], f[2], f[3], f[7] = "A_" + f[0], "6", str(int(f[3]) + LEFT), str(int(f[7]) + LEFT)
            rows.append("\t".join(f))
    right = locus_span()[1]
    for k in range(150):
        rows.append(_decoy("before%03d" % k, "6", 1 + 90 * k))                         # 1 .. 13 411: in front of the locus
    for k in range(150):
        rows.append(_decoy("after%03d" % k, "6", right + 400 + 150 * k))               # behind it, into the third window
    for k in range(60):
        rows.append(_decoy("far%03d" % k, "6", 150000 + 37 * k))
    rows.append(_decoy("spliced", "6", SPLICED_AT + 1, "50M40000N50M", n=100))
    rows.append(_decoy("unmapped_placed", "6", 9 * W + 5, "*", flag=4))
    for k in range(2400):
        rows.append(_decoy("other%04d" % k, "7", 1 + 20 * k))
    for k in range(3):
        rows.append(_decoy("unplaced%d" % k, "*", 0, "*", flag=4))
    order = {n: i for i, (n, _) in enumerate(REFS)}
    return tuple(sorted(rows, key=lambda l: (order.get(l.split("\t")[2], len(REFS)), int(l.split("\t")[3]))))


def write_fixture(directory, block_size, lines=None, name=None, refs=None):
    """`refs`: the header's references in another order (the records are sorted to it)."""
    path = os.path.join(str(directory), name or "wgs_%d.bam" % block_size)
    lines = lines or sam_lines()
    if refs is not None:
        order = {n: i for i, (n, _) in enumerate(refs)}
        lines = sorted(lines, key=lambda l: (order.get(l.split("\t")[2], len(refs)), int(l.split("\t")[3])))
    bamio.write_bam(path, "\n".join(lines) + "\n", refs or REFS, block_size=block_size)
    return path


def locus_regions():
    left, right = locus_span()
    return ["6:%d-%d" % (left + 1, right + 1), "A*BACKBONE"]                           # what genotype-genome mode asks for


def region_grid():
    """name -> region list (samtools strings): both sides of a 16 kb window boundary, empty and unknown places, whole references, lists
    whose chunks share a block or overlap, more regions than the device route takes, a record found through a parent bin."""
    left, right = locus_span()
    g = {}
    for d in (-1, 0, 1):
        g["left edge %+d" % d] = ["6:%d-%d" % (W + d + 1, W + d + 600)]               # left0 = W + d
        g["right edge %+d" % d] = ["6:%d-%d" % (W - 700, W + d + 1)]                   # right0 = W + d
    g["nothing there"] = ["6:130001-130100"]
    g["beyond the end"] = ["6:300001-300100"]
    g["whole 6"] = ["6"]
    g["whole 7"] = ["7"]
    g["no records"] = ["8"]
    g["unknown"] = ["nope"]
    g["open end"] = ["6:%d" % 150500]
    g["open start"] = ["6:-200"]
    g["two, one block"] = ["6:%d-%d" % (left + 100, left + 150), "6:%d-%d" % (left + 160, left + 200)]
    g["two, overlapping"] = ["6:%d-%d" % (left + 1, left + 2000), "6:%d-%d" % (left + 1000, right + 1)]
    g["nine"] = ["6:%d-%d" % (left + 1 + 300 * k, left + 250 + 300 * k) for k in range(8)] + ["7:1-3000"]
    g["spliced, from a later window"] = ["6:%d-%d" % (7 * W + 10, 7 * W + 20)]
    g["unmapped but placed"] = ["6:%d-%d" % (9 * W + 1, 9 * W + 10)]
    g["locus"] = locus_regions()
    return g
