#!/usr/bin/env python3
"""Golden vectors of the reference's LINEAR-index typing (typing_core.py:1597-1677, 1791-1797), recorded from the REAL
reference in the build container (make_golden.setup_reference: a scratch copy plus a stub ``samtools`` whose ``view`` prints
the SAM body in file order and ignores a region -- what the linear branch reads).  The *_region fixtures therefore pin the
genotype-genome call path (genotype_genome != "") and not a region filter: the stub hands every record over.

Per fixture (``tests/golden/linear_<name>.json.gz``, data only):
  sam          the record stream
  options      gene, base_fname, aligners, genotype_genome
  sections     per aligner: Gene_counts and Gene_cmpt in dict order (captured off add_alleles' closure cells)
  em           every single_abundance call: its class dict, flags, result at repr precision, outer iterations
  report       the report text from the first aligner section on
  error        the exception typing() raised, if any
Run:  PYTHONHASHSEED=0 python tests/golden/make_linear_golden.py [scenario ...]
"""
import gzip
import json
import os
import random
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (re-execs under PYTHONHASHSEED=0 and sets up the import path)
from hisatgenotype_amd import synth  # noqa: E402


def line(qname, flag, rname, AS, extra=(), pos=1):
    cols = [qname, str(flag), rname, str(pos), "60", "20M", "*", "0", "0", "ACGTACGTACGTACGTACGT", "I" * 20]
    cols += list(extra)
    if AS is not None:
        cols.append("AS:i:%d" % AS)
    cols.append("NM:i:0")
    return "\t".join(cols)


def hla_locus():
    return synth.make_hla_like_locus(n_alleles=40, n_vars=60, seed=11)


def codis_locus():
    return synth.make_str_like_locus(seed=3)


def alleles_of(loc):
    return [a for a in loc.allele_names if "BACKBONE" not in a]


SCENARIOS = {}


def scenario(fn):
    SCENARIOS[fn.__name__] = fn
    return fn


def mixed_lines(loc, rng, n_groups, interleave=True, max_k=6, with_noise=True):
    al = alleles_of(loc)
    out = []
    for g in range(n_groups):
        k = rng.randint(1, max_k)
        base = rng.randint(-30, 0)
        for j in range(k):
            AS = base + rng.choice([0, 0, -2, 2, -5])
            flag = rng.choice([0, 256, 16, 272, 2048]) if j else rng.choice([0, 16])
            out.append(line("r%d" % g, flag, rng.choice(al), AS))
        if with_noise and rng.random() < 0.2:
            out.append(line("r%d" % g, 4, "*", None))
        if with_noise and rng.random() < 0.1:
            out.append(line("r%d" % g, 0, loc.ref_allele, -1))
        if with_noise and rng.random() < 0.1:
            out.append(line("r%d" % g, 0, "ZZ*01:01", -1))
    if interleave:                        # the same read ids again, after others: new groups in the reference's loop
        for g in range(0, n_groups, 3):
            out.append(line("r%d" % g, 256, rng.choice(al), rng.randint(-10, 0)))
    return out


@scenario
def hla_mixed():
    loc = hla_locus()
    rng = random.Random(1)
    return dict(locus=loc, lines=mixed_lines(loc, rng, 60), aligners=[["hisat2", "linear"]])


@scenario
def codis_mixed():
    loc = codis_locus()
    rng = random.Random(2)
    return dict(locus=loc, lines=mixed_lines(loc, rng, 80), aligners=[["hisat2", "linear"]])


@scenario
def codis_as_order():
    """AS rising, falling and equal inside groups; secondary records kept."""
    loc = codis_locus()
    al = alleles_of(loc)
    L = [line("a", 0, al[0], 5), line("a", 256, al[1], 10), line("a", 256, al[2], 10), line("a", 256, al[3], 7),
         line("b", 0, al[4], 10), line("b", 256, al[5], 10), line("b", 2048, al[6], 3),
         line("c", 16, al[1], -4), line("c", 272, al[2], -6), line("c", 272, al[0], -4),
         line("d", 0, al[3], 0, extra=["AS:i:99"]), line("d", 256, al[2], 1),
         line("e", 0, al[1], -1), line("e", 256, al[1], -1)]
    return dict(locus=loc, lines=L, aligners=[["hisat2", "linear"]])


def bowtie_lines(loc, last_big):
    al = alleles_of(loc)
    L = [line("x", 0, al[i], 0) for i in range(12)]              # 12 names mid-file: not counted by bowtie2
    L += [line("y", 0, al[i], 0) for i in range(3)]
    L += [line("z", 0, al[i], 0) for i in range(9)]              # 9 names: counted
    L += [line("w", 0, al[i], 0) for i in range(10)]             # exactly 10: not counted
    L += [line("v", 0, al[i], 0) for i in range(2)]
    if last_big:
        L += [line("u", 0, al[i], 0) for i in range(11)]         # the last group is always counted
    return L


@scenario
def codis_bowtie2_mid():
    loc = codis_locus()
    return dict(locus=loc, lines=bowtie_lines(loc, False), aligners=[["bowtie2", "linear"]])


@scenario
def codis_bowtie2_last():
    loc = codis_locus()
    return dict(locus=loc, lines=bowtie_lines(loc, True), aligners=[["bowtie2", "linear"]])


@scenario
def codis_two_aligners():
    loc = codis_locus()
    return dict(locus=loc, lines=bowtie_lines(loc, True), aligners=[["hisat2", "linear"], ["bowtie2", "linear"]])


@scenario
def codis_other_aligner():
    loc = codis_locus()
    return dict(locus=loc, lines=bowtie_lines(loc, False), aligners=[["bwa", "linear"]])


def last_line_case(loc, tail):
    al = alleles_of(loc)
    L = [line("p", 0, al[0], 0), line("p", 256, al[1], 0), line("q", 0, al[2], 0), line("q", 256, al[0], -3),
         line("s", 0, al[1], 0), line("s", 256, al[2], 0)]
    return L + tail


@scenario
def codis_last_unmapped():
    loc = codis_locus()
    return dict(locus=loc, lines=last_line_case(loc, [line("t", 4, "*", None)]), aligners=[["hisat2", "linear"]])


@scenario
def codis_last_other_gene():
    loc = codis_locus()
    return dict(locus=loc, lines=last_line_case(loc, [line("t", 0, "TPOX*7", -2)]), aligners=[["hisat2", "linear"]])


@scenario
def codis_last_backbone():
    loc = codis_locus()
    return dict(locus=loc, lines=last_line_case(loc, [line("t", 0, loc.ref_allele, -2)]), aligners=[["hisat2", "linear"]])


@scenario
def hla_last_backbone():
    loc = hla_locus()
    return dict(locus=loc, lines=last_line_case(loc, [line("t", 0, loc.ref_allele, -2)]), aligners=[["hisat2", "linear"]])


@scenario
def codis_one_class():
    loc = codis_locus()
    al = alleles_of(loc)
    L = [line("a", 0, al[0], 0), line("a", 256, al[1], 0), line("b", 0, al[1], 0), line("b", 256, al[0], 0)]
    return dict(locus=loc, lines=L, aligners=[["hisat2", "linear"]])


@scenario
def codis_zero_classes():
    loc = codis_locus()
    L = [line("a", 4, "*", None), line("b", 0, loc.ref_allele, 0), line("c", 0, "TPOX*7", 0)]
    return dict(locus=loc, lines=L, aligners=[["hisat2", "linear"]])


@scenario
def hla_region():
    loc = hla_locus()
    rng = random.Random(7)
    return dict(locus=loc, lines=mixed_lines(loc, rng, 30), aligners=[["hisat2", "linear"]], genotype_genome="genotype_genome")


@scenario
def codis_region():
    loc = codis_locus()
    rng = random.Random(8)
    return dict(locus=loc, lines=mixed_lines(loc, rng, 30), aligners=[["hisat2", "linear"]], genotype_genome="genotype_genome")


@scenario
def codis_coordinate_sorted():
    """What align_reads writes: a coordinate-sorted BAM -- the records of one read rarely sit next to each other."""
    loc = codis_locus()
    rng = random.Random(9)
    L = mixed_lines(loc, rng, 120, interleave=False, with_noise=False)
    rng.shuffle(L)
    return dict(locus=loc, lines=L, aligners=[["hisat2", "linear"]])


class Recorder:
    def __init__(self, common):
        self.common = common
        self.sections = []          # [(Gene_counts, Gene_cmpt)] dict objects, one per add_alleles closure seen
        self.em = []
        self._seen = set()

    def profile(self, frame, event, arg):
        if event == "return" and frame.f_code.co_name == "add_alleles":
            gc, gm = frame.f_locals["Gene_counts"], frame.f_locals["Gene_cmpt"]
            if id(gc) not in self._seen:
                self._seen.add(id(gc))
                self.sections.append((gc, gm))

    def install(self):
        c = self.common
        self._orig = (c.single_abundance, c.prob_diff)
        orig_sa, orig_pd = self._orig
        rec = self

        def pd(a, b):
            rec._iters += 1
            return orig_pd(a, b)

        def sa(Gene_cmpt, remove_low_abundance_allele=False, Gene_length={}):
            call = {"cmpt": list(Gene_cmpt.items()), "remove_low": bool(remove_low_abundance_allele),
                    "use_length": len(Gene_length) > 0}
            rec._iters = 0
            res = orig_sa(Gene_cmpt, remove_low_abundance_allele, Gene_length)
            call["result"] = [[a, repr(float(p))] for a, p in res]
            call["n_iter"] = rec._iters
            rec.em.append(call)
            return res
        c.single_abundance, c.prob_diff = sa, pd

    def restore(self):
        self.common.single_abundance, self.common.prob_diff = self._orig


def run_reference(core, common, loc, sam, aligners, genotype_genome, workdir):
    d = loc.reference_dicts()
    os.makedirs(workdir, exist_ok=True)
    cwd = os.getcwd()
    os.chdir(workdir)
    bam = os.path.join(workdir, "lin.bam")
    with open(bam, "w") as f:
        f.write(sam)
    rec = Recorder(common)
    rec.install()
    err = None
    stderr_fd = os.dup(2)
    devnull = os.open(os.devnull, os.O_WRONLY)
    try:
        os.dup2(devnull, 2)
        sys.setprofile(rec.profile)
        try:
            core.typing(False, os.path.join(workdir, loc.base_fname), [loc.gene], genotype_genome, True, set(), d["refGenes"],
                        d["Genes"], d["Gene_names"], d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"],
                        aligners, 2, False, "assembly_graph", True, True, False, False, True, [], False,
                        ["reads_1.fa", "reads_2.fa"], bam, [], 150, 400, 1, False, 0, False, workdir, "NONE", False, 0)
        except Exception as e:
            err = "%s: %s" % (type(e).__name__, e)
        finally:
            sys.setprofile(None)
    finally:
        os.dup2(stderr_fd, 2)
        os.close(devnull)
        os.close(stderr_fd)
        rec.restore()
        os.chdir(cwd)
    rep = [f for f in os.listdir(workdir) if f.endswith(".report")]
    report = open(os.path.join(workdir, rep[0])).read() if rep else ""
    body = report.split("\n")
    k = next((i for i, l in enumerate(body) if l.startswith("\t\t") and l.strip().endswith("linear")), None)
    if k is not None:
        report = "\n".join(body[k - 1:])          # from the blank line the section header opens with
    return rec, report, err


def main():
    names = sys.argv[1:] or list(SCENARIOS)
    tmp = mg.setup_reference()
    import hisatgenotype_typing_common as common
    import hisatgenotype_typing_core as core
    try:
        for name in names:
            sc = SCENARIOS[name]()
            loc = sc["locus"]
            sam = "".join(l + "\n" for l in sc["lines"])
            gg = sc.get("genotype_genome", "")
            rec, report, err = run_reference(core, common, loc, sam, sc["aligners"], gg, os.path.join(tmp, "work_" + name))
            fx = {
                "name": "linear_" + name,
                "options": {"gene": loc.gene, "base_fname": loc.base_fname, "aligners": sc["aligners"], "genotype_genome": gg},
                "locus": loc.to_json(),
                "sam": sam,
                "sections": [{"counts": list(gc.items()), "classes": list(gm.items())} for gc, gm in rec.sections],
                "em": rec.em,
                "report": report,
                "error": err,
            }
            out = os.path.join(HERE, "linear_%s.json.gz" % name)
            with gzip.GzipFile(out, "wb", mtime=0) as f:
                f.write(json.dumps(fx, separators=(",", ":")).encode())
            print("%-24s lines=%d sections=%d classes=%s em=%d err=%s size=%.1f KB" % (
                name, len(sc["lines"]), len(rec.sections), [len(gm) for _, gm in rec.sections], len(rec.em), err,
                os.path.getsize(out) / 1024.0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
