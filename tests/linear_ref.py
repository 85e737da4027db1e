"""Plain-Python statement of the reference's linear-index typing (typing_core.py:1597-1677, 1791-1797): the test oracle of
the linear route (hgx_type_linear_* / typing.type_locus_linear).

Input: the record stream ``samtools view <file> [region]`` prints, in FILE order (no name sort, no ref_allele filter).
Rules, as the reference's loop applies them:
  * a record is skipped iff ``flag & 0x4``, its RNAME does not start with the gene, or RNAME contains ``BACKBONE``;
  * AS = int(col[5:]) of the LAST column among cols[11:] starting with ``AS`` (none: AssertionError);
  * a group is a run of consecutive kept records with one read id (the same id later again starts a new group);
  * a record joins the class iff its AS >= the max AS of the group's records before it (segmented exclusive prefix max);
  * a group is flushed when the next group's first kept record arrives, and counted iff aligner == "hisat2" or
    (aligner == "bowtie2" and it holds < 10 names); the last group is always counted;
  * a counted group adds 1 to Gene_counts[allele], where `allele` is the free variable of the loop: the RNAME of the next
    group's first kept record, or for the final flush the RNAME of the last line read; and 1 to Gene_cmpt['-'.join(sorted)].
"""
import pyref


def records(sam_text):
    """The lines of the stream (bytes or str) as the loop sees them."""
    if isinstance(sam_text, bytes):
        sam_text = sam_text.decode()
    return [l for l in sam_text.split("\n") if l != ""]


def gene_counts_and_classes(lines, gene, aligner):
    """(Gene_counts dict, Gene_cmpt dict) in insertion order; raises what the reference raises."""
    Gene_counts, Gene_cmpt = {}, {}
    allele = None

    def add_alleles(alleles):
        Gene_counts[allele] = Gene_counts.get(allele, 0) + 1
        key = "-".join(sorted(alleles))
        Gene_cmpt[key] = Gene_cmpt.get(key, 0) + 1

    prev_read_id = prev_AS = None
    alleles = set()
    for line in lines:
        cols = line.split()
        read_id, flag, allele = cols[:3]
        flag = int(flag)
        if flag & 0x4 != 0:
            continue
        if not allele.startswith(gene):
            continue
        if allele.find("BACKBONE") != -1:
            continue
        AS = None
        for col in cols[11:]:
            if col.startswith("AS"):
                AS = int(col[5:])
        assert AS is not None
        if read_id != prev_read_id:
            if alleles:
                if aligner == "hisat2" or (aligner == "bowtie2" and len(alleles) < 10):
                    add_alleles(alleles)
                alleles = set()
            prev_AS = None
        if prev_AS is not None and AS < prev_AS:
            continue
        prev_read_id = read_id
        prev_AS = AS
        alleles.add(allele)
    if alleles:
        add_alleles(alleles)
    return Gene_counts, Gene_cmpt


def counts_sorted(Gene_counts):
    """core:1650-1651: by count, descending, stable over insertion order."""
    return sorted([[a, c] for a, c in Gene_counts.items()], key=lambda x: x[1], reverse=True)


def abundance(Gene_cmpt, is_hla, stats=None):
    """core:1681-1797 for the linear branch: HLA -> single_abundance({}) = [] (Gene_exons_cmpt is empty), else
    single_abundance(Gene_cmpt) with the default flags; one class raises TypeError (Gene_cmpt.keys()[0], core:1795)."""
    if is_hla:
        return []
    if len(Gene_cmpt) <= 1:
        if len(Gene_cmpt) == 1:
            raise TypeError("'dict_keys' object is not subscriptable (typing_core.py:1795)")
        return []
    return pyref.single_abundance(Gene_cmpt, False, None, stats)


def report_lines(counts, gene_prob, simulation=False, true_alleles=(), output_allele_counts=False, best_alleles=False):
    """The section body of one locus (core:1650-1672, 2076-2121): no 'reads and pairs' line in the linear branch."""
    out = []
    for i, (a, c) in enumerate(counts):
        if simulation:
            found = False
            for t in true_alleles:
                if a == t:
                    out.append("\t\t\t*** %d ranked %s (count: %d)" % (i + 1, t, c))
                    found = True
            if i < 5 and not found:
                out.append("\t\t\t\t%d %s (count: %d)" % (i + 1, a, c))
        else:
            out.append("\t\t\t\t%d %s (count: %d)" % (i + 1, a, c))
            if i >= 9 and not output_allele_counts:
                break
    out.append("\n")
    for i, (a, p) in enumerate(gene_prob):
        if p < 0.01:
            break
        out.append("\t\t\t\t%d ranked %s (abundance: %.2f%%)" % (i + 1, a, p * 100.0))
        if best_alleles and i < 2:
            out.append("SingleModel %s (abundance: %.2f%%)" % (a, p * 100.0))
        if not simulation and i >= 9:
            break
        if i >= 19:
            break
    return out


def run(sam_text, gene, aligner, is_hla, output_allele_counts=False):
    """Everything the linear branch computes for one locus: dict with counts (dict order), classes (dict order), the sorted
    counts, the abundance list (or the exception) and the section's report lines."""
    Gene_counts, Gene_cmpt = gene_counts_and_classes(records(sam_text), gene, aligner)
    out = {"counts": Gene_counts, "classes": Gene_cmpt, "counts_sorted": counts_sorted(Gene_counts), "error": None}
    st = {}
    try:
        out["gene_prob"] = abundance(Gene_cmpt, is_hla, st)
    except TypeError as e:
        out["gene_prob"], out["error"] = None, e
        return out
    out["n_iter"] = st.get("n_iter")
    out["report"] = report_lines(out["counts_sorted"], out["gene_prob"], output_allele_counts=output_allele_counts)
    return out
