"""The rule of the "hgx" aligner on a LINEAR index as plain Python: the yardstick of the host route
(csrc/hgx_align_linear_host.cpp) and of the kernels (csrc/hgx_align_linear.hip), which must write these bytes.  Clarity over
speed; nothing here is shared with them.  It is NOT HISAT2 or Bowtie2 and nothing is compared with their output.

Index.  Every gene of `Genes` in dict order, every entry of Genes[gene] in dict order EXCEPT the backbone entry refGenes[gene]
(the linear typing skips records whose RNAME contains BACKBONE: indexing it would only spend k slots).  An allele's place in this
list is its index.  Sequences are upper-cased; an allele base outside ACGT matches no read base.

Seeds.  K = 16.  The seeds of a read of length L are the disjoint 16-mers at offsets 0, 16, 32, ...: the first
min(max_edits + 1, L // 16) of them, on each strand's oriented read.  A seed that holds a base outside ACGT does not seed.

Hits.  (allele, pos0, strand) with 0 <= pos0 <= len(allele) - L, Hamming distance NM <= max_edits between the oriented read and
allele[pos0 : pos0 + L] (a read N is a mismatch), and at least one seed matching exactly at its place.  With
L >= 16 * (max_edits + 1) the last condition is implied (pigeonhole): hits_brute() is the seedless form.  L < 16 has no hit.

Order and k.  A read's hits by (NM, allele index, pos0, strand); the first min(k, hits) are written.  Mates are placed
independently.

Records.  QNAME as the graph aligner cuts it; FLAG = 0x1 + 0x40 / 0x80 (paired input) + 0x10 (reverse strand) + 0x100 (every record
of the read but its first) + 0x8 (the mate wrote nothing), never 0x2 or 0x20; RNAME the allele's name; POS pos0 + 1; MAPQ 60 if the
read has ONE hit, else 1; CIGAR <L>M; RNEXT *, PNEXT 0, TLEN 0 (deliberately: the linear branch of the typing reads none of them, and
mates are not placed together); SEQ and QUAL oriented as the graph aligner's records are (FASTA input: 'I' x L); tags AS:i:<-6 NM>,
NM:i, MD:Z, NH:i:<records written for this read>.

Text.  @HD, one @SQ per indexed allele in index order, the records in read order (mate 1's before mate 2's): a pair's records are
one run of one read id.
"""
import gzip

K = 16
ACGT = frozenset("ACGT")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
HEADER = "@HD\tVN:1.0\tSO:unsorted"


def revcomp(s):
    return "".join(_COMP.get(b, b) for b in reversed(s))


def index_of(Genes, refGenes):
    """[(name, SEQUENCE)] in index order."""
    return [(name, seq.upper()) for g in Genes for name, seq in Genes[g].items() if name != refGenes[g]]


def seeds(s, max_edits):
    """[(offset, 16-mer)] of the oriented read that seed."""
    out = []
    for j in range(min(max_edits + 1, len(s) // K)):
        w = s[j * K:(j + 1) * K]
        if set(w) <= ACGT:
            out.append((j * K, w))
    return out


def hamming(s, window, stop=None):
    """Mismatches of the oriented read on the window (a base outside ACGT on either side matches nothing); counting stops once
    `stop` is passed."""
    nm = 0
    for a, b in zip(s, window):
        if a != b or a not in ACGT:
            nm += 1
            if stop is not None and nm > stop:
                break
    return nm


def hits(alleles, seq, max_edits, seeded=True):
    """The read's hits, ordered: [(NM, allele index, pos0, strand)]."""
    seq = seq.upper()
    L = len(seq)
    out = []
    if L < K:
        return out
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        sd = seeds(s, max_edits)
        for a, (_, text) in enumerate(alleles):
            for pos0 in range(0, len(text) - L + 1):
                w = text[pos0:pos0 + L]
                nm = hamming(s, w, max_edits)
                if nm > max_edits:
                    continue
                if seeded and not any(w[o:o + K] == word for o, word in sd):
                    continue
                out.append((nm, a, pos0, strand))
    return sorted(out)


def candidates(alleles, seq, max_edits):
    """Seed-table entries the read looks at: for every seeding seed of both strands, the places of its 16-mer in the alleles."""
    seq = seq.upper()
    n = 0
    for strand in (0, 1):
        s = seq if strand == 0 else revcomp(seq)
        for _, word in seeds(s, max_edits):
            for _, text in alleles:
                n += sum(1 for p in range(len(text) - K + 1) if text[p:p + K] == word)
    return n


def hits_brute(alleles, seq, max_edits):
    return hits(alleles, seq, max_edits, seeded=False)


def md_of(s, window):
    md, run = [], 0
    for a, b in zip(s, window):
        if a == b and a in ACGT:
            run += 1
        else:
            md.append("%d%s" % (run, b))
            run = 0
    md.append("%d" % run)
    return "".join(md)


def read_records(path_or_text):
    """[(qname, seq, qual or None)] of a FASTA / FASTQ file (plain or .gz) or of its text (bytes)."""
    if isinstance(path_or_text, bytes):
        data = path_or_text
    else:
        with open(path_or_text, "rb") as f:
            data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = [l.rstrip("\r") for l in data.decode().split("\n")]
    if lines and lines[-1] == "":
        lines.pop()
    out, k = [], 0
    while k < len(lines):
        head = lines[k]
        name = head[1:].split()[0] if head[1:].split() else ""
        if head.startswith("@"):
            out.append((name, lines[k + 1], lines[k + 3]))
            k += 4
        elif head.startswith(">"):
            k += 1
            seq = ""
            while k < len(lines) and not lines[k].startswith(">"):
                seq += lines[k]
                k += 1
            out.append((name, seq, None))
        else:
            raise ValueError("neither FASTA nor FASTQ: %r" % head[:40])
    return out


def align_text(alleles, reads, max_edits=2, k=10):
    """The SAM text for `reads` = [records of file 1] or [records of file 1, records of file 2]."""
    paired = len(reads) == 2
    lines = [HEADER] + ["@SQ\tSN:%s\tLN:%d" % (name, len(text)) for name, text in alleles]
    memo = {}                                        # hits() is a function of the sequence alone: equal reads are searched once

    def hits_of(seq):
        if seq not in memo:
            memo[seq] = hits(alleles, seq, max_edits)
        return memo[seq]

    for i in range(len(reads[0])):
        found = [hits_of(reads[m][i][1]) for m in range(len(reads))]
        for m in range(len(reads)):
            qname, seq, qual = reads[m][i]
            seq = seq.upper()
            h = found[m]
            written = h[:k]
            for rank, (nm, a, pos0, strand) in enumerate(written):
                s = seq if strand == 0 else revcomp(seq)
                q = ("I" * len(s)) if qual is None else (qual if strand == 0 else qual[::-1])
                flag = 0x10 if strand else 0
                if paired:
                    flag |= 0x1 | (0x40 if m == 0 else 0x80)
                    if not found[1 - m]:
                        flag |= 0x8
                if rank:
                    flag |= 0x100
                name, text = alleles[a]
                tags = ["AS:i:%d" % (-6 * nm), "NM:i:%d" % nm, "MD:Z:%s" % md_of(s, text[pos0:pos0 + len(s)]), "NH:i:%d" % len(written)]
                lines.append("\t".join([qname, str(flag), name, str(pos0 + 1), "60" if len(h) == 1 else "1", "%dM" % len(s), "*", "0", "0",
                                        s, q] + tags))
    return "\n".join(lines) + "\n"


def counters(alleles, reads, max_edits=2, k=10):
    """(reads, aligned, records) of align_text's call: reads given, reads with a hit, records written."""
    n = aligned = records = 0
    memo = {}
    for m in range(len(reads)):
        for _, seq, _ in reads[m]:
            if seq not in memo:
                memo[seq] = hits(alleles, seq, max_edits)
            h = memo[seq]
            n += 1
            aligned += bool(h)
            records += min(k, len(h))
    return n, aligned, records
