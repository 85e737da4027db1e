"""Inputs the aligner's three statements (tests/align_ref.py, the host route, the kernels) are judged on: the simulated reads of
tests/golden/selftest_loop.json.gz, reads of a synth locus, and hand-made loci with their expected records."""
import contextlib
import gzip
import io
import json
import os
import random

import align_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def selftest_calls(case, workdir):
    """The typing() calls of the self-test loop on golden case `case`, without typing anything: one dict per call with the
    reference dicts and the simulated reads [(name, seq, None)] of both mates as that call would have aligned them."""
    from hisatgenotype_amd import driver
    import hisatgenotype_amd as hgx
    with gzip.open(os.path.join(HERE, "golden", "selftest_loop.json.gz"), "rb") as f:
        spec = json.loads(f.read().decode())[case]
    ix_dir, out_dir = os.path.join(workdir, "ix"), os.path.join(workdir, "out")
    os.makedirs(ix_dir)
    os.makedirs(out_dir)
    for name, text in spec["index_files"].items():
        with open(os.path.join(ix_dir, name), "w") as f:
            f.write(text)
    calls = []

    def stub(*a, **k):
        calls.append(dict(refGenes=a[6], Genes=a[7], Vars=a[11], Var_list=a[12], num_editdist=a[15], args=a,
                          reads=[align_ref.read_records(p) for p in a[25]]))
        return {}

    p = spec["params"]
    cwd, real = os.getcwd(), driver.typing
    driver.typing = stub
    os.chdir(workdir)
    try:
        with contextlib.redirect_stderr(io.StringIO()):
            hgx.genotyping_locus("hla", list(spec["gene_order"]), "", ix_dir, [], True, [["hisat2", "graph"]], [], False, "",
                                 1, p["simulate_interval"], p["read_len"], p["fragment_len"], False, 2, p["perbase_errorrate"],
                                 0.0, [], False, "assembly_graph", True, False, False, False, True, [], 0, False, out_dir,
                                 False, dict(p["debug"]))
    finally:
        driver.typing = real
        os.chdir(cwd)
    return calls


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def fasta(records):
    return "".join(">%s\n%s\n" % (n, s) for n, s in records).encode()


def fastq(records):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, q) for n, s, q in records).encode()


# ------------------------------------------------------------------------------------------------------------------
# hand-made loci.  Every backbone is random (seeded) except where a case needs a homopolymer or a repeat; reads are cut from
# the backbone with the named variants applied, so the expected record can be written down from the construction.
# ------------------------------------------------------------------------------------------------------------------
def _bb(seed, n):
    return rand_seq(random.Random(seed), n)


def _other(b, k=1):
    return "ACGT"[("ACGT".index(b) + k) % 4]


def hand_cases():
    """[(title, [Locus], reads [(name, seq)], max_edits, expected)] with expected = one entry per read: None (unaligned) or
    (flag, rname, pos1, mapq, cigar, "NM:i:.. MD:Z:.. [Zs:Z:..] NH:i:.." tags joined by tabs, without YT)."""
    cases = []
    L = align_ref.Locus

    # -- two singles with different data at one position ------------------------------------------------------------
    bb = _bb(1, 400)
    a, b_ = _other(bb[150], 1), _other(bb[150], 2)
    loc = L("H1*BACKBONE", bb, [("single", 150, a, "hv0"), ("single", 150, b_, "hv1")])
    r0 = bb[100:150] + a + bb[151:200]
    r1 = bb[100:150] + b_ + bb[151:200]
    r2 = bb[100:150] + _other(bb[150], 3) + bb[151:200]
    cases.append(("two singles at one position", [loc], [("a", r0), ("b", r1), ("c", r2)], 2, [
        (0, "H1*BACKBONE", 101, 60, "100M", "NM:i:0\tMD:Z:50%s49\tZs:Z:50|S|hv0\tNH:i:1" % bb[150]),
        (0, "H1*BACKBONE", 101, 60, "100M", "NM:i:0\tMD:Z:50%s49\tZs:Z:50|S|hv1\tNH:i:1" % bb[150]),
        (0, "H1*BACKBONE", 101, 60, "100M", "NM:i:1\tMD:Z:50%s49\tNH:i:1" % bb[150])]))

    # -- a deletion inside a homopolymer beside a second known deletion one base on (the tie) -----------------------------
    bb = _bb(2, 200)[:150] + "CAAAAAAG" + _bb(3, 242)            # A-run at 151..156
    loc = L("H2*BACKBONE", bb, [("deletion", 152, "1", "hv0"), ("deletion", 153, "1", "hv1")])
    read = bb[100:152] + bb[153:201]                              # one A fewer: both deletions explain it; hv0 is first in Var_list
    cases.append(("homopolymer deletion tie", [loc], [("t", read)], 2, [
        (0, "H2*BACKBONE", 101, 60, "52M1D48M", "NM:i:0\tMD:Z:52^A48\tZs:Z:52|D|hv0\tNH:i:1")]))

    # -- adjacent deletions: the second starts where the first ends, so only one of them can be taken in one walk; a read that
    #    lacks both stretches is explained by the covering deletion hv2 -------------------------------------------------------
    bb = _bb(4, 400)
    loc = L("H3*BACKBONE", bb, [("deletion", 150, "3", "hv0"), ("deletion", 150, "7", "hv2"), ("deletion", 153, "4", "hv1")])
    ra = bb[100:150] + bb[153:203]
    rb = bb[100:150] + bb[157:207]
    rc = bb[100:153] + bb[157:204]
    cases.append(("adjacent deletions", [loc], [("a", ra), ("b", rb), ("c", rc)], 2, [
        (0, "H3*BACKBONE", 101, 60, "50M3D50M", "NM:i:0\tMD:Z:50^%s50\tZs:Z:50|D|hv0\tNH:i:1" % bb[150:153]),
        (0, "H3*BACKBONE", 101, 60, "50M7D50M", "NM:i:0\tMD:Z:50^%s50\tZs:Z:50|D|hv2\tNH:i:1" % bb[150:157]),
        (0, "H3*BACKBONE", 101, 60, "53M4D47M", "NM:i:0\tMD:Z:53^%s47\tZs:Z:53|D|hv1\tNH:i:1" % bb[153:157])]))

    # -- insertions: inside a read, cut by the right end, the left end falling into one (not taken) -----------------------
    bb = _bb(5, 400)
    ins = "GATTACAGG"
    loc = L("H4*BACKBONE", bb, [("insertion", 200, ins, "hv0")])
    inside = bb[150:200] + ins + bb[200:241]
    cut = bb[104:200] + ins[:4]
    left_in = ins[5:] + bb[200:296]                                # its first 4 bases are inserted ones: unknown edits or unaligned
    cases.append(("insertions", [loc], [("in", inside), ("cut", cut), ("lf", left_in)], 4, [
        (0, "H4*BACKBONE", 151, 60, "50M9I41M", "NM:i:0\tMD:Z:91\tZs:Z:50|I|hv0\tNH:i:1"),
        (0, "H4*BACKBONE", 105, 60, "96M4I", "NM:i:0\tMD:Z:96\tZs:Z:96|I|hv0\tNH:i:1"),
        (0, "H4*BACKBONE", 197, 60, "100M", "NM:i:%d\tMD:Z:%s\tNH:i:1" % _plain_md(bb, 196, left_in))]))

    # -- an insertion and a deletion at one position ------------------------------------------------------------------------
    bb = _bb(6, 400)
    loc = L("H5*BACKBONE", bb, [("deletion", 200, "5", "hv0"), ("insertion", 200, "CCATGG", "hv1")])
    both = bb[150:200] + "CCATGG" + bb[205:249]
    only_i = bb[150:200] + "CCATGG" + bb[200:244]
    only_d = bb[150:200] + bb[205:255]
    cases.append(("insertion and deletion at one position", [loc], [("both", both), ("i", only_i), ("d", only_d)], 2, [
        (0, "H5*BACKBONE", 151, 60, "50M6I5D44M", "NM:i:0\tMD:Z:50^%s44\tZs:Z:50|I|hv1,6|D|hv0\tNH:i:1" % bb[200:205]),
        (0, "H5*BACKBONE", 151, 60, "50M6I44M", "NM:i:0\tMD:Z:94\tZs:Z:50|I|hv1\tNH:i:1"),
        (0, "H5*BACKBONE", 151, 60, "50M5D50M", "NM:i:0\tMD:Z:50^%s50\tZs:Z:50|D|hv0\tNH:i:1" % bb[200:205])]))

    # -- the - strand, a read with N, NM at max_edits and one more ----------------------------------------------------------
    bb = _bb(7, 300)
    loc = L("H6*BACKBONE", bb, [("single", 120, _other(bb[120]), "hv0")])
    fwd = bb[100:120] + _other(bb[120]) + bb[121:180]
    with_n = bb[60:90] + "N" + bb[91:140]
    e2 = bb[30:50] + _other(bb[50]) + bb[51:70] + _other(bb[70]) + bb[71:110]
    e3 = e2[:60] + _other(e2[60]) + e2[61:]
    cases.append(("strand, N, edit budget", [loc], [("rc", align_ref.revcomp(fwd)), ("n", with_n), ("e2", e2), ("e3", e3)], 2, [
        (16, "H6*BACKBONE", 101, 60, "80M", "NM:i:0\tMD:Z:20%s59\tZs:Z:20|S|hv0\tNH:i:1" % bb[120]),
        (0, "H6*BACKBONE", 61, 60, "80M", "NM:i:1\tMD:Z:30%s49\tNH:i:1" % bb[90]),
        (0, "H6*BACKBONE", 31, 60, "80M", "NM:i:2\tMD:Z:20%s19%s39\tNH:i:1" % (bb[50], bb[70])),
        None]))

    # -- two loci sharing a 120 bp segment; a repeat inside one locus ----------------------------------------------------
    shared = _bb(8, 120)
    la = L("H7*BACKBONE", _bb(9, 200) + shared + _bb(10, 100), [])
    lb = L("H8*BACKBONE", _bb(11, 90) + shared + _bb(12, 150), [])
    rep = _bb(13, 110)
    lc = L("H9*BACKBONE", _bb(14, 100) + rep + _bb(15, 80) + rep + _bb(16, 100), [])
    cases.append(("shared segment and repeat", [la, lb, lc], [("sh", shared[10:110]), ("rp", rep[5:105]), ("u", la.bb[20:120])], 2, [
        (0, "H7*BACKBONE", 211, 1, "100M", "NM:i:0\tMD:Z:100\tNH:i:2"),
        (0, "H9*BACKBONE", 106, 1, "100M", "NM:i:0\tMD:Z:100\tNH:i:2"),
        (0, "H7*BACKBONE", 21, 60, "100M", "NM:i:0\tMD:Z:100\tNH:i:1")]))
    return cases


def _plain_md(bb, pos0, s):
    nm, md, run = 0, "", 0
    for k, c in enumerate(s):
        if c == bb[pos0 + k]:
            run += 1
        else:
            md += "%d%s" % (run, bb[pos0 + k])
            run, nm = 0, nm + 1
    return nm, md + "%d" % run


def expected_text(loci, reads, expected):
    """The single-end SAM text the hand-written records of a case make up."""
    lines = ["@SQ\tSN:%s\tLN:%d" % (l.name, len(l.bb)) for l in loci]
    for (name, seq), e in zip(reads, expected):
        if e is None:
            continue
        flag, rname, pos1, mapq, cigar, tags = e
        s = align_ref.revcomp(seq) if flag & 16 else seq
        lines.append("\t".join([name, str(flag), rname, str(pos1), str(mapq), cigar, "*", "0", "0", s, "I" * len(s), tags, "YT:Z:UU"]))
    return "\n".join(lines) + "\n"


def synth_reads(err_percent, workdir, interval=97, seed=3):
    """(reference dicts, [mate-1 records, mate-2 records]) of simulate_reads over two alleles of a synth HLA-like locus (its
    variants include deletions), `err_percent` per-base errors."""
    from hisatgenotype_amd import simulate, synth
    loc = synth.make_hla_like_locus(n_alleles=60, n_vars=500, seed=seed)
    d = loc.reference_dicts()
    alleles = [a for a in loc.allele_names[1:] if len(loc.allele_vars.get(a, [])) >= 5][:2]
    state, cwd = random.getstate(), os.getcwd()
    os.chdir(workdir)
    try:
        random.seed(seed)
        simulate.simulate_reads(d["Genes"], "synth", [alleles], d["Vars"], d["Links"], simulate_interval=interval,
                                perbase_errorrate=err_percent, out_dir=workdir)
        reads = [align_ref.read_records(os.path.join(workdir, "synth_input_%d.fa" % m)) for m in (1, 2)]
    finally:
        random.setstate(state)
        os.chdir(cwd)
    return d, reads


# ------------------------------------------------------------------------------------------------------------------
# the inputs the host route (tests/test_align_host.py) and the kernels (tests/test_gpu_align.py) are compared on, each with
# the Python statement's text, computed once per process
# ------------------------------------------------------------------------------------------------------------------
def dicts_of(loci):
    """Reference dicts (Genes, Vars, Var_list, refGenes) of hand-made loci."""
    Genes, Vars, Var_list, refGenes = {}, {}, {}, {}
    for k, l in enumerate(loci):
        g = "G%d" % k
        Genes[g] = {l.name: l.bb}
        refGenes[g] = l.name
        Vars[g] = {vid: [t, p, d] for t, p, d, vid in l.variants}
        Var_list[g] = [[p, vid] for t, p, d, vid in l.variants]
    return Genes, Vars, Var_list, refGenes


def pair_loci():
    return [align_ref.Locus("P1*BACKBONE", _bb(21, 2500), [("single", 150, _other(_bb(21, 2500)[150]), "hv0")]),
            align_ref.Locus("P2*BACKBONE", _bb(22, 600), [])]


def pair_reads():
    """(mate-1 records, mate-2 records, expected (FLAG, YT) per written record): concordant in both orientations, too far apart,
    same strand, facing outwards, two loci, one mate unaligned, both unaligned."""
    a, b = (l.bb for l in pair_loci())
    rc = align_ref.revcomp
    junk = _bb(23, 100)
    m1 = [("fr", a[100:200]), ("rf", rc(a[300:400])), ("far", a[0:100]), ("same", a[100:200]), ("out", rc(a[100:200])),
          ("loci", a[100:200]), ("half", a[500:600]), ("none", junk)]
    m2 = [("fr", rc(a[300:400])), ("rf", a[100:200]), ("far", rc(a[1200:1300])), ("same", a[300:400]), ("out", a[300:400]),
          ("loci", rc(b[300:400])), ("half", junk), ("none", rc(junk))]
    flags = [(99, "CP"), (147, "CP"), (83, "CP"), (163, "CP"), (97, "DP"), (145, "DP"), (65, "DP"), (129, "DP"),
             (81, "DP"), (161, "DP"), (97, "DP"), (145, "DP"), (73, "UP")]
    return m1, m2, flags


LENGTHS = [15, 16, 17, 19, 20, 63, 64, 65, 100, 250]


def length_locus():
    bb = _bb(31, 1600)
    return align_ref.Locus("L1*BACKBONE", bb, [("single", 40, _other(bb[40]), "hv0"), ("deletion", 300, "2", "hv1")])


def length_reads(lengths):
    bb = length_locus().bb
    return [("len%d" % n, bb[20:20 + n]) for n in lengths]


def _quals(seq, k):
    return "".join(chr(33 + (k + j) % 40) for j in range(len(seq)))


_INPUTS = {}


def inputs():
    """{id: (dicts, [input texts (bytes)], max_edits)}"""
    if _INPUTS:
        return _INPUTS
    import shutil
    import tempfile
    for k, (title, loci, reads, me, _) in enumerate(hand_cases()):
        _INPUTS["hand%d" % k] = (dicts_of(loci), [fasta(reads)], me)
    tmp = tempfile.mkdtemp()
    try:
        for case in ("pairs_two_genes", "single_test_id_and_list", "basic_with_errors"):
            for n, c in enumerate(selftest_calls(case, os.path.join(tmp, case))):
                texts = [fasta([(q, s) for q, s, _ in m]) for m in c["reads"]]
                _INPUTS["%s-%d" % (case, n)] = ((c["Genes"], c["Vars"], c["Var_list"], c["refGenes"]), texts, c["num_editdist"])
        for err in (0.0, 1.0):
            os.makedirs(os.path.join(tmp, "s%d" % err))
            d, reads = synth_reads(err, os.path.join(tmp, "s%d" % err))
            texts = [fasta([(q, s) for q, s, _ in m]) for m in reads]
            _INPUTS["synth-err%d" % err] = ((d["Genes"], d["Vars"], d["Var_list"], d["refGenes"]), texts, 2)
    finally:
        shutil.rmtree(tmp)
    # formats: FASTA and FASTQ, plain and .gz, single and paired, on the pair cases; names with '|', a trailing /1, words behind
    m1, m2, _ = pair_reads()
    m1 = [("%s|x/1 some words" % n if k == 0 else n + "\tmore" if k == 1 else n, s) for k, (n, s) in enumerate(m1)]
    m2 = [("%s|x/2" % n if k == 0 else n, s) for k, (n, s) in enumerate(m2)]
    pd = dicts_of(pair_loci())
    q1 = [(n, s, _quals(s, k)) for k, (n, s) in enumerate(m1)]
    q2 = [(n, s, _quals(s, k + 7)) for k, (n, s) in enumerate(m2)]
    _INPUTS["pairs-fasta"] = (pd, [fasta(m1), fasta(m2)], 2)
    _INPUTS["pairs-fastq"] = (pd, [fastq(q1), fastq(q2)], 2)
    _INPUTS["pairs-fasta-gz"] = (pd, [gzip.compress(fasta(m1)), gzip.compress(fasta(m2))], 2)
    _INPUTS["pairs-fastq-gz"] = (pd, [gzip.compress(fastq(q1)), gzip.compress(fastq(q2))], 2)
    _INPUTS["single-fastq"] = (pd, [fastq(q1 + q2)], 2)
    _INPUTS["single-fasta-gz-multiline"] = (pd, [gzip.compress(b"".join(
        (">%s\n%s\n%s\n" % (n, s[:37], s[37:])).encode() for n, s in m1 + m2))], 2)
    _INPUTS["lengths"] = (dicts_of([length_locus()]), [fasta(length_reads(LENGTHS))], 2)
    _INPUTS["empty"] = (pd, [b""], 2)
    _INPUTS["empty-pair"] = (pd, [b"", b""], 2)
    return _INPUTS


_REF = {}


def ref_text(key):
    """The Python statement's SAM text for inputs()[key] (bytes)."""
    if key not in _REF:
        d, texts, me = inputs()[key]
        loci = align_ref.loci_from_dicts(d[0], d[1], d[2], d[3])
        _REF[key] = align_ref.align_text(loci, [align_ref.read_records(t) for t in texts], me).encode()
    return _REF[key]


INPUT_IDS = (["hand%d" % k for k in range(7)] + ["pairs_two_genes-%d" % n for n in range(3)] +
             ["single_test_id_and_list-%d" % n for n in range(2)] + ["basic_with_errors-%d" % n for n in range(4)] +
             ["synth-err0", "synth-err1", "pairs-fasta", "pairs-fastq", "pairs-fasta-gz", "pairs-fastq-gz", "single-fastq",
              "single-fasta-gz-multiline", "lengths", "empty", "empty-pair"])


# ------------------------------------------------------------------------------------------------------------------
# inputs that reach the limits of the kernels' fixed scratch (csrc/hgx_align_core.hpp: HGX_ALN_DEV_*)
# ------------------------------------------------------------------------------------------------------------------
DEV_MAX_READ, DEV_ANCHORS, DEV_STK, DEV_VARS = 256, 128, 32, 32


def limit_case(kind, n):
    """(loci, reads): `n` anchors of one read ("anchors": a 16-base read whose bases stand n times in the locus), `n` known
    1-base deletions that a 100-base read passes without taking ("stack": every one is a pending choice of the search), `n` known
    singles in one read ("vars"), a read of n bases ("length")."""
    if kind == "anchors":
        rng = random.Random(41)
        w = rand_seq(rng, 16)
        bb = "".join(rand_seq(rng, 23) + w for _ in range(n)) + rand_seq(rng, 23)
        return [align_ref.Locus("R1*BACKBONE", bb, [])], [("rep", w)]
    bb = _bb(42, 400)
    if kind == "stack":
        loc = align_ref.Locus("S1*BACKBONE", bb, [("deletion", 120 + 2 * j, "1", "hv%d" % j) for j in range(n)])
        return [loc], [("st", bb[100:200])]
    if kind == "vars":
        loc = align_ref.Locus("V1*BACKBONE", bb, [("single", 120 + 2 * j, _other(bb[120 + 2 * j]), "hv%d" % j) for j in range(n)])
        read = list(bb[100:200])
        for j in range(n):
            read[20 + 2 * j] = _other(bb[120 + 2 * j])
        return [loc], [("va", "".join(read))]
    assert kind == "length"
    return [length_locus()], length_reads([n])


def tandem_case(n, read_len=250, mismatches=1, units=40, start=60, singles=0):
    """A 360-base locus holding GATA x 40 with `n` known 4-base deletions and `n` known GATA insertions inside the repeat, and a
    read across it with `mismatches` errors right of the repeat: every combination of k deletions and k insertions leads to the
    same state, so a search that enumerates WAYS instead of states grows exponentially with n."""
    rng = random.Random(51)
    bb = rand_seq(rng, 100) + "GATA" * units + rand_seq(rng, 100)
    variants = []
    for j in range(n):
        variants.append(("deletion", 104 + 8 * j, "4", "hv%d" % (2 * j)))
        variants.append(("insertion", 108 + 8 * j, "GATA", "hv%d" % (2 * j + 1)))
    marks = [101 + singles * m for m in range(4 * units // singles)] if singles else []      # known A>C every `singles` bases, all in the read:
    variants += [("single", p, "C", "hs%d" % p) for p in marks]                             # no 16-mer of the repeat seeds, the walk costs nothing
    variants.sort(key=lambda v: v[1])
    loc = align_ref.Locus("T1*BACKBONE", bb, variants)
    read = list(bb[start:start + read_len])
    for p in marks:
        if start <= p < start + read_len:
            read[p - start] = "C"
    for m in range(mismatches):
        read[read_len - 20 - 9 * m] = _other(read[read_len - 20 - 9 * m])
    return [loc], [("tr", "".join(read))]
