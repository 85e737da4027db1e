"""Linear-index typing on the device route (csrc/hgx_linear.hip) against the recorded fixtures, the host route and the
plain-Python statement (tests/linear_ref.py)."""
import importlib
import os
import random

import pytest

import linear_ref
from hisatgenotype_amd import bamio, capi, engine, synth
from hisatgenotype_amd.locus import PackedLocus
from test_linear_golden import NAMES, load, sections

ht = importlib.import_module("hisatgenotype_amd.typing")
pytestmark = pytest.mark.gpu


def both_routes(pl, sam, aligner="hisat2", **kw):
    with engine.test_switches(front="device"):
        dev = ht.linear_counts(pl, sam, aligner, **kw)
        route = engine.front_last()
    with engine.test_switches(front="host"):
        host = ht.linear_counts(pl, sam, aligner, **kw)
    return dev, route, host


def same(a, b):
    return list(a.counts.items()) == list(b.counts.items()) and list(a.classes.items()) == list(b.classes.items())


@pytest.mark.parametrize("name", NAMES)
def test_device_route_reproduces_fixture(name, tmp_path):
    capi.set_device(0)
    fx = load(name)
    opt = fx["options"]
    loc = fx["_locus"]
    pl = PackedLocus.from_synth(loc)
    bam = str(tmp_path / "lin.bam")
    refs = sorted({l.split("\t")[2] for l in fx["sam"].split("\n") if l and l.split("\t")[2] != "*"} | set(loc.allele_names))
    bamio.write_bam_native(bam, fx["sam"], [(r, 100000) for r in refs])
    try:
        got_sam, got_bam = [], []
        for aligner, _ in opt["aligners"]:
            dev, route, host = both_routes(pl, fx["sam"], aligner)
            assert route == (2, 0), route
            assert same(dev, host)
            got_sam.append((list(dev.counts.items()), list(dev.classes.items())))
            with engine.test_switches(front="device"):
                db = ht.linear_counts(pl, None, aligner, alignment_file=bam)
                assert engine.front_last() == (2, 0)
            got_bam.append((list(db.counts.items()), list(db.classes.items())))
        exp = sections(fx)
        assert got_sam[:len(exp)] == exp and got_bam[:len(exp)] == exp
        # the abundance step: the recorded single_abundance results, reference-exact
        with engine.test_switches(front="device"):
            res = ht.type_locus_linear(pl, fx["sam"], opt["aligners"][0][0])
        if fx["error"]:
            assert isinstance(res.error, TypeError)
        elif opt["base_fname"] != "hla" and len(res.classes) > 1:
            e = fx["em"][0]
            assert [[a, repr(p)] for a, p in res.gene_prob] == e["result"] and res.n_iter == e["n_iter"]
    finally:
        pl.close()


def random_sam(loc, rng, n_groups, max_k, coordinate=False, ids=None):
    al = [a for a in loc.allele_names if "BACKBONE" not in a]
    lines = []
    for g in range(n_groups):
        k = rng.randint(1, max_k)
        base = rng.randint(-40, 0)
        for j in range(k):
            lines.append("r%d\t%d\t%s\t1\t60\t20M\t*\t0\t0\tACGT\tIIII\tAS:i:%d\tNM:i:0" % (
                g if ids is None else ids(g), 0 if j == 0 else 256, rng.choice(al), base + rng.choice([0, 0, 1, -1, -3])))
        if rng.random() < 0.05:
            lines.append("r%d\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII" % g)
    if coordinate:
        rng.shuffle(lines)
    return "".join(l + "\n" for l in lines)


@pytest.mark.parametrize("layout", ["name", "coordinate"])
@pytest.mark.parametrize("aligner", ["hisat2", "bowtie2"])
def test_random_inputs_device_host_and_statement_agree(layout, aligner):
    capi.set_device(0)
    loc = synth.make_hla_like_locus(n_alleles=300, n_vars=200, seed=21)
    pl = PackedLocus.from_synth(loc)
    rng = random.Random({"name": 1, "coordinate": 2}[layout] * 10 + {"hisat2": 1, "bowtie2": 2}[aligner])
    try:
        sam = random_sam(loc, rng, 200000, 20, coordinate=(layout == "coordinate"))
        dev, route, host = both_routes(pl, sam, aligner)
        assert route == (2, 0)
        assert same(dev, host)
        c, k = linear_ref.gene_counts_and_classes(linear_ref.records(sam), loc.gene, aligner)
        assert list(dev.counts.items()) == list(c.items()) and list(dev.classes.items()) == list(k.items())
    finally:
        pl.close()


def test_million_groups_device_equals_host():
    capi.set_device(0)
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    try:
        sam = random_sam(loc, random.Random(5), 1000000, 10)
        dev, route, host = both_routes(pl, sam, "bowtie2")
        assert route == (2, 0) and same(dev, host)
        with engine.test_switches(front="device"):
            a = ht.type_locus_linear(pl, sam, "bowtie2")
        with engine.test_switches(front="host"):
            b = ht.type_locus_linear(pl, sam, "bowtie2")
        assert a.gene_prob == b.gene_prob and a.n_iter == b.n_iter
        assert ht.report_lines_linear(a) == ht.report_lines_linear(b)
    finally:
        pl.close()


def test_forced_collisions_give_the_same_classes():
    capi.set_device(0)
    loc = synth.make_hla_like_locus(n_alleles=100, n_vars=100, seed=4)
    pl = PackedLocus.from_synth(loc)
    try:
        sam = random_sam(loc, random.Random(8), 5000, 4)
        with engine.test_switches(front="host"):
            host = ht.linear_counts(pl, sam)
        with engine.test_switches(front="device", linear_collide="1"):
            dev = ht.linear_counts(pl, sam)
            assert engine.front_last()[1] == 6        # HGX_LIN_DECLINE_COLLISION: finished by the host route
        assert same(dev, host)
    finally:
        pl.close()


def test_declines_end_on_the_host_route():
    capi.set_device(0)
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    gene = loc.gene
    try:
        good = random_sam(loc, random.Random(3), 3000, 3)
        unknown = good + "z\t0\t%s*999\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tAS:i:0\n" % gene + good
        with engine.test_switches(front="device"):
            r = ht.linear_counts(pl, unknown)
            assert engine.front_last() == (0, 3)
        assert "%s*999" % gene in r.counts or any("%s*999" % gene in k for k in r.classes)
        c, k = linear_ref.gene_counts_and_classes(linear_ref.records(unknown), gene, "hisat2")
        assert list(r.counts.items()) == list(c.items()) and list(r.classes.items()) == list(k.items())
        for bad, exc in (("\tAS:f:1.5", ValueError), ("", AssertionError)):
            a = [n for n in loc.allele_names if "BACKBONE" not in n][0]
            sam = good + "z\t0\t%s\t1\t60\t4M\t*\t0\t0\tACGT\tIIII%s\n" % (a, bad)
            with engine.test_switches(front="device"):
                with pytest.raises(exc):
                    ht.linear_counts(pl, sam)
    finally:
        pl.close()


def test_declines_are_taken_by_the_device_route_first(tmp_path):
    """Each decline code on the device route, from SAM text and from BAM (AS missing), then the host route's result or error."""
    capi.set_device(0)
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    a = [n for n in loc.allele_names if "BACKBONE" not in n][0]
    try:
        good = random_sam(loc, random.Random(4), 3000, 3)
        cases = [(good + "z\t0\t%s\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tAS:f:1.5\n" % a, ValueError, 4),
                 (good + "z\t0\t%s\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\n" % a, AssertionError, 4),
                 (good + "z\t0\n", ValueError, 5),
                 (good + "z\tx\t%s\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tAS:i:0\n" % a, ValueError, 5)]
        for sam, exc, code in cases:
            with engine.test_switches(front="device"):
                with pytest.raises(exc):
                    ht.linear_counts(pl, sam)
                assert engine.front_last()[1] == code
        # BAM: a kept record without AS declines on the device, the host route raises the reference's AssertionError
        bam = str(tmp_path / "noas.bam")
        bamio.write_bam_native(bam, good + "z\t0\t%s\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n" % a, [(n, 100000) for n in loc.allele_names])
        with engine.test_switches(front="device"):
            with pytest.raises(AssertionError):
                ht.linear_counts(pl, None, alignment_file=bam)
            assert engine.front_last()[1] == 4
        # ... and a BAM without such a record stays on the device
        bam2 = str(tmp_path / "ok.bam")
        bamio.write_bam_native(bam2, good, [(n, 100000) for n in loc.allele_names])
        with engine.test_switches(front="device"):
            r = ht.linear_counts(pl, None, alignment_file=bam2)
            assert engine.front_last() == (2, 0)
        c, k = linear_ref.gene_counts_and_classes(linear_ref.records(good), loc.gene, "hisat2")
        assert list(r.counts.items()) == list(c.items()) and list(r.classes.items()) == list(k.items())
    finally:
        pl.close()


@pytest.mark.parametrize("layout", ["name", "coordinate"])
def test_random_inputs_em_and_report_equal_the_statement(layout):
    """EM doubles, iterations and report text of the device route against linear_ref (the reference's EM restated)."""
    capi.set_device(0)
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    try:
        sam = random_sam(loc, random.Random(31 if layout == "name" else 32), 200000, 4, coordinate=(layout == "coordinate"))
        with engine.test_switches(front="device"):
            res = ht.type_locus_linear(pl, sam, "hisat2")
            assert engine.front_last() == (2, 0)
        exp = linear_ref.run(sam, loc.gene, "hisat2", False)
        assert list(res.counts.items()) == list(exp["counts"].items())
        assert list(res.classes.items()) == list(exp["classes"].items())
        assert res.gene_prob == exp["gene_prob"] and res.n_iter == exp["n_iter"]
        assert ht.report_lines_linear(res) == exp["report"]
    finally:
        pl.close()


def _typing(loc, path, aligners, out):
    d = loc.reference_dicts()
    os.makedirs(out, exist_ok=True)
    ht.typing(False, os.path.join(os.path.dirname(path), loc.base_fname), [loc.gene], "", True, set(), d["refGenes"], d["Genes"],
              d["Gene_names"], d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"], aligners, 2, False,
              "assembly_graph", True, True, False, False, True, [], False, ["reads_1.fa"], path, [], 150, 400, 1, False, 0, False,
              out, "NONE", False, 0)
    rep = [f for f in os.listdir(out) if f.endswith(".report")]
    return open(os.path.join(out, rep[0])).read()


EM_FIXTURES = [n for n in NAMES if not n.endswith("_region") and not load(n)["error"]]


@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("name", EM_FIXTURES)
def test_typing_writes_the_recorded_report(name, fmt, tmp_path):
    """typing() end to end (abundance lines and two-aligner flow included) on the device route, from SAM text and from BAM."""
    capi.set_device(0)
    fx = load(name)
    loc = fx["_locus"]
    path = str(tmp_path / ("lin." + fmt))
    if fmt == "sam":
        with open(path, "w") as f:
            f.write(fx["sam"])
    else:
        refs = sorted({l.split("\t")[2] for l in fx["sam"].split("\n") if l and l.split("\t")[2] != "*"} | set(loc.allele_names))
        bamio.write_bam_native(path, fx["sam"], [(r, 100000) for r in refs])
    with engine.test_switches(front="device"):
        text = _typing(loc, path, fx["options"]["aligners"], str(tmp_path / "out"))
    k = text.index("\n\t\t%s linear" % fx["options"]["aligners"][0][0])
    assert text[k:] == fx["report"]


def test_one_file_serves_a_graph_and_a_linear_section(tmp_path):
    """aligners = [hisat2 graph, hisat2 linear] over ONE alignment file: the graph section is the graph-only call's, the linear
    section the recorded one (graph records sit on the backbone, which the linear branch filters out)."""
    capi.set_device(0)
    fx = load("linear_hla_mixed")
    loc = fx["_locus"]
    graph_sam = synth.simulate_sam_fast(loc, synth.pick_sample(loc, 3), 300, err_rate=0.002, seed=9)
    path = str(tmp_path / "both.sam")
    # the fixture's own backbone records (filtered by the linear branch, and not the last line) would be graph records without the
    # tags a graph alignment carries: left out, which leaves the linear section as recorded
    lines = [l for l in fx["sam"].split("\n") if l and l.split("\t")[2] != loc.ref_allele]
    assert fx["sam"].rstrip("\n").split("\n")[-1] == lines[-1]
    with open(path, "w") as f:
        f.write(graph_sam + ("" if graph_sam.endswith("\n") else "\n") + "".join(l + "\n" for l in lines))
    graph_only = _typing(loc, path, [["hisat2", "graph"]], str(tmp_path / "g"))
    both = _typing(loc, path, [["hisat2", "graph"], ["hisat2", "linear"]], str(tmp_path / "b"))
    g0 = graph_only.index("\n\t\thisat2 graph")
    k = both.index("\n\t\thisat2 linear")
    assert both[g0:k] + "\n" == graph_only[g0:] or both[g0:k] == graph_only[g0:]
    assert both[k:] == fx["report"]
