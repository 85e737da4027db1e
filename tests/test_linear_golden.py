"""Linear-index typing (typing_core.py:1597-1677) against fixtures recorded from the real reference
(tests/golden/make_linear_golden.py): the plain-Python statement (tests/linear_ref.py), the host route through the C-ABI, and
typing() itself.  No GPU: the inputs are below the device route's record gate, and the abundances are checked on the GPU
(tests/test_gpu_linear.py)."""
import glob
import gzip
import json
import os

import pytest

import importlib

import linear_ref
from hisatgenotype_amd import synth
from hisatgenotype_amd.locus import PackedLocus

ht = importlib.import_module("hisatgenotype_amd.typing")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[:-len(".json.gz")] for p in glob.glob(os.path.join(GOLDEN, "linear_*.json.gz")))


def load(name):
    with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rb") as f:
        fx = json.loads(f.read().decode())
    fx["_locus"] = synth.Locus.from_json(fx["locus"])
    return fx


def sections(fx):
    """Per aligner: (counts, classes) as lists in dict order; an aligner section without any class left no capture."""
    out = [(list(map(tuple, s["counts"])), list(map(tuple, s["classes"]))) for s in fx["sections"]]
    while len(out) < len(fx["options"]["aligners"]) and not fx["error"]:
        out.append(([], []))
    return out


def reference_report(fx, per_section):
    """The report text linear_ref writes for the fixture's sections (abundances: the recorded ones)."""
    txt = ""
    ems = iter(fx["em"])
    for (aligner, index_type), (counts, classes) in zip(fx["options"]["aligners"], per_section):
        txt += "\n\t\t%s %s\n" % (aligner, index_type)
        cs = linear_ref.counts_sorted(dict(counts))
        gp = []
        if fx["options"]["base_fname"] == "hla" or len(classes) > 1:
            gp = [[a, float(p)] for a, p in next(ems)["result"]]
        txt += "\n".join(linear_ref.report_lines(cs, gp)) + "\n"
    return txt


def test_fixtures_present():
    assert len(NAMES) >= 16


@pytest.mark.parametrize("name", NAMES)
def test_linear_ref_reproduces_fixture(name):
    fx = load(name)
    opt = fx["options"]
    got = []
    for aligner, _ in opt["aligners"]:
        c, k = linear_ref.gene_counts_and_classes(linear_ref.records(fx["sam"]), opt["gene"], aligner)
        got.append((list(c.items()), list(k.items())))
    exp = sections(fx)
    assert got[:len(exp)] == exp
    # abundance: the recorded single_abundance calls, in order (HLA: single_abundance({}) = [])
    ems = iter(fx["em"])
    for c, k in got:
        try:
            st = {}
            gp = linear_ref.abundance(dict(k), opt["base_fname"] == "hla", st)
        except TypeError:
            assert fx["error"] and fx["error"].startswith("TypeError")
            return
        if opt["base_fname"] == "hla" or len(k) > 1:
            e = next(ems)
            assert [[a, repr(float(p))] for a, p in gp] == e["result"]
            if opt["base_fname"] != "hla":
                assert st["n_iter"] == e["n_iter"]
    if not fx["error"]:
        assert reference_report(fx, got) == fx["report"]


@pytest.mark.parametrize("name", NAMES)
def test_host_route_reproduces_fixture(name):
    """Gene_counts and Gene_cmpt through the C-ABI (hgx_linear_type_sam; the host route below the record gate)."""
    fx = load(name)
    opt = fx["options"]
    pl = PackedLocus.from_synth(fx["_locus"])
    try:
        got = []
        for aligner, _ in opt["aligners"]:
            res = ht.linear_counts(pl, fx["sam"], aligner)
            assert res.route == 0
            got.append((list(res.counts.items()), list(res.classes.items())))
        exp = sections(fx)
        assert got[:len(exp)] == exp
    finally:
        pl.close()


def test_host_route_words_the_reference_errors():
    loc = synth.make_str_like_locus(seed=3)
    pl = PackedLocus.from_synth(loc)
    a = [n for n in loc.allele_names if "BACKBONE" not in n][0]
    base = "\t".join(["r", "0", a, "1", "60", "20M", "*", "0", "0", "ACGT", "IIII"])
    try:
        with pytest.raises(AssertionError):
            ht.linear_counts(pl, base + "\tNM:i:0\n")
        with pytest.raises(ValueError):
            ht.linear_counts(pl, base + "\tAS:f:1.5\n")
        # a record the filters skip needs no AS
        res = ht.linear_counts(pl, "\t".join(["r", "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]) + "\n")
        assert res.counts == {} and res.classes == {}
    finally:
        pl.close()


def _run_typing(fx, tmp_path):
    loc = fx["_locus"]
    d = loc.reference_dicts()
    sam = tmp_path / "lin.sam"
    sam.write_text(fx["sam"])
    out = tmp_path / "out"
    out.mkdir()
    err = None
    try:
        ht.typing(False, str(tmp_path / loc.base_fname), [loc.gene], fx["options"]["genotype_genome"], True, set(), d["refGenes"],
                  d["Genes"], d["Gene_names"], d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"],
                  fx["options"]["aligners"], 2, False, "assembly_graph", True, True, False, False, True, [], False,
                  ["reads_1.fa"], str(sam), [], 150, 400, 1, False, 0, False, str(out), "NONE", False, 0)
    except Exception as e:
        err = e
    rep = [f for f in os.listdir(out) if f.endswith(".report")]
    text = open(os.path.join(out, rep[0])).read()
    k = text.index("\n\t\t%s linear" % fx["options"]["aligners"][0][0])
    return text[k:], err


# the fixtures whose abundance step runs no EM (HLA: single_abundance({}); no class; one class): typing() end to end on the CPU
# (the region fixtures are left out here: the recording's stub samtools ignores a region, typing() applies it as samtools does)
NO_EM = [n for n in NAMES if (n.startswith("linear_hla_") or n in ("linear_codis_zero_classes", "linear_codis_one_class",
                                                                     "linear_codis_other_aligner")) and not n.endswith("_region")]


@pytest.mark.parametrize("name", NO_EM)
def test_typing_linear_writes_the_recorded_report(name, tmp_path):
    fx = load(name)
    text, err = _run_typing(fx, tmp_path)
    assert text == fx["report"]
    if fx["error"]:
        assert err is not None and fx["error"].split(":")[0] == type(err).__name__
    else:
        assert err is None


def test_typing_linear_simulation_stays_outside(tmp_path):
    loc = synth.make_str_like_locus(seed=3)
    d = loc.reference_dicts()
    with pytest.raises(NotImplementedError, match="linear index"):
        ht.typing(True, "/nonexistent/codis", [[loc.allele_names[1]]], "", True, set(), d["refGenes"], d["Genes"],
                  d["Gene_names"], d["Gene_lengths"], d["refGene_loci"], d["Vars"], d["Var_list"], d["Links"],
                  [["hisat2", "linear"]], 2, False, "x", True, False, False, False, True, [], False, ["r.fa"], "", [], 150, 400,
                  1, False, 0, False, str(tmp_path), "NONE", False, 0)
