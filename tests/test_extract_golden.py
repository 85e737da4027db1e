"""Read extraction against the fixtures recorded from the real reference (tests/golden/make_extract_golden.py): the spec
(tests/extract_ref.py) and the library's host route through the C-ABI reproduce every recorded file, fname_list and exception.
No GPU needed."""
import pytest

import extract_ref

NAMES = extract_ref.fixture_names()
REQUIRED = ["hisat2_mixed_nh", "right_mate_quirk", "right_mate_last_wins", "reverse_with_n", "two_families", "overlap_break", "half_open",
            "unmapped_mates", "name_again", "unpaired", "fasta_out", "simulation_names", "database_filter", "database_append",
            "bowtie2_as_xs", "error_short_line", "error_no_mate_flag", "error_names_differ", "error_no_read2", "error_no_read1",
            "error_bowtie2_no_xs", "error_tag_value", "omit_existing", "big_random"]


def test_every_scenario_is_recorded():
    assert sorted(REQUIRED) == NAMES
    kinds = {extract_ref.load(n)["exception"] for n in NAMES}
    assert kinds == {None, "ValueError", "AssertionError", "SystemExit", "IndexError", "TypeError"}


@pytest.mark.parametrize("name", NAMES)
def test_spec_matches_reference(name):
    fx = extract_ref.load(name)
    files, exc, dbl = extract_ref.expected_files(fx)
    assert (exc.__name__ if exc else None) == fx["exception"]
    assert dbl == fx["database_list_after"]
    if fx["pre_existing"]:                      # the omit rule: nothing is run, the files stay
        assert fx["files"] == fx["pre_existing"] and fx["fname_list"] is not None
        return
    assert sorted(files) == sorted(fx["files"])
    for n, text in fx["files"].items():
        assert files[n] == text, n
    if fx["exception"] is None:
        assert fx["fname_list"] == {f: ["%s-%s" % (fx["base"], f)] for f in dbl}


def _host_library():
    try:
        from hisatgenotype_amd import capi
        capi.lib()
    except (ImportError, OSError) as e:
        pytest.skip("libhgx.so does not load here: %s" % e)


@pytest.mark.parametrize("name", NAMES)
def test_host_route_matches_reference(name, tmp_path):
    _host_library()
    import extract_cases
    from hisatgenotype_amd import engine
    fx = extract_ref.load(name)
    with engine.test_switches(front="host"):
        got = extract_cases.run_fixture(fx, tmp_path)
    extract_cases.check_against_fixture(fx, got)
    if got[4] is not None:
        assert got[4]["route"] == 0 and got[4]["chunks_device"] == 0


def test_extract_whole_is_not_built(tmp_path):
    _host_library()
    from hisatgenotype_amd import extract_reads
    with pytest.raises(NotImplementedError):
        extract_reads("genotype_genome", str(tmp_path), [], "", str(tmp_path), "fq", ["a_1.fq", "a_2.fq"], True, True, False, 1, 1, 1, [0, 1],
                      "hisat2", 1000000, False)


def test_missing_aligner_is_named(tmp_path, monkeypatch):
    _host_library()
    import os
    from hisatgenotype_amd import extract
    fx = extract_ref.load("two_families")
    ix = tmp_path / "ix"
    ix.mkdir()
    for e in ("fa", "snp", "haplotype", "link", "coord", "clnsig") + tuple("%d.ht2" % (i + 1) for i in range(8)):
        (ix / ("genotype_genome." + e)).write_text("")
    (ix / "genotype_genome.locus").write_text(fx["locus"])
    for n in ("s_1.fq", "s_2.fq"):
        (tmp_path / n).write_text("")
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError, match="hisat2"):
        extract.extract_reads("genotype_genome", str(ix), [], "", str(tmp_path / "out"), "fq", [str(tmp_path / "s_1.fq"), str(tmp_path / "s_2.fq")],
                              True, True, False, 1, 1, 1, [0, 1], "hisat2", 0, False)


def test_aligner_stream_is_fed_in_blocks(tmp_path, monkeypatch):
    """The aligner's stdout through hgx_extract_feed in blocks that cut lines and groups anywhere."""
    _host_library()
    import os
    import stat
    import extract_cases
    from hisatgenotype_amd import engine, extract
    fx = extract_ref.load("big_random")
    ix = tmp_path / "ix"
    ix.mkdir()
    for e in ("fa", "snp", "haplotype", "link", "coord", "clnsig") + tuple("%d.ht2" % (i + 1) for i in range(8)):
        (ix / ("genotype_genome." + e)).write_text("")
    (ix / "genotype_genome.locus").write_text(fx["locus"])
    bindir = tmp_path / "bin"
    bindir.mkdir()
    (tmp_path / "stub.sam").write_text(fx["sam"])
    stub = bindir / "hisat2"
    stub.write_text("#!/bin/sh\ncat '%s'\n" % (tmp_path / "stub.sam"))
    stub.chmod(stub.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    monkeypatch.setattr(extract, "FEED_BYTES", 7001)
    for n in ("sample_1.fq", "sample_2.fq"):
        (tmp_path / n).write_text("")
    out = tmp_path / "out"
    with engine.test_switches(front="host"):
        fl = extract.extract_reads("genotype_genome", str(ix), [], "", str(out), "fq", [str(tmp_path / "sample_1.fq"), str(tmp_path / "sample_2.fq")],
                                   True, True, False, 2, 1, 1, [0, 1], "hisat2", 0, False)
    assert fl == fx["fname_list"]
    import gzip
    for n, text in fx["files"].items():
        with gzip.open(str(out / n), "rt") as f:
            assert f.read() == text, n
