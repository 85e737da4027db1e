"""Shared by tests/test_extract_golden.py and tests/test_gpu_extract.py: run extract.extract_reads on a fixture's recorded input."""
import gzip
import os

import extract_ref
from hisatgenotype_amd import extract


def run_fixture(fx, tmp, alignment="sam"):
    """-> (files {name: decompressed text}, fname_list, exception name or None, database_list afterwards, stats of the sample)."""
    a = fx["args"]
    ix_dir, out_dir = os.path.join(str(tmp), "ix"), os.path.join(str(tmp), "out")
    os.makedirs(ix_dir)
    os.makedirs(out_dir)
    with open(os.path.join(ix_dir, "genotype_genome.locus"), "w") as f:
        f.write(fx["locus"])
    for name, text in fx["pre_existing"].items():
        with gzip.open(os.path.join(out_dir, name), "wt") as f:
            f.write(text)
    if alignment == "bam":
        from hisatgenotype_amd import bamio
        path = os.path.join(str(tmp), "records.bam")
        bamio.write_bam(path, fx["sam"])
    else:
        path = os.path.join(str(tmp), "records.sam")
        with open(path, "w") as f:
            f.write(fx["sam"])
    ext = "fq" if a["fastq"] else "fa"
    read_fname = ["reads/sample_1." + ext, "reads/sample_2." + ext] if a["paired"] else ["reads/sample." + ext]
    dbl = list(a["database_list"])
    exc, fname_list = None, None
    extract.last_stats = None
    try:
        fname_list = extract.extract_reads("genotype_genome", ix_dir, dbl, "reads", out_dir, ext, read_fname, a["fastq"], a["paired"],
                                           a["simulation"], 2, 1, 1 << 62, [0, 1], a["aligner"], 0, False, alignment_fname=path)
    except (ValueError, AssertionError, SystemExit, IndexError, TypeError) as e:
        exc = type(e).__name__
    files = {}
    for n in sorted(os.listdir(out_dir)):
        with gzip.open(os.path.join(out_dir, n), "rt") as f:
            files[n] = f.read()
    return files, fname_list, exc, dbl, extract.last_stats


def check_against_fixture(fx, got):
    files, fname_list, exc, dbl, _ = got
    assert exc == fx["exception"]
    assert fname_list == fx["fname_list"]
    assert dbl == fx["database_list_after"]
    assert sorted(files) == sorted(fx["files"])
    for n in fx["files"]:
        assert files[n] == fx["files"][n], n


def spec_files(fx):
    files, exc, dbl = extract_ref.expected_files(fx)
    return files, (exc.__name__ if exc else None), dbl
