"""Build tools/align_linear_host_main.cpp with -fsanitize=address,undefined (host code only; nothing is preloaded into Python) and run
it over the case table of tests/align_linear_cases.py: the index build and the host route of the "hgx" aligner on a linear index
must write the statement's bytes (tests/align_linear_ref.py) and count the statement's reads, records and candidates, with no
sanitizer report.

    python tools/align_linear_host_check.py [--keep DIR] [--cases name,name,...]

Exit status 0: every case equal and clean.  A tool, not a test: it compiles for half a minute.  build() and run_case() are also what
tools/align_linear_mutants.py runs its changed builds with.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (HGX_ALIGN_LINEAR_TABLE: a directory with another align_linear_cases.py and align_linear_ref.py, e.g. an earlier commit's tests/)
sys.path.insert(0, os.environ.get("HGX_ALIGN_LINEAR_TABLE") or os.path.join(ROOT, "tests"))

import align_linear_cases as lc          # noqa: E402
import align_linear_ref as ref           # noqa: E402

CSRC = os.path.join(ROOT, "hisat-genotype_amd", "csrc")
SANITIZE = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(exe, csrc=CSRC, flags=SANITIZE, quiet=False):
    """The stand-alone program from the sources in `csrc`; returns the compiler's exit status."""
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17"] + list(flags) + [
        "-DHGX_ALIGN_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "hgx_align_host.cpp"),
        os.path.join(csrc, "hgx_align_linear_host.cpp"), os.path.join(ROOT, "tools", "align_linear_host_main.cpp"), "-lz", "-o", exe]
    if not quiet:
        print(" ".join(cmd), flush=True)
    return subprocess.call(cmd, stderr=subprocess.DEVNULL if quiet else None)


_WANT = {}


def expected(name):
    """(the statement's text, its counters line) of the case; computed once."""
    if name not in _WANT:
        c = lc.BY_NAME[name]
        alleles = ref.index_of(c["Genes"], c["refGenes"])
        n, aligned, records = ref.counters(alleles, c["reads"], c["max_edits"], c["k"])
        cand = None
        if not name.startswith("reads-"):
            cand = sum(ref.candidates(alleles, s, c["max_edits"]) for recs in c["reads"] for _, s, _ in recs)
        _WANT[name] = (lc.ref_text(name), (n, aligned, records, cand))
    return _WANT[name]


def write_inputs(work, name):
    """The case's index file and read files under `work`; returns their paths."""
    c = lc.BY_NAME[name]
    ixf = os.path.join(work, "index.txt")
    alleles = [(n, s) for g in c["Genes"] for n, s in c["Genes"][g].items() if n != c["refGenes"][g]]
    with open(ixf, "w") as f:
        f.write("%d\n" % len(alleles) + "".join("%s %d %s\n" % (n, len(s), s) for n, s in alleles))
    paths = []
    for m, t in enumerate(lc.texts(c)):
        paths.append(os.path.join(work, "reads_%d.txt" % m))
        with open(paths[-1], "wb") as f:
            f.write(t)
    return [ixf] + paths


def run_case(exe, work, name, timeout=120, files=None):
    """(None or what differs, stderr) of one run of the program on the case (files: what write_inputs gave for it beforehand)."""
    c = lc.BY_NAME[name]
    files = files or write_inputs(work, name)
    try:
        p = subprocess.run([exe, files[0], str(c["max_edits"]), str(c["k"])] + files[1:], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        return "no end within %d s" % timeout, ""
    err = p.stderr.decode(errors="replace")
    text, (n, aligned, records, cand) = expected(name)
    if p.returncode:
        return "exit %d" % p.returncode, err
    if "runtime error" in err or "Sanitizer" in err:
        return "sanitizer report", err
    if p.stdout != text:
        return "bytes", err
    m = re.search(r"route (-?\d+) decline (-?\d+) reads (\d+) aligned (\d+) records (\d+) candidates (\d+)\s*$", err)
    if not m:
        return "no counters line", err
    got = tuple(int(x) for x in m.groups())
    if got[:2] != (0, 7) or got[2:5] != (n, aligned, records):
        return "counters", err
    if cand is not None and got[5] != cand:
        return "candidates", err
    return None, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None)
    ap.add_argument("--cases", default=None)
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "align_linear_host_main")
    if build(exe):
        return 1
    names = a.cases.split(",") if a.cases else lc.NAMES
    bad = 0
    for name in names:
        why, err = run_case(exe, work, name)
        print("%-36s %s  %s" % (name, "ok" if why is None else "FAILED (%s)" % why, err.strip().split("\n")[-1]), flush=True)
        if why is not None:
            bad += 1
            sys.stderr.write(err[-3000:])
    print("%d of %d cases clean and equal" % (len(names) - bad, len(names)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
