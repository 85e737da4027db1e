"""Build tools/align_linear_host_main.cpp with -fsanitize=address,undefined (host code only; nothing is preloaded into Python) and run
it over the case table of tests/align_linear_cases.py: the index build and the host route of the "hgx" aligner on a linear index
must write the statement's bytes (tests/align_linear_ref.py) with no sanitizer report.

    python tools/align_linear_host_check.py [--keep DIR] [--cases name,name,...]

Exit status 0: every case equal and clean.  A tool, not a test: it compiles for half a minute.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_linear_cases as lc          # noqa: E402
import align_linear_ref as ref           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None)
    ap.add_argument("--cases", default=None)
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "align_linear_host_main")
    csrc = os.path.join(ROOT, "hisat-genotype_amd", "csrc")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DHGX_ALIGN_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "hgx_align_host.cpp"),
           os.path.join(csrc, "hgx_align_linear_host.cpp"), os.path.join(ROOT, "tools", "align_linear_host_main.cpp"), "-lz", "-o", exe]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    names = a.cases.split(",") if a.cases else lc.NAMES
    bad = 0
    for name in names:
        c = lc.BY_NAME[name]
        ixf = os.path.join(work, "index.txt")
        alleles = [(n, s) for g in c["Genes"] for n, s in c["Genes"][g].items() if n != c["refGenes"][g]]
        with open(ixf, "w") as f:
            f.write("%d\n" % len(alleles) + "".join("%s %s\n" % (n, s) for n, s in alleles))
        paths = []
        for m, t in enumerate(lc.texts(c)):
            paths.append(os.path.join(work, "reads_%d.txt" % m))
            with open(paths[-1], "wb") as f:
                f.write(t)
        p = subprocess.run([exe, ixf, str(c["max_edits"]), str(c["k"])] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        ok = p.returncode == 0 and p.stdout == lc.ref_text(name) and b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr
        print("%-32s %s  %s" % (name, "ok" if ok else "FAILED (exit %d)" % p.returncode, p.stderr.decode(errors="replace").strip().split("\n")[-1]),
              flush=True)
        if not ok:
            bad += 1
            sys.stderr.write(p.stderr.decode(errors="replace")[-3000:])
    print("%d of %d cases clean and equal" % (len(names) - bad, len(names)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
