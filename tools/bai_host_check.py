"""The index reader under AddressSanitizer and UBSan, as a stand-alone host program (no GPU, not through python's process):
builds tools/bai_host_check.cpp with -fsanitize=address,undefined, writes the test fixture BAM and its index, and runs the program over
every prefix of the index and over copies with one byte changed.  Usage: tools/bai_host_check.py [block size]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hisatgenotype_amd  # noqa: E402,F401
import bai_cases  # noqa: E402
import bai_ref  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    exe = os.path.join(d, "bai_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DHGX_BAI_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hisat-genotype_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bai_host_check.cpp"), "-o", exe])
    bam = bai_cases.write_fixture(d, int(sys.argv[1]) if len(sys.argv) > 1 else 700)
    bai = bam + ".bai"
    with open(bai, "wb") as f:
        f.write(bai_ref.build(bam))
    subprocess.check_call([exe, bai, str(os.path.getsize(bam)), str(len(bai_cases.REFS))])
