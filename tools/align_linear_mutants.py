"""How much a wrong build of the "hgx" aligner on a linear index gets past the case table (tests/align_linear_cases.py).

For every one-line change listed in MUTANTS the stand-alone host program (tools/align_linear_host_main.cpp, no sanitizer) is built
from a temporary copy of csrc with that change, and run over the whole table as tools/align_linear_host_check.py runs it: bytes,
counters and the `candidates` counter against the statement.  A change that passes every case has SURVIVED: the table does not see
it.  CPU only: the core (hgx_align_linear_core.hpp) is shared by the host route and the kernels, so a change in it is tried here on
the host route; nothing changed is ever built for or run on a GPU.

    python tools/align_linear_mutants.py [--only M1,M5b] [--jobs N] [--keep DIR]
    HGX_ALIGN_LINEAR_TABLE=<another tests/ directory> python tools/align_linear_mutants.py     # the same builds against that table

Exit status 0: every listed change is killed by a case (and the unchanged build passes all of them).
"""
import argparse
import concurrent.futures
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_linear_host_check as chk          # noqa: E402

CORE, HOST = "hgx_align_linear_core.hpp", "hgx_align_linear_host.cpp"

# (id, file, the line's text, its replacement, what a build with it does wrong); each `text` stands exactly once in its file
MUTANTS = [
    ("M1", CORE, "if (pos0 < 0 || pos0 > len - L) return false;", "if (pos0 < 0) return false;",
     "reports hits whose window runs into the next allele"),
    ("M2", CORE, "if (pos0 < 0 || pos0 > len - L) return false;", "if (pos0 > len - L) return false;",
     "reports hits that start in the previous allele"),
    ("M4", CORE, "return (int32_t)((k >> 21) & 0xfffff); }", "return (int32_t)((k >> 21) & 0xffff); }",
     "wrong RNAME from allele 65 536 on"),
    ("M5", CORE, "return (int32_t)((k >> 1) & 0xfffff); }", "return (int32_t)((k >> 1) & 0xffff); }",
     "wrong POS and MD from position 65 536 on"),
    ("M5b", CORE, "return (int32_t)((k >> 1) & 0xfffff); }", "return (int32_t)((k >> 1) & 0x3ff); }",
     "wrong POS and MD from position 1 024 on"),
    ("M33", CORE, "return (int32_t)((k >> 1) & 0xfffff); }", "return (int32_t)((k >> 1) & 0x7ffff); }",
     "wrong POS in the upper half of the accepted allele length"),
    ("M13", HOST, "reads.len[first + m], max_edits, hits[m]", "reads.len[m], max_edits, hits[m]",
     "every read is aligned with the first read's (pair's) length"),
    ("M24", CORE, "return n < max_edits + 1 ? n : max_edits + 1;", "return max_edits + 1;",
     "short reads seed behind their end"),
    ("M28", HOST, "(char)toupper((unsigned char)seqs[a][k])", "seqs[a][k]",
     "lower-case allele text is never hit"),
    ("M23", CORE, "        if (s) {", "        if (s && s != 33) {",
     "wrong windows at text offset 33 (mod 64)"),
    ("M23b", CORE, "        if (s) {", "        if (s && s != 63) {",
     "wrong windows at text offset 63 (mod 64)"),
    ("M15", HOST, "P + HGX_ALNL_K <= ix->off[a + 1]; ++P", "P + HGX_ALNL_K < ix->off[a + 1]; ++P",
     "an allele's last 16-mer is not in the seed table"),
    ("M27", CORE, "if (hgx_alnl_bits16(mask, at)) return false;", "",
     "a read's N seeds as A"),
    ("M40", CORE, "if (s > 48) v |= p[q + 1] << (64 - s);", "if (s > 49) v |= p[q + 1] << (64 - s);",
     "a 16-mer at bit 49 of a plane word loses its last base"),
    ("M41", CORE, "& 0xffffu) == 0) return false;", "& 0xffffu) == 0) continue;",
     "a hit is taken from every seed that matches at it: written twice"),
    ("M42", CORE, "if (j == nw - 1 && (L & 63)) x &= (1ull << (L & 63)) - 1;", "",
     "the allele's bases behind the read's end count as mismatches"),
    ("M43", CORE, "const int nw = (L + 63) >> 6, s = (int)(P & 63);", "const int nw = (L + 64) >> 6, s = (int)(P & 63);",
     "a read of 64, 128, ... bases is compared over one word too many"),
    ("M44", HOST, "const bool mate_wrote = step == 2 && !hits[1 - m].empty();", "const bool mate_wrote = step == 2 && !hits[m].empty();",
     "flag 0x8 from the read itself, not from its mate"),
]


def changed_copy(work, mutant):
    """A copy of csrc under `work` with the mutant's line replaced."""
    mid, fname, old, new, _ = mutant
    dst = os.path.join(work, "csrc_" + mid)
    shutil.copytree(chk.CSRC, dst, ignore=shutil.ignore_patterns("*.o", "*.so", "*.hip", "*.hsaco", "build*"))
    path = os.path.join(dst, fname)
    with open(path) as f:
        text = f.read()
    if text.count(old) != 1:
        raise SystemExit("%s: its line stands %d times in %s: the list is out of date" % (mid, text.count(old), fname))
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    return dst


def failing_cases(exe, work, files):
    out = []
    for name in chk.lc.NAMES:
        why, _ = chk.run_case(exe, work, name, timeout=60, files=files[name])
        if why is not None:
            out.append("%s (%s)" % (name, why))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    todo = [m for m in MUTANTS if not a.only or m[0] in a.only.split(",")]
    files = {}
    for name in chk.lc.NAMES:                              # inputs and expectations once, shared by every build
        d = os.path.join(work, "case_" + name)
        os.makedirs(d, exist_ok=True)
        files[name] = chk.write_inputs(d, name)
        chk.expected(name)
    flags = ["-O1"]

    def one(mutant):
        exe = os.path.join(work, "main_" + (mutant[0] if mutant else "unchanged"))
        if chk.build(exe, changed_copy(work, mutant) if mutant else chk.CSRC, flags, quiet=True):
            return ["(does not build)"]
        return failing_cases(exe, work, files)
    with concurrent.futures.ThreadPoolExecutor(max(1, a.jobs)) as pool:
        results = list(pool.map(one, [None] + todo))
    print("%d cases in the table %s" % (len(chk.lc.NAMES), os.path.dirname(os.path.abspath(chk.lc.__file__))))
    print("%-5s %-9s %s" % ("unchanged", "", "passes every case" if not results[0] else "FAILS: " + ", ".join(results[0])))
    survived = []
    for mutant, failed in zip(todo, results[1:]):
        print("%-5s %-9s %s: %s\n      fails %d: %s" % (mutant[0], "killed" if failed else "SURVIVES", mutant[1], mutant[4], len(failed),
                                                       ", ".join(failed[:8]) + (", ..." if len(failed) > 8 else "")))
        if not failed:
            survived.append(mutant[0])
    print("%d of %d changes killed%s" % (len(todo) - len(survived), len(todo), "; SURVIVING: " + ", ".join(survived) if survived else ""))
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 1 if survived or results[0] else 0


if __name__ == "__main__":
    sys.exit(main())
