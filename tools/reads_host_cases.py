"""The case texts of tests/reads_table_cases.py as files for tools/reads_host_main.cpp (the sanitizer build of the read table's host
half), the program run over every case, and its output compared with the plain statement (tests/reads_table_ref.py):

    python tools/reads_host_cases.py <reads_host_main> <directory>

Every second case is written gzip-compressed.  Every FASTQ case is also run through `reads_host_main keep`: the bookkeeping of the
extractor's keep mode (host and "device" segments in mixed chunk order, an empty family, the 2 GB rule) and the loader over the
joined text.  Exit status 0: every case gave the statement's records (or, where the statement
raises, the program ended with status 1) and the sanitizers reported nothing (they end the program with a status of their own)."""
import gzip
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hisatgenotype_amd  # noqa: E402,F401
import reads_table_cases as rc  # noqa: E402
import reads_table_ref as ref  # noqa: E402


def main():
    prog, out = sys.argv[1], sys.argv[2]
    os.makedirs(out, exist_ok=True)
    bad = kept = 0
    for k, (name, case) in enumerate(rc.cases().items()):
        paths = []
        for i, t in enumerate(case.texts):
            paths.append(os.path.join(out, "%s.%d%s" % (name, i, ".gz" if k % 2 else "")))
            with open(paths[-1], "wb") as f:
                f.write(gzip.compress(t) if k % 2 else t)
        p = subprocess.run([prog, str(-1 if case.fastq is None else int(case.fastq))] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if case.error is not None:
            ok = p.returncode == 1 and ref.MESSAGES[case.error].encode() in p.stderr
        else:
            want = ref.records(case.texts, case.fastq)
            lines = [b"reads %d longest %d route 0 decline 2" % (len(want), max([len(s) for _, s, _ in want] + [0]))]
            lines += [b"\t".join((n, s, b"-" if q is None else q)) for n, s, q in want]
            lines += [b"input %d: %d bytes" % (i, len(t)) for i, t in enumerate(case.texts)]
            ok = p.returncode == 0 and p.stdout == b"".join(l + b"\n" for l in lines)
        if ok and case.fastq is not False and not any(t[:1] == b">" for t in case.texts) and any(case.texts):
            # the keep mode's bookkeeping over the same files (the extractor writes FASTQ or FASTA as told: fastq = 1 here)
            kp = subprocess.run([prog, "keep", "1"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            fq_error = case.error
            try:
                ref.records(case.texts, True)
            except ref.ReadsError as e:
                fq_error = e.kind
            else:
                fq_error = None
            if fq_error is not None:
                ok = kp.returncode == 1 and ref.MESSAGES[fq_error].encode() in kp.stderr
            else:
                want = ref.records(case.texts, True)
                lines = [b"reads %d longest %d route 0 decline 2" % (len(want), max([len(s) for _, s, _ in want] + [0]))]
                lines += [b"\t".join((n, s, b"-" if q is None else q)) for n, s, q in want]
                lines += [b"input %d: %d bytes" % (i, len(t)) for i, t in enumerate(case.texts)]
                ok = kp.returncode == 0 and kp.stdout == b"".join(l + b"\n" for l in lines)
            kept += 1
            if not ok:
                p = kp
        if not ok:
            bad += 1
            print("FAILED %s: status %d\n%s" % (name, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    print("%d cases (%d of them through the keep mode as well), %d failed" % (len(rc.cases()), kept, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
