"""Read extraction: stage 1 of a real-data run (hisatgenotype_typing_process.extract_reads, process:1330-1784).

The aligner's SAM stream over the whole genotype genome (or a BAM file of it, fed as deflated bytes) goes through the library's extraction handle (include/hgx.h "read
extraction": record pass, grouping, family decision and FASTQ / FASTA text as gfx950 kernels, csrc/hgx_extract.hip); this module
keeps the reference's file discovery, file names, "Files found: Omitted" rule and return value, starts the aligner with the
reference's command line when no alignment file is given, and compresses the text it takes from the library on host threads."""
import ctypes as C
import glob
import gzip
import os
import subprocess
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import capi

ALIGNER_CODE = {"hisat2": 0, "bowtie2": 1}
ERRORS = {1: ValueError, 2: AssertionError, 3: SystemExit, 4: IndexError, 5: TypeError}
FEED_BYTES = 64 << 20            # the aligner's stdout is read in blocks of this size


class ExtractOpts(C.Structure):
    _fields_ = [("aligner", C.c_int32), ("paired", C.c_int32), ("simulation", C.c_int32), ("fastq", C.c_int32)]


def read_locus_table(path, database_list):
    """The region table of process:1364-1380: [(family lower, chromosome, left, right)] in file order, filtered by database_list,
    which gets the families met appended in place."""
    filter_region = len(database_list) > 0
    regions, names = [], set()
    for line in open(path):
        family, allele_name, chrom, left, right = line.strip().split()[:5]
        if filter_region and family.lower() not in database_list:
            continue
        region_name = "%s-%s" % (family, allele_name.split('*')[0])
        assert region_name not in names
        names.add(region_name)
        regions.append((family.lower(), chrom, int(left), int(right)))
        if family.lower() not in database_list:
            database_list.append(family.lower())
    return regions


class Extractor:
    """One sample's stream: feed() bytes, take() the text per family and mate.  keep=True: the text stays where the chunks' routes
    made it (a device chunk's in HBM) and take_reads(family) hands it to the aligner as an engine.Reads; take() then raises."""

    def __init__(self, regions, families, aligner, paired, simulation, fastq, stream=None, keep=False):
        self.families = list(families)
        self.paired = bool(paired)
        fam_ix = {f: i for i, f in enumerate(self.families)}
        regions = [r for r in regions if r[0] in fam_ix]
        fam = np.array([fam_ix[r[0]] for r in regions], np.int32)
        pool = b"".join(r[1].encode() + b"\0" for r in regions)
        left = np.array([r[2] for r in regions], np.int64)
        right = np.array([r[3] for r in regions], np.int64)
        opts = ExtractOpts(ALIGNER_CODE.get(aligner, 2), int(bool(paired)), int(bool(simulation)), int(bool(fastq)))
        self.h = C.c_void_p()
        self.stream = stream
        capi.check(capi.lib().hgx_extract_open(C.byref(self.h), C.c_int32(len(regions)), capi.ptr(fam), C.c_char_p(pool),
                                               C.c_size_t(len(pool)), capi.ptr(left), capi.ptr(right), C.c_int32(len(self.families)),
                                               C.byref(opts)))
        self.keep = bool(keep)
        if self.keep:
            capi.check(capi.lib().hgx_extract_keep(self.h, C.c_int32(1)))

    def _raise(self, rc):
        if rc == 0:
            return
        kind = self.stats()["error_kind"]
        msg = capi.lib().hgx_last_error().decode(errors="replace")
        if kind == 3:
            print("Error: Paired read names are not the same", file=sys.stderr)
            raise SystemExit(1)
        if kind in ERRORS:
            raise ERRORS[kind](msg)
        capi.check(rc)

    def feed(self, data, last=False):
        self._raise(capi.lib().hgx_extract_feed(self.h, C.c_char_p(data) if isinstance(data, bytes) else capi.ptr(data),
                                                C.c_size_t(len(data)), C.c_int32(1 if last else 0), self.stream))

    def feed_bam(self, data, last=False):
        """The next bytes of a BAM file (its BGZF container), cut anywhere."""
        self._raise(capi.lib().hgx_extract_feed_bam(self.h, C.c_char_p(data) if isinstance(data, bytes) else capi.ptr(data),
                                                    C.c_size_t(len(data)), C.c_int32(1 if last else 0), self.stream))

    def feed_file(self, path):
        self._raise(capi.lib().hgx_extract_file(self.h, C.c_char_p(os.fsencode(path)), self.stream))

    def take(self, family, mate):
        p, n = C.c_void_p(), C.c_size_t(0)
        capi.check(capi.lib().hgx_extract_take(self.h, C.c_int32(family), C.c_int32(mate), C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def take_reads(self, family):
        """The reads of `family` kept since the last call, both mates, as an engine.Reads (hgx_extract_take_reads)."""
        from . import engine
        h = C.c_void_p()
        capi.check(capi.lib().hgx_extract_take_reads(self.h, C.c_int32(family), C.byref(h)))
        return engine.Reads.from_handle(h)

    def stats(self):
        rec, grp, ck_d, ck_h = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        route, dec, kind = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        written = np.zeros(max(len(self.families), 1), np.int64)
        capi.check(capi.lib().hgx_extract_stats(self.h, C.byref(rec), C.byref(grp), capi.ptr(written), C.byref(route), C.byref(dec),
                                                C.byref(kind), C.byref(ck_d), C.byref(ck_h)))
        return {"records": rec.value, "groups": grp.value, "written": {f: int(written[i]) for i, f in enumerate(self.families)},
                "route": route.value, "decline": dec.value, "error_kind": kind.value, "chunks_device": ck_d.value,
                "chunks_host": ck_h.value}

    def close(self):
        if self.h:
            capi.lib().hgx_extract_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


last_stats = None        # stats of the last sample extract_reads ran (tests, tools)


def get_filename_match(fns):
    """typing_common.get_filename_match (common:644-687) without its prompt: the common stem of each consecutive file pair."""
    fnames, fnames2, fnbase = [], [], []
    for i in range(0, len(fns), 2):
        file_l, file_r = fns[i:i + 2]
        common = ''
        for j in range(len(file_l)):
            s = file_l[j]
            if s != file_r[j]:
                if s not in "LR12":
                    print("Potential Error: Paired-end mode is selected and files %s and %s have an unexpected character %s to mark "
                          "left and right pairings" % (file_l, file_r, s))
                if common[-1] in "._-":
                    common = common[:-1]
                break
            common += s
        if not common:
            print("Error matching files %s and %s. Names don't match. Skipping inclusion" % (file_l, file_r))
            continue
        fnames.append(file_l)
        fnames2.append(file_r)
        fnbase.append(common)
    return fnames, fnames2, fnbase


def check_base(base_fname, aligner, ix_dir="."):
    """typing_common.check_base (common:87-109)."""
    full = ix_dir + "/" + base_fname
    names = ["%s.%s" % (full, e) for e in ("fa", "locus", "snp", "haplotype", "link", "coord", "clnsig")]
    if aligner == "hisat2":
        names += ["%s.%d.ht2" % (full, i + 1) for i in range(8)]
    else:
        assert aligner == "bowtie2"
        names = ["%s.%d.bt2" % (full, i + 1) for i in range(4)] + ["%s.rev.%d.bt2" % (full, i + 1) for i in range(2)]
    ok = True
    for fname in names:
        if not os.path.exists(fname):
            print("No %s file found" % fname, file=sys.stderr)
            ok = False
    if not ok:
        print("Error: %s related files are missing in %s!" % (base_fname, ix_dir), file=sys.stderr)
    return ok


def aligner_command(aligner, base_filepath, fastq, paired, threads_aprocess, fq_fname, fq_fname2):
    """The command line of process:1468-1488."""
    cmd = [aligner]
    if threads_aprocess > 1:
        cmd += ["-p", "%d" % threads_aprocess]
    if not fastq:
        cmd += ["-f"]
    cmd += ["-x", base_filepath]
    if aligner == "hisat2":
        cmd += ["--no-spliced-alignment"]
    cmd += ["-X", "1000"]
    if paired:
        cmd += ["-1", fq_fname, "-2", fq_fname2]
    else:
        cmd += ["-U", fq_fname]
    return cmd


def is_bam(path):
    """A BGZF file (magic 1f 8b) whose inflated bytes start with a BAM header's magic; a bgzipped SAM text is not."""
    with open(path, "rb") as f:
        if f.read(2) != b"\x1f\x8b":
            return False
    try:
        with gzip.open(path, "rb") as g:
            return g.read(4) == b"BAM\x01"
    except (OSError, EOFError, zlib.error):
        return True          # a damaged container: the BAM reader words the error


def _out_names(out_dir, base, database, paired):
    if paired:
        return ["%s%s-%s-extracted-1.fq.gz" % (out_dir, base, database), "%s%s-%s-extracted-2.fq.gz" % (out_dir, base, database)]
    return ["%s%s-%s-extracted.fq.gz" % (out_dir, base, database)]


def _gzip_member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def _work(ex, files, pool, source, verbose):
    """Feed the stream, and after every feed write what is ready: one gzip member per taken block (concatenated members are a valid
    .gz; the contract is the decompressed bytes)."""
    n_mates = 2 if ex.paired else 1

    wrote = set()

    def drain():
        jobs = []
        for f in range(len(ex.families)):
            for m in range(n_mates):
                data = ex.take(f, m)
                if data:
                    wrote.add((f, m))
                    jobs.append((files[f][m], pool.submit(_gzip_member, data)))
        for fh, job in jobs:
            fh.write(job.result())

    try:
        source(ex, drain)
    finally:
        drain()                      # the files hold what was written before an error
        for f in range(len(ex.families)):
            for m in range(n_mates):
                if (f, m) not in wrote:
                    files[f][m].write(_gzip_member(b""))


def extract_reads(base_fname, ix_dir, database_list, read_dir, out_dir, suffix, read_fname, fastq, paired, simulation, threads,
                  threads_aprocess, max_sample, job_range, aligner, block_size, verbose, alignment_fname=None):
    """extract_reads of the reference (process:1330-1784): the same 17 positional parameters, file names and return value
    (fname_list).  alignment_fname (a path, or {sample base name: path}) names a SAM / BAM file that is the record stream of the
    sample instead of a run of the aligner."""
    global last_stats
    if block_size > 0:
        raise NotImplementedError("--extract-whole (block_size > 0) is not built: the reference itself raises TypeError there under "
                                  "Python 3 (range() of a float, process:1549-1556)")
    run_aligner = alignment_fname is None
    if run_aligner and not check_base(base_fname, aligner, ix_dir):
        raise SystemExit(1)
    base_filepath = ix_dir + "/" + base_fname
    fname_list = {}
    regions = read_locus_table("%s.locus" % base_filepath, database_list)

    if out_dir != "":
        if not os.path.exists(out_dir):
            os.mkdir(out_dir)
        out_dir = out_dir if out_dir.endswith("/") else out_dir + "/"
    else:
        out_dir = "./"

    if len(read_fname) > 0:
        if paired:
            fq_fnames, fq_fnames2 = [read_fname[0]], [read_fname[1]]
        else:
            fq_fnames = read_fname
    else:
        fq_fnames = sorted(glob.glob("%s/*.%s" % (read_dir, suffix)))
        if paired:
            fq_fnames, fq_fnames2, paired_fq_basen = get_filename_match(fq_fnames)
        if len(fq_fnames) == 0:
            print("Error: no files identified in %s directory with suffix .%s" % (read_dir, suffix), file=sys.stderr)
            raise SystemExit(1)

    count = 0
    with ThreadPoolExecutor(max_workers=max(1, min(int(threads), 16))) as pool:
        for file_i in range(len(fq_fnames)):
            if file_i >= max_sample:
                break
            fq_fname = fq_fnames[file_i]
            if job_range[1] > 1 and job_range[0] != (file_i % job_range[1]):
                continue
            if paired:
                fq_fname_base = fq_fname.split('/')[-1] if len(read_fname) > 0 else paired_fq_basen[file_i].split('/')[-1]
            else:
                fq_fname_base = fq_fname.split('/')[-1].split('.')[0]
            if paired:
                fq_fname2 = fq_fnames2[file_i]
                if run_aligner and not os.path.exists(fq_fname2):
                    print("%s does not exist." % fq_fname2, file=sys.stderr)
                    continue
            else:
                fq_fname2 = ""

            omit_extract = True
            for database in database_list:
                fname_list.setdefault(database, []).append('%s-%s' % (fq_fname_base, database))
                if paired and os.path.exists("%s%s-%s-extracted-1.fq.gz" % (out_dir, fq_fname_base, database)):
                    continue
                elif os.path.exists("%s%s-%s-extracted.fq.gz" % (out_dir, fq_fname_base, database)):
                    continue
                omit_extract = False
            if omit_extract:
                print("\tFiles found: Omitted extracting reads from %s" % fq_fname_base, file=sys.stderr)
                continue

            count += 1
            print("\t%d: Extracting reads from %s" % (count, fq_fname_base), file=sys.stderr)

            if run_aligner:
                cmd = aligner_command(aligner, base_filepath, fastq, paired, threads_aprocess, fq_fname, fq_fname2)
                if verbose:
                    print("\t\trunning", ' '.join(cmd), file=sys.stderr)

                def source(ex, drain, cmd=cmd):
                    try:
                        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
                    except FileNotFoundError:
                        raise FileNotFoundError("the aligner executable %r is not on PATH" % cmd[0]) from None
                    try:
                        while True:
                            block = proc.stdout.read(FEED_BYTES)
                            if not block:
                                break
                            ex.feed(block)
                            drain()
                        ex.feed(b"", last=True)
                    finally:
                        proc.stdout.close()
                        proc.wait()
            else:
                if isinstance(alignment_fname, dict):
                    path = alignment_fname[fq_fname_base]
                else:
                    path = alignment_fname

                if is_bam(path):
                    def source(ex, drain, path=path):
                        # the file's deflated bytes block by block: what is ready is compressed and written while the file is read
                        with open(path, "rb") as f:
                            block = f.read(FEED_BYTES)
                            while True:
                                nxt = f.read(FEED_BYTES)
                                ex.feed_bam(block, last=not nxt)
                                drain()
                                if not nxt:
                                    break
                                block = nxt
                else:
                    def source(ex, drain, path=path):
                        ex.feed_file(path)

            ex = Extractor(regions, database_list, aligner, paired, simulation, fastq)
            files = [[open(n, "wb") for n in _out_names(out_dir, fq_fname_base, database, paired)] for database in database_list]
            try:
                _work(ex, files, pool, source, verbose)
            finally:
                for fs in files:
                    for fh in fs:
                        fh.close()
                last_stats = ex.stats()
                ex.close()
    return fname_list


def extract_reads_resident(base_fname, ix_dir, database_list, alignment_fname, fastq, paired, simulation, aligner, stream=None):
    """One sample's genome-wide alignment stream -> {database: engine.Reads}, no file in between: the extractor keeps each family's
    FASTA / FASTQ text in HBM (Extractor(keep=True)) and the aligner's read table is made over it where it lies.
    alignment_fname: a SAM / BAM path, or an open binary pipe of SAM text read in FEED_BYTES blocks.  database_list is filtered and
    extended as extract_reads does it.  The objects go to typing_options.reads (one family per typing() call); close() them."""
    global last_stats
    regions = read_locus_table("%s/%s.locus" % (ix_dir, base_fname), database_list)
    ex = Extractor(regions, database_list, aligner, paired, simulation, fastq, stream=stream, keep=True)
    try:
        if isinstance(alignment_fname, (str, bytes, os.PathLike)):
            path = os.fspath(alignment_fname)
            if is_bam(path):
                with open(path, "rb") as f:
                    block = f.read(FEED_BYTES)
                    while True:
                        nxt = f.read(FEED_BYTES)
                        ex.feed_bam(block, last=not nxt)
                        if not nxt:
                            break
                        block = nxt
            else:
                ex.feed_file(path)
        else:
            while True:
                block = alignment_fname.read(FEED_BYTES)
                if not block:
                    break
                ex.feed(block)
            ex.feed(b"", last=True)
        out = {}
        try:
            for f, database in enumerate(database_list):
                out[database] = ex.take_reads(f)
        except BaseException:
            for r in out.values():
                r.close()
            raise
        return out
    finally:
        last_stats = ex.stats()
        ex.close()


def synth_stream(n_pairs, regions, seed=1, hit_fraction=0.015, read_len=100, chroms=None):
    """A seeded paired-end HISAT2-like SAM stream for tests and timing: most pairs outside every region, `hit_fraction` of them
    inside one, a few unmapped pairs, secondary records and reverse strands.  -> bytes."""
    rng = np.random.default_rng(seed)
    chroms = chroms or [str(i + 1) for i in range(22)] + ["X"]
    bases = np.frombuffer(b"ACGT", np.uint8)
    seqs = bases[rng.integers(0, 4, size=(2 * n_pairs, read_len))]
    quals = (rng.integers(0, 40, size=(2 * n_pairs, read_len)) + 35).astype(np.uint8)
    u = rng.random(n_pairs)
    out = []
    for g in range(n_pairs):
        name = "read%09d" % g
        s1, s2 = seqs[2 * g].tobytes().decode(), seqs[2 * g + 1].tobytes().decode()
        q1, q2 = quals[2 * g].tobytes().decode(), quals[2 * g + 1].tobytes().decode()
        if u[g] < hit_fraction and regions:
            _, c, left, right = regions[int(rng.integers(0, len(regions)))]
            p = int(rng.integers(left + 1, max(right, left + 2)))
        else:
            c, p = chroms[int(rng.integers(0, len(chroms)))], int(rng.integers(10_000_000, 90_000_000))
        if u[g] > 0.97:
            out.append("%s\t77\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tYT:Z:UP\n%s\t141\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tYT:Z:UP\n" % (name, s1, q1, name, s2, q2))
            continue
        nh = 1 if rng.random() < 0.85 else int(rng.integers(2, 6))
        f1 = 0x43 | (0x10 if rng.random() < 0.5 else 0x20)
        f2 = 0x83 | (0x20 if f1 & 0x10 else 0x10)
        tl = int(rng.integers(150, 500))
        tags = "AS:i:%d\tZS:i:-12\tXN:i:0\tXM:i:1\tXO:i:0\tXG:i:0\tNM:i:1\tYS:i:0\tYT:Z:CP\tNH:i:%d" % (-int(rng.integers(0, 9)), nh)
        out.append("%s\t%d\t%s\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\t%s\n" % (name, f1, c, p, read_len, p + tl, tl, s1, q1, tags))
        if nh > 1 and rng.random() < 0.5:
            out.append("%s\t%d\t%s\t%d\t1\t%dM\t=\t%d\t%d\t%s\t%s\t%s\n" % (name, f1 | 0x100, chroms[int(rng.integers(0, len(chroms)))],
                                                                          int(rng.integers(1, 9_000_000)), read_len, p, tl, s1, q1, tags))
        out.append("%s\t%d\t%s\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\t%s\n" % (name, f2, c, p + tl, read_len, p, -tl, s2, q2, tags))
    return "".join(out).encode()
