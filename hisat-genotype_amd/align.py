"""The "hgx" aligner: reads that belong to a locus family, aligned to the backbones in `Genes` through the known
variants in `Vars` -- end to end, at most `max_edits` unknown mismatches, known variants free -- and written as SAM text in the
dialect the front end consumes (NM, MD, Zs, NH, YT as simulate._truth_record renders them).

It is NOT HISAT2 and its output is not compared with HISAT2's anywhere: no whole-genome index, no secondary records; mates placed
independently unless pair="aware" (tests/align_pair_ref.py); soft clips only with clip=N, and only for a read that has no
end-to-end alignment (tests/align_clip_ref.py); a novel indel only with gap=N, one per read, and only for a read that has no
end-to-end alignment (tests/align_gap_ref.py); both of these in one call, the cheaper rescue per read, only with rescue=(G, C)
(tests/align_rescue_ref.py).  The rules are stated in plain Python in tests/align_ref.py; the kernels
(csrc/hgx_align.hip) and the host route (csrc/hgx_align_host.cpp) run one shared core (csrc/hgx_align_core.hpp, and csrc/hgx_align_states.hpp for the search over states).

LinearAlignIndex is the same family's aligner on a LINEAR index: the reads against the loci's ALLELE SEQUENCES,
ungapped, end to end, at most `max_edits` mismatches, up to `k` records per read -- what the linear typing (typing.type_locus_linear)
groups by read.  It is NOT HISAT2 or Bowtie2 either, and its output is compared with neither: no gaps, clips or splices, mates
placed independently, RNEXT / PNEXT / TLEN left empty on purpose (the linear branch reads none of them).  The rule is stated in plain
Python in tests/align_linear_ref.py; the kernels (csrc/hgx_align_linear.hip) and the host route (csrc/hgx_align_linear_host.cpp) run
one shared core (csrc/hgx_align_linear_core.hpp).
"""
import ctypes as C

from . import capi

_TYPES = {"insertion": capi.VAR_INSERTION, "single": capi.VAR_SINGLE, "deletion": capi.VAR_DELETION}
ROUTES = {"auto": 0, "host": 1, "device": 2}
SEARCHES = {"ways": 0, "states": 1, "states_all": 2}
PAIRS = {"independent": 0, "aware": 1}
NAMED_CLIP = 32                      # the clip budget of the aligner name "hgx.clip"
CLIP_MAX, CLIP_MAX_EDITS = 255, 4    # HGX_ALN_CLIP_MAX, HGX_ALN_CLIP_EDITS of csrc/hgx_align_core.hpp
NAMED_GAP = 16                       # the longest novel gap of the aligner name "hgx.gap"
GAP_MAX = 16                         # HGX_ALN_GAP_MAX of include/hgx.h
NAMED_RESCUE = (NAMED_GAP, NAMED_CLIP)   # (gap, clip) of the aligner name "hgx.rescue"


class AlignOpts(C.Structure):
    _fields_ = [("max_edits", C.c_int32), ("max_fragment", C.c_int32), ("fastq", C.c_int32), ("route", C.c_int32),
                ("search", C.c_int32), ("pair", C.c_int32), ("clip", C.c_int32)]


class AlignMore(C.Structure):
    """hgx_align_more: the options behind hgx_align_opts (which keeps its seven words); `bytes` = sizeof."""
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32)]


class AlignMoreRescue(C.Structure):
    """hgx_align_more with its third word (12 bytes): passed only where rescue= is given; AlignMore stays the 8-byte first version."""
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("rescue_clip", C.c_int32)]


class AlignMoreOrder(C.Structure):
    """hgx_align_more with its fourth word (16 bytes): passed only where order="coordinate" or align_resident() is asked for."""
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("rescue_clip", C.c_int32), ("order", C.c_int32)]


ORDERS = {"read": 0, "coordinate": 1}


class AlignIndex:
    """The loci of `Genes` (in its order) with their variants in `Var_list` order, ready for align()."""

    def __init__(self, Genes, Vars, Var_list, refGenes):
        names, bbs, off, vtype, vpos, vdata, vid = [], [], [0], [], [], [], []
        for g in Genes:
            names.append(refGenes[g].encode())
            bbs.append(Genes[g][refGenes[g]].encode())
            gv = Vars.get(g, {})
            for _, v in Var_list.get(g, []):
                t, p, d = gv[v][:3]
                vtype.append(_TYPES[t])
                vpos.append(int(p))
                vdata.append(str(d).encode())
                vid.append(v.encode())
            off.append(len(vtype))
        n = len(vtype)
        self.n_loci = len(names)
        self.h = C.c_void_p()
        capi.check(capi.lib().hgx_align_index_create(
            C.byref(self.h), C.c_int32(self.n_loci), (C.c_char_p * len(names))(*names), (C.c_char_p * len(bbs))(*bbs),
            (C.c_int32 * len(off))(*off), (C.c_int32 * max(n, 1))(*vtype), (C.c_int32 * max(n, 1))(*vpos),
            (C.c_char_p * max(n, 1))(*vdata), (C.c_char_p * max(n, 1))(*vid)))

    @staticmethod
    def _call_args(reads, max_edits, max_fragment, fastq, route, search, pair, clip, gap, rescue, order):
        """(opts, more, n, paths, texts, sizes, what keeps them alive) of one hgx_align_reads_x / hgx_align_reads_resident call;
        `reads` an engine.Reads: (opts, more, None, None, None, None, reads) of one hgx_align_reads_dev / _dev_resident call."""
        made = hasattr(reads, "n_reads")
        assert made or len(reads) in (1, 2)
        opts = AlignOpts(int(max_edits), int(max_fragment), -1 if fastq is None else int(bool(fastq)), ROUTES[route],
                         search if isinstance(search, int) else SEARCHES[search], pair if isinstance(pair, int) else PAIRS[pair], int(clip))
        order = order if isinstance(order, int) else ORDERS[order]
        if rescue is not None and gap:
            raise ValueError("rescue=(G, C) names the gap tier's budget itself: gap= stays 0")
        if order:
            more = AlignMoreOrder(C.sizeof(AlignMoreOrder), int(rescue[0] if rescue is not None else gap),
                                  int(rescue[1]) if rescue is not None else 0, order)
        elif rescue is None:
            more = AlignMore(C.sizeof(AlignMore), int(gap))
        else:
            more = AlignMoreRescue(C.sizeof(AlignMoreRescue), int(rescue[0]), int(rescue[1]))
        if made:
            return opts, more, None, None, None, None, reads
        if all(isinstance(r, str) for r in reads):
            paths = (C.c_char_p * len(reads))(*[r.encode() for r in reads])
            return opts, more, C.c_int32(len(reads)), paths, None, None, None
        bufs = [bytes(r) for r in reads]
        texts = (C.c_char_p * len(bufs))(*bufs)
        sizes = (C.c_size_t * len(bufs))(*[len(b) for b in bufs])
        return opts, more, C.c_int32(len(bufs)), None, texts, sizes, bufs

    def align_resident(self, reads, max_edits=2, max_fragment=1000, fastq=None, route="auto", search="ways", pair="independent",
                       clip=0, gap=0, rescue=None, stream=None):
        """align(..., order="coordinate") whose text is NOT copied back: an engine.Alignment over the ordered text in HBM
        (hgx_align_reads_resident), ready for parse_dev(locus, regions) per locus -- what the coordinate-sorted BAM between aligner
        and front end gave them, without the file.  `.text()` copies the text back, `.save(path)` writes that BAM; `.close()` frees
        it (and removes the temporary BAM a per-path fallback may have written).  align_last() reports as for align()."""
        from . import engine
        opts, more, n, paths, texts, sizes, _keep = self._call_args(reads, max_edits, max_fragment, fastq, route, search, pair, clip, gap,
                                                                    rescue, "coordinate")
        h = C.c_void_p()
        if n is None:                            # an engine.Reads: the loading step is the object
            capi.check(capi.lib().hgx_align_reads_dev_resident(self.h, _keep.h, C.byref(opts), C.byref(more), C.byref(h), stream))
        else:
            capi.check(capi.lib().hgx_align_reads_resident(self.h, n, paths, texts, sizes, C.byref(opts), C.byref(more), C.byref(h), stream))
        return engine.Alignment.from_handle(h)

    def align(self, reads, max_edits=2, max_fragment=1000, fastq=None, route="auto", search="ways", pair="independent",
              clip=0, gap=0, rescue=None, order="read"):
        """SAM text (bytes) for `reads` = one or two FASTA / FASTQ[.gz] paths (str) or in-memory texts (bytes), or an engine.Reads
        made of them beforehand (its table is read where it lies; `fastq` is then not looked at).  `search`: "ways"
        (per anchor, the ways through the known indels), "states" (reads that pass the kernels' anchor slots, stack or step limit
        -- on the host route: every read -- are searched over (read base, backbone position) states instead), "states_all" (every
        read is); an int is passed through as hgx_align_opts.search.  The bytes are the same.  `pair`: "independent" (each mate's
        smallest alignment, as before) or "aware" (where a combination of the mates' candidates is concordant, both records come
        from the smallest such combination and NH counts the pair's placements: tests/align_pair_ref.py); an int is passed
        through as hgx_align_opts.pair.  "aware" needs search="ways".  `clip`: 0 (end to end only, every byte as before) or N <= 255:
        a read WITHOUT an end-to-end alignment may be written with up to N bases soft-clipped in total (an overhang over a backbone
        end, a tail that does not match), by the order (clipped bases, then the usual key) of tests/align_clip_ref.py; a read that
        aligns end to end is written as with 0, except for the mate fields of a record whose mate is aligned only now.  Needs
        search="ways", pair="independent" and max_edits <= 4.  `gap`: 0 (no novel indels, every byte as before) or N <= 16: a read
        WITHOUT an end-to-end alignment may be written with ONE novel deletion of up to N backbone bases or insertion of up to N read
        bases, its length counted into NM <= max_edits, by the order of tests/align_gap_ref.py (the usual key, then the leftmost
        gap); a read that aligns end to end is written as with 0, except for the mate fields of a record whose mate is aligned only
        now.  Needs search="ways", pair="independent" and clip=0.  `rescue`: None, or (G, C) = both tiers in one call, the gap tier with
        gap=G and the clip tier with clip=C: a read WITHOUT an end-to-end alignment is written from the clip tier's result unless the
        gap tier's costs fewer read bases given up or edited (NM with the gap counted < clipped bases + NM of the clipped record; a
        tie goes to the clip), by tests/align_rescue_ref.py; no record carries both.  Needs search="ways", pair="independent",
        max_edits <= 4, and gap=0 and clip=0 (they stay mutually exclusive and keep their meaning).  `order`: "read" (the records in
        input order, mate 1 before mate 2: the 8- and 12-byte hgx_align_more are passed as before) or "coordinate" (stable-sorted by
        (locus in @SQ order, POS), the order of the BAM that simulate._store_as_the_reference_does writes:
        tests/align_resident_ref.py); an int is passed through as hgx_align_more.order.  Valid with every form above."""
        opts, more, n_in, paths, texts, sizes, _keep = self._call_args(reads, max_edits, max_fragment, fastq, route, search, pair, clip, gap,
                                                                       rescue, order)
        out_p, n = C.c_void_p(), C.c_size_t(0)
        if n_in is None:                         # an engine.Reads: the loading step is the object
            rc = capi.lib().hgx_align_reads_dev(self.h, _keep.h, C.byref(opts), C.byref(more), C.byref(out_p), C.byref(n))
        else:
            rc = capi.lib().hgx_align_reads_x(self.h, n_in, paths, texts, sizes, C.byref(opts), C.byref(more), C.byref(out_p), C.byref(n))
        capi.check(rc)
        try:
            return C.string_at(out_p.value, n.value)
        finally:
            capi.lib().hgx_free_text(out_p)

    def close(self):
        if self.h:
            capi.lib().hgx_align_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align_last():
    """dict(route, reads, aligned, pairs_concordant, decline, states_reads, states_anchors, states_cells) of the calling thread's
    last align(): route 2 = the kernels, 0 = the host route (decline says why: HGX_ALN_DECLINE_* of csrc/hgx_align_core.hpp and
    hgx_align_states.hpp); states_* = the reads, anchors and table cells the states search took on that route; pairs_searched /
    pairs_placed / pairs_changed (pair="aware") = pairs with candidates on both mates, with a concordant combination, and with a
    record that differs from the independent one in alignment or NH; clip_searched / clip_clipped / clip_bases (clip=N) = reads
    without an end-to-end alignment that the clip tier searched, reads written with a clip, bases clipped; gap_searched /
    gap_gapped / gap_bases (gap=N) = the same of the gap tier: reads searched, reads written with a novel gap, gap bases.  With
    rescue=(G, C) both groups are set: clip_searched = reads without an end-to-end alignment that have an anchor, gap_searched =
    those of them the clip tier left unaligned or with a cost of 2 or more; clipped / gapped and bases = the reads WRITTEN so."""
    route, dec = C.c_int32(0), C.c_int32(0)
    reads, aligned, conc = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_last(C.byref(route), C.byref(reads), C.byref(aligned), C.byref(conc), C.byref(dec)))
    sr, sa, sc = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_last_states(C.byref(sr), C.byref(sa), C.byref(sc)))
    ps, pp, pc = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_last_pairs(C.byref(ps), C.byref(pp), C.byref(pc)))
    cs, cc, cb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_last_clip(C.byref(cs), C.byref(cc), C.byref(cb)))
    gs, gg, gb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_last_gap(C.byref(gs), C.byref(gg), C.byref(gb)))
    return dict(route=route.value, reads=reads.value, aligned=aligned.value, pairs_concordant=conc.value, decline=dec.value,
                states_reads=sr.value, states_anchors=sa.value, states_cells=sc.value,
                pairs_searched=ps.value, pairs_placed=pp.value, pairs_changed=pc.value,
                clip_searched=cs.value, clip_clipped=cc.value, clip_bases=cb.value,
                gap_searched=gs.value, gap_gapped=gg.value, gap_bases=gb.value)


def align_last_clip():
    """(searched, clipped, bases) of hgx_align_last_clip for the calling thread's last align()."""
    last = align_last()
    return last["clip_searched"], last["clip_clipped"], last["clip_bases"]


def align_last_gap():
    """(searched, gapped, bases) of hgx_align_last_gap for the calling thread's last align()."""
    last = align_last()
    return last["gap_searched"], last["gap_gapped"], last["gap_bases"]


DECLINE_GATE, DECLINE_READ_LEN, DECLINE_ANCHORS, DECLINE_STACK, DECLINE_VARS, DECLINE_STEPS, DECLINE_SWITCH = 1, 2, 3, 4, 5, 6, 7
DECLINE_WINDOW = 8

# the read table made on the device (engine.Reads): HGX_RD_TILE, HGX_RD_GATE and HGX_RD_DECLINE_* of csrc/hgx_reads.hpp
READS_TILE = 4096                    # bytes per tile of the newline pass
READS_GATE = 512 << 10               # bytes of inflated text from which the kernels make the table (the measured break-even, rounded up)
READS_MAX_BYTES = (1 << 32) - 64     # padded text from which the table declines with SIZE (test switch reads_max_bytes=N: another)
(READS_DECLINE_GATE, READS_DECLINE_SWITCH, READS_DECLINE_EMPTY_LINE, READS_DECLINE_MARKER, READS_DECLINE_TRUNCATED, READS_DECLINE_QUAL_LEN,
 READS_DECLINE_LOWER, READS_DECLINE_COUNT, READS_DECLINE_READ_LEN, READS_DECLINE_SIZE) = range(1, 11)
MAX_READ = 1024                      # HGX_ALN_MAX_READ of csrc/hgx_align_core.hpp
STATES_MAX_WINDOW, STATES_MARGIN = 8192, 128      # HGX_ALN_STATES_MAX_WINDOW, HGX_ALN_STATES_MARGIN of csrc/hgx_align_states.hpp

_INDEX_CACHE = []          # [(Genes, Vars, Var_list, refGenes, AlignIndex)]: typing() runs once per sample on the same dicts


def cached_index(Genes, Vars, Var_list, refGenes):
    """The index of these dicts, found again by the IDENTITY of the four dict objects only (the packed-locus cache also keeps a
    content key; this one does not): dicts edited in place after the first call return the index of their old content, and dicts
    re-read from the index files (every genotyping_locus call) miss, so the index is built and uploaded again -- 3 ms for a
    six-locus panel.  Callers that edit their dicts build an AlignIndex themselves."""
    for g, v, vl, rg, ix in _INDEX_CACHE:
        if g is Genes and v is Vars and vl is Var_list and rg is refGenes:
            return ix
    ix = AlignIndex(Genes, Vars, Var_list, refGenes)
    _INDEX_CACHE.append((Genes, Vars, Var_list, refGenes, ix))
    del _INDEX_CACHE[:-4]
    return ix


# ---- the linear index -----------------------------------------------------------------------------------------------
LINEAR_MAX_EDITS, LINEAR_MAX_K = 4, 1024         # HGX_ALNL_MAX_EDITS, HGX_ALNL_MAX_K of csrc/hgx_align_linear_core.hpp
LINEAR_DEV_MAX_READ = 256                        # HGX_ALNL_DEV_MAX_READ: a longer read declines the kernels' route
(LINEAR_DECLINE_GATE, LINEAR_DECLINE_READ_LEN, LINEAR_DECLINE_BUDGET, LINEAR_DECLINE_LINE) = 1, 2, 3, 4      # HGX_ALNL_DECLINE_*
LINEAR_DECLINE_SWITCH = 7
LINEAR_GATE = 16384                              # HGX_ALNL_GATE: reads x alleles from which route="auto" takes the kernels


class AlignLinearOpts(C.Structure):
    """hgx_align_linear_opts (include/hgx.h); `bytes` = sizeof."""
    _fields_ = [("bytes", C.c_int32), ("max_edits", C.c_int32), ("k", C.c_int32), ("fastq", C.c_int32), ("route", C.c_int32)]


def linear_alleles(Genes, refGenes):
    """[(name, sequence)] in index order: every gene of `Genes` in dict order, its entries in dict order except the backbone
    refGenes[gene] (the linear typing skips records whose RNAME contains BACKBONE: indexing it would only spend k slots)."""
    return [(name, seq) for g in Genes for name, seq in Genes[g].items() if name != refGenes[g]]


class LinearAlignIndex:
    """The allele sequences of `Genes` (linear_alleles order) with their seed table, ready for align()."""

    def __init__(self, Genes, refGenes):
        alleles = linear_alleles(Genes, refGenes)
        self.names = [n for n, _ in alleles]
        names = [n.encode() for n, _ in alleles]
        seqs = [s.encode() for _, s in alleles]
        self.h = C.c_void_p()
        capi.check(capi.lib().hgx_align_linear_index_create(C.byref(self.h), C.c_int32(len(names)), (C.c_char_p * max(len(names), 1))(*names),
                                                            (C.c_char_p * max(len(seqs), 1))(*seqs)))

    def align(self, reads, max_edits=2, k=10, fastq=None, route="auto"):
        """SAM text (bytes) for `reads` = one or two FASTA / FASTQ[.gz] paths (str) or in-memory texts (bytes), or an engine.Reads made
        of them beforehand (`fastq` is then not looked at): @HD, an @SQ per allele, and per read up to `k` records (k = 10 is the
        reference's `-k 10`) of its hits with at most `max_edits` (0 .. 4) mismatches, ordered by (NM, allele, position, strand).
        `route`: "auto" (the kernels from reads x alleles >= LINEAR_GATE, the measured break-even; the host route below), "host",
        "device" (the kernels; they decline to the host route with a code of LINEAR_DECLINE_*: align_linear_last()).  The bytes are
        the same."""
        made = hasattr(reads, "n_reads")
        opts = AlignLinearOpts(C.sizeof(AlignLinearOpts), int(max_edits), int(k), -1 if fastq is None else int(bool(fastq)), ROUTES[route])
        out_p, n = C.c_void_p(), C.c_size_t(0)
        if made:
            rc = capi.lib().hgx_align_linear_reads_dev(self.h, reads.h, C.byref(opts), C.byref(out_p), C.byref(n))
        else:
            assert len(reads) in (1, 2)
            if all(isinstance(r, str) for r in reads):
                paths = (C.c_char_p * len(reads))(*[r.encode() for r in reads])
                rc = capi.lib().hgx_align_linear_reads(self.h, C.c_int32(len(reads)), paths, None, None, C.byref(opts), C.byref(out_p), C.byref(n))
            else:
                bufs = [bytes(r) for r in reads]
                texts = (C.c_char_p * len(bufs))(*bufs)
                sizes = (C.c_size_t * len(bufs))(*[len(b) for b in bufs])
                rc = capi.lib().hgx_align_linear_reads(self.h, C.c_int32(len(bufs)), None, texts, sizes, C.byref(opts), C.byref(out_p), C.byref(n))
        capi.check(rc)
        try:
            return C.string_at(out_p.value, n.value)
        finally:
            capi.lib().hgx_free_text(out_p)

    def close(self):
        if self.h:
            capi.lib().hgx_align_linear_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align_linear_last():
    """dict(route, reads, aligned, records, candidates, decline) of the calling thread's last LinearAlignIndex.align(): route 2 = the
    kernels, 0 = the host route (decline says why); reads given, reads with a record, records written, seed-table entries looked at."""
    route, dec = C.c_int32(0), C.c_int32(0)
    reads, aligned, records, cand = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().hgx_align_linear_last(C.byref(route), C.byref(reads), C.byref(aligned), C.byref(records), C.byref(cand), C.byref(dec)))
    return dict(route=route.value, reads=reads.value, aligned=aligned.value, records=records.value, candidates=cand.value, decline=dec.value)


_LINEAR_INDEX_CACHE = []   # [(Genes, refGenes, LinearAlignIndex)]


def cached_linear_index(Genes, refGenes):
    """The linear index of these dicts, found again by the IDENTITY of the two dict objects (as cached_index: dicts edited in place
    return the index of their old content; callers that edit their dicts build a LinearAlignIndex themselves)."""
    for g, rg, ix in _LINEAR_INDEX_CACHE:
        if g is Genes and rg is refGenes:
            return ix
    ix = LinearAlignIndex(Genes, refGenes)
    _LINEAR_INDEX_CACHE.append((Genes, refGenes, ix))
    del _LINEAR_INDEX_CACHE[:-4]
    return ix
