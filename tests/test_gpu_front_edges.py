"""The DEVICE front end (csrc/hgx_front.hip, csrc/hgx_front_core.hpp) where read length and per-read counts change its path: reads longer
than the decode kernel's LDS staging (FE_SEQ_STAGE_DWORDS = 43 dwords: 172 text bases, 344 packed ones) and right at its edges, staged and
unstaged keys in one wavefront, lengths that leave a partial last dword, odd lengths with a packed SEQ, long reads across the pileup's
backbone tiles -- and the fixed scratch limits (FE_MAX_CMP, FE_MAX_OPS, FE_MAX_ZS) met one step below and one step above, with the call that
declines followed by one that does not.  The fixtures (golden_util.LONG) were recorded from the real reference; the device's batch must
be the host front end's byte for byte and its per-record trace and pileup the reference's."""
import os
import sys

import pytest

import golden_util as gu
from hisatgenotype_amd import capi, engine, locus as hl
from test_gpu_front import same_batch
from trace_util import check_pileup, check_trace, fmt_record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLINED = (0, gu.FE_E_CAP)


def _kw(fx):
    o = fx["options"]
    return dict(num_editdist=o["num_editdist"], error_correction=o["error_correction"], allow_discordant=o["allow_discordant"],
                simulation=o["simulation"], keep_trace=True)


def _three_ways(pl, loc, sam, tmp_path, kw):
    """(what, route a taken call reports, the call): the record route, the key route, a coordinate-sorted BAM with the locus' region."""
    from hisatgenotype_amd import bamio
    p_bam = str(tmp_path / "s.bam")
    bamio.write_bam_native(p_bam, sam.encode(), [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
    return (("records", dict(front="device"), 2, lambda: pl.parse_sam_dev(sam, **kw)),
            ("keys", dict(front="device,keys"), 1, lambda: pl.parse_sam_dev(sam, **kw)),
            ("bam", dict(front="device"), 2, lambda: pl.parse_alignment_file_dev(p_bam, regions=[loc.ref_allele], **kw)))


def _run(switches, call):
    with engine.test_switches(**switches):
        dev = call()
        last = engine.front_last()
    return dev, last


def _taken_everywhere(name, tmp_path):
    fx = gu.load(name)
    loc = fx["_locus"]
    pl = hl.PackedLocus.from_synth(loc)
    kw = _kw(fx)
    host = pl.parse_sam(fx["sam"], **kw)
    for what, switches, route, call in _three_ways(pl, loc, fx["sam"], tmp_path, kw):
        dev, last = _run(switches, call)
        assert last == (route, 0), (name, what, last)
        b = dev.to_host()
        same_batch(host, b, len(loc.backbone))
        check_pileup(fx, b)
        check_trace(fx, b)


@pytest.mark.parametrize("name", gu.LONG_TAKEN)
def test_long_and_odd_length_reads_three_ways(name, tmp_path):
    """hla_long_251: from text every SEQ is longer than the staging (k_fe_decode reads it where it lies), from the BAM every SEQ is
    staged and odd.  hla_len_edges: 75, 171, 172 | 173, 251, 343, 344 | 345 in turn in one stream -- wavefronts with staged and unstaged
    keys, staged lengths whose last dword is partial (text 75, 171; packed 75, 171, 173, 251, 343)."""
    _taken_everywhere(name, tmp_path)


def test_unused_nibble_of_an_odd_packed_seq_is_no_part_of_the_read(tmp_path):
    """A BAM of 2x251 whose writer left something in the low nibble of every odd-length SEQ's last byte, differently from record to
    record, with duplicate lines that differ in nothing else: k_fe_records / k_fe_rec_filter_insert make one key of a duplicate
    (fe_rec_key, fe_rec_same_key), k_fe_pileup and k_fe_decode (FeSeq::at, from staged bytes) read 251 bases -- the batch and the
    trace of the clean BAM."""
    fx = gu.load("hla_long_251")
    loc = fx["_locus"]
    pl = hl.PackedLocus.from_synth(loc)
    kw = _kw(fx)
    lines = [l for l in fx["sam"].split("\n") if l]
    sam = "".join(l + "\n" + (l + "\n" if k % 9 == 0 else "") for k, l in enumerate(lines))
    from hisatgenotype_amd import bamio
    p_clean, p_junk = str(tmp_path / "clean.bam"), str(tmp_path / "junk.bam")
    bamio.write_bam_native(p_clean, sam.encode(), [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
    assert gu.junk_nibble_bam(p_clean, p_junk) > len(lines) * 3 // 4
    host = pl.parse_sam(sam, **kw)
    assert host.n_reads == len(fx["records"])                     # (the second line of a duplicate counts for nothing)
    for path in (p_clean, p_junk):
        dev, last = _run(dict(front="device"), lambda: pl.parse_alignment_file_dev(path, regions=[loc.ref_allele], **kw))
        assert last == (2, 0), (path, last)
        b = dev.to_host()
        same_batch(host, b, len(loc.backbone))
        assert b.trace_text() == host.trace_text(), path


def test_dense_long_read_sample_declines_with_the_cap_code_and_the_next_call_is_right(tmp_path):
    """hla_dense_301: cmp_list outgrows FE_MAX_CMP on some keys while the others are decoded -- a call that ran most of its kernels
    declines with FE_E_CAP on every route (with keep_trace too: the trace pool holds the largest trace of every key) and returns the host
    front end's batch; the next call of the process, on another fixture, is taken and right: nothing of the declined call's control
    block or pools is left behind."""
    fx = gu.load("hla_dense_301")
    loc = fx["_locus"]
    pl = hl.PackedLocus.from_synth(loc)
    kw = _kw(fx)
    host = pl.parse_sam(fx["sam"], **kw)
    check_trace(fx, host)
    for what, switches, route, call in _three_ways(pl, loc, fx["sam"], tmp_path, kw):
        dev, last = _run(switches, call)
        assert last == DECLINED, (what, last)
        same_batch(host, dev.to_host(), len(loc.backbone), pileup=False)
        (tmp_path / what).mkdir()
        _taken_everywhere("hla_len_edges", tmp_path / what)


@pytest.mark.parametrize("name", sorted(gu.LONG_FAMILIES))
def test_cap_families_are_taken_up_to_the_limit_and_declined_beyond(name, tmp_path):
    """hla_cap_cmp (cmp_list2 of 60 .. 69 entries around FE_MAX_CMP = 64) and hla_cap_ops (21 .. 27 CIGAR ops around FE_MAX_OPS = 24),
    hla_cap_zs (46 .. 50 Zs items around FE_MAX_ZS = 48, in runs of adjacent known SNPs so that cmp_list2 stays short), one read per call: the device takes exactly the members the REFERENCE's recorded counts put at or below the limit -- with the
    reference's trace line -- and declines the others with FE_E_CAP; the batch is the host front end's either way."""
    fx = gu.load(name)
    kind = gu.LONG_FAMILIES[name]
    loc = fx["_locus"]
    pl = hl.PackedLocus.from_synth(loc)
    kw = _kw(fx)
    seen = set()
    for qname, line, k, n_cmp, n_ops, n_zs in gu.family_members(fx):
        taken = gu.member_taken(kind, n_cmp, n_ops, n_zs)
        seen.add(taken)
        host = pl.parse_sam(line, **kw)
        assert host.trace_text().splitlines() == [fmt_record(fx["records"][k])]
        (tmp_path / qname).mkdir()
        for what, switches, route, call in _three_ways(pl, loc, line, tmp_path / qname, kw):
            dev, last = _run(switches, call)
            assert last == ((route, 0) if taken else DECLINED), (qname, what, n_cmp, n_ops, n_zs, last)
            b = dev.to_host()
            same_batch(host, b, len(loc.backbone), pileup=taken)
            if taken:
                assert b.trace_text().splitlines() == [fmt_record(fx["records"][k])], (qname, what)
    assert seen == {True, False}
    # the whole family as one stream: declined, the host's batch
    host = pl.parse_sam(fx["sam"], **kw)
    for what, switches, route, call in _three_ways(pl, loc, fx["sam"], tmp_path, kw):
        dev, last = _run(switches, call)
        assert last == DECLINED, (what, last)
        same_batch(host, dev.to_host(), len(loc.backbone), pileup=False)


def test_long_reads_through_scoring_and_em_give_the_recorded_report(tmp_path):
    """hgx_type_file on hla_long_251 under front=device, from the SAM text and from a coordinate-sorted BAM: the long-read batch goes
    through scoring and both EMs to the report the reference wrote."""
    import hisatgenotype_amd as hgx
    from hisatgenotype_amd import bamio
    fx = gu.load("hla_long_251")
    o = fx["options"]
    loc = fx["_locus"]
    pl = hl.PackedLocus.from_synth(loc)
    p_sam, p_bam = tmp_path / "reads.sam", tmp_path / "sorted.bam"
    p_sam.write_text(fx["sam"])
    bamio.write_bam_native(str(p_bam), fx["sam"].encode(), [(loc.ref_allele, len(loc.backbone))], sort_by_coordinate=True)
    keep = lambda ls: [l for l in ls if "aligned" in l or "ranked" in l or "(count:" in l]
    want = keep(fx["report"].split("\n"))
    assert len(want) > 2
    for path in (p_sam, p_bam):
        with engine.test_switches(front="device"):
            res = hgx.type_file(pl, str(path), num_editdist=o["num_editdist"], error_correction=o["error_correction"],
                                allow_discordant=o["allow_discordant"], remove_low_abundance_alleles=o["remove_low"], simulation=o["simulation"])
            assert engine.front_last() == (2, 0), (path.name, engine.front_last())
        assert (res.num_reads, res.num_pairs) == (len(fx["records"]), len(fx["pairs"]))
        assert [e["n_iter"] for e in res.em] == [e["n_iter"] for e in fx["em"]]
        got, _ = hgx.report_lines(res, o["simulation"], (), True)
        assert keep(got) == want, path.name


def test_device_front_end_on_fuzz_cases_of_other_read_lengths(tmp_path):
    """tools/fuzz_parity.py's cases with reads of 75, 151, 173, 251 and 345 bases (HLA-like and STR loci, errors, soft clips, novel indels,
    multi-hit and duplicate records, single-end samples): the record route, the key route and a coordinate-sorted BAM against the host
    front end, as test_gpu_front.test_device_front_end_on_fuzz_cases compares them.  Dense cases may decline: the codes are printed."""
    from hisatgenotype_amd import bamio
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    why = {}
    for k in range(20):
        read_len = (75, 151, 173, 251, 345)[k % 5]
        loc, sam, single = fuzz_parity.make_case(990000, k, 1, read_len=read_len)
        pl = hl.PackedLocus.from_synth(loc)
        kw = dict(error_correction=k % 2 == 0, allow_discordant=single)
        (tmp_path / str(k)).mkdir()
        ways = _three_ways(pl, loc, sam, tmp_path / str(k), kw)
        try:
            host = pl.parse_sam(sam, **kw)
        except capi.HgxError:
            for what, switches, route, call in ways:
                with engine.test_switches(**switches), pytest.raises(capi.HgxError):
                    call()
            continue
        for what, switches, route, call in ways:
            dev, (ran, code) = _run(switches, call)
            assert ran in (0, route), (k, what, ran, code)
            why[(what, ran, code)] = why.get((what, ran, code), 0) + 1
            same_batch(host, dev.to_host(), len(loc.backbone), pileup=ran > 0)
        pl.close()
    print("read lengths 75 .. 345: (way, route, decline code) -> cases: %s" % sorted(why.items()))
