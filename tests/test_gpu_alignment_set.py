"""Many alignment files x many loci, every file read ONCE (hgx_alignment_set_*, hgx_many_create_set): a panel is one BAM per sample,
each holding the records of every locus (hisatgenotype:613-665 pools the samples; typing_core.py:370, 436-468 loops the loci over
each sample's one file).  engine.AlignmentSet reads, sends, inflates and walks the files once, route() sends every record to the
loci that keep it in one pass, and ManyBatch.from_set makes a locus' many-task batch from the resident bytes.  Held here to: the
batch of the per-locus path (ManyBatch.from_files) and of the host front end, array for array; the Python oracle; the plain-Python
routing of tests/route_ref.py; the partition kernels' tile edges; bytes sent once; slots made side by side; the fallbacks."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

import hisatgenotype_amd as hgx
from hisatgenotype_amd import bamio, capi, engine, indexio, locus as hl, synth

import oracle_util as ou
import route_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyref  # noqa: E402

htyping = sys.modules["hisatgenotype_amd.typing"]
pytestmark = pytest.mark.gpu
EM_TOL = 1e-9
N_FILES = 3
DECOY = ("DECOY*BACKBONE", 5000)


def same_merged(a, b):
    assert (a.n_reads, a.n_pairs, a.n_pieces, a.n_refs, a.n_mask_u32) == (b.n_reads, b.n_pairs, b.n_pieces, b.n_refs, b.n_mask_u32)
    for k in ("pieces", "masks", "pair_off", "pair_ref"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def same_many(dev, host):
    assert dev.n_tasks == host.n_tasks
    assert (dev.n_pieces, dev.n_pairs, dev.n_refs, dev.n_reads) == (host.n_pieces, host.n_pairs, host.n_refs, host.n_reads)
    assert dev.pair_base == host.pair_base
    assert dev.task_reads == host.task_reads and dev.task_pieces == host.task_pieces and dev.task_refs == host.task_refs
    same_merged(dev.merged(), host.merged())


def same_results(pl, dev, host):
    for em_fast in (False, None):
        for g, h in zip(htyping.type_many(pl, dev, em_fast=em_fast), htyping.type_many(pl, host, em_fast=em_fast)):
            assert g.num_reads == h.num_reads and g.num_pairs == h.num_pairs
            if g.num_reads == 0:
                continue
            assert np.array_equal(g.counts_order, h.counts_order) and np.array_equal(g.counts, h.counts)
            assert [e["n_iter"] for e in g.em] == [e["n_iter"] for e in h.em]
            assert [e["result"] for e in g.em] == [e["result"] for e in h.em]
            assert g.gene_prob == h.gene_prob


@functools.lru_cache(maxsize=None)
def _loci():
    specs = [("A", 600, 3569, 1300, 0), ("B", 800, 4081, 1500, 5000), ("C", 500, 4305, 1200, 10000)]
    return [synth.make_hla_like_locus(gene=g, n_alleles=n, length=ln, n_vars=v, seed=300 + k, var_id_base=base)
            for k, (g, n, ln, v, base) in enumerate(specs)]


@functools.lru_cache(maxsize=None)
def _sams(n_pairs=1500):
    """[file][locus] -> name-grouped SAM text of that sample at that locus."""
    return [[synth.simulate_sam_fast(loc, synth.pick_sample(loc, 40 + 7 * f + k), n_pairs + 100 * k + 31 * f, err_rate=0.003, seed=50 + 10 * f + k)
             for k, loc in enumerate(_loci())] for f in range(N_FILES)]


def _oracle_one(locus_json, sam):
    return pyref.RefLocus(synth.Locus.from_json(locus_json)).run(sam)


@functools.lru_cache(maxsize=None)
def _oracle():
    """The Python oracle on every (sample, locus), the nine runs side by side on the host's cores."""
    with ou.pool(N_FILES * len(_loci())) as ex:
        fut = {(f, loc.gene): ex.submit(_oracle_one, loc.to_json(), _sams()[f][k]) for f in range(N_FILES) for k, loc in enumerate(_loci())}
        return {key: f.result() for key, f in fut.items()}


def _extra_lines(f):
    """Records no locus keeps: a decoy reference's, and unmapped ones without a reference."""
    seq = "ACGT" * 25
    decoy = ["decoy%d_%d\t0\t%s\t%d\t60\t100M\t*\t0\t0\t%s\t*" % (f, i, DECOY[0], 1 + 37 * i, seq) for i in range(40)]
    unmapped = ["unmapped%d_%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*" % (f, i, seq) for i in range(25)]
    return "\n".join(decoy + unmapped) + "\n"


def _refs(order=None):
    refs = [(loc.ref_allele, len(loc.backbone)) for loc in _loci()] + [DECOY]
    return refs if order is None else [refs[i] for i in order]


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    """Three sample files, each holding the records of loci A, B and C, a decoy reference's and unmapped ones: file 0 sorted by
    coordinate, files 1 and 2 name-grouped; file 2's header lists the references in another order."""
    d = tmp_path_factory.mktemp("panel")
    paths = []
    for f in range(N_FILES):
        p = str(d / ("sample%d.bam" % f))
        text = "".join(_sams()[f]) + _extra_lines(f)
        bamio.write_bam_native(p, text.encode(), _refs([2, 3, 0, 1] if f == 2 else None), sort_by_coordinate=(f == 0))
        paths.append(p)
    pls = [hl.PackedLocus.from_synth(loc) for loc in _loci()]
    regions = [loc.ref_allele for loc in _loci()]
    return paths, pls, regions


def _host_many(pl, paths, region):
    return engine.ManyBatch(pl, [pl.parse_alignment_file(p, [region] if region else None) for p in paths])


def test_same_batch_as_the_per_locus_path(panel):
    capi.set_device(0)
    paths, pls, regions = panel
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths) as aset:
            assert aset.resident and aset.n_files == N_FILES and aset.n_records == sum(len(bamio.read_bam(p)) for p in paths)
            aset.route(regions)
            assert aset.kept == route_ref.kept_counts(paths, regions)
            for slot, (pl, region) in enumerate(zip(pls, regions)):
                got = engine.ManyBatch.from_set(pl, aset, slot)
                assert engine.front_last() == (2, 0), engine.front_last()
                per_locus = engine.ManyBatch.from_files(pl, paths, regions=[region] * N_FILES)
                assert engine.front_last() == (2, 0), engine.front_last()
                host = _host_many(pl, paths, region)
                same_many(got, per_locus)
                same_many(got, host)
                same_results(pl, got, host)


def test_pinned_to_the_oracle(panel):
    capi.set_device(0)
    paths, pls, _ = panel
    names = {loc.gene: [n for n in loc.allele_names if "BACKBONE" not in n] for loc in _loci()}
    for em_fast in (None, False):
        got = htyping.type_panel_files(pls, paths, em_fast=em_fast)
        assert set(got) == set(_oracle())
        for key, exp in _oracle().items():
            res = got[key]
            assert (res.num_reads, res.num_pairs) == (exp["num_reads"], exp["num_pairs"]), key
            assert res.counts_sorted == exp["counts_sorted"], key
            assert len(res.em) == len(exp["em"]), key
            for g, e in zip(res.em, exp["em"]):
                assert g["n_iter"] == e["n_iter"] and [a for a, _ in g["result"]] == [a for a, _ in e["result"]], key
                for (_, p), (_, q) in zip(g["result"], e["result"]):
                    assert p == q if em_fast is False else abs(p - q) <= EM_TOL, key
            assert [a for a, _ in res.gene_prob] == [a for a, _ in exp["gene_prob"]], key
            for (_, p), (_, q) in zip(res.gene_prob, exp["gene_prob"]):
                assert p == q if em_fast is False else abs(p - q) <= EM_TOL, key
            assert all(a in names[key[1]] for a, _ in res.gene_prob)


@pytest.fixture(scope="module")
def odd_files(tmp_path_factory):
    """x: A, B, C, decoy, unmapped, sorted by coordinate; y: A and C only (no record of B), name-grouped, its header in another order."""
    d = tmp_path_factory.mktemp("odd")
    s = _sams()
    x, y = str(d / "x.bam"), str(d / "y.bam")
    bamio.write_bam_native(x, ("".join(s[0]) + _extra_lines(0)).encode(), _refs(), sort_by_coordinate=True)
    bamio.write_bam_native(y, (s[1][0] + _extra_lines(1) + s[1][2]).encode(), _refs([3, 2, 1, 0]))
    return [x, y]


def test_routing_against_the_reference(odd_files):
    capi.set_device(0)
    paths = odd_files
    loci = _loci()
    pls = [hl.PackedLocus.from_synth(loc) for loc in loci]
    a_ref = loci[0].ref_allele
    # a span whose edges fall on record ends: r1 ends exactly at left0, r2 starts exactly at right0
    spans = sorted({route_ref.record_span(l)[1:] for l in bamio.read_bam(paths[0], [a_ref])})
    left0 = spans[len(spans) // 4][1]
    right0 = min(p for p, _ in spans if p > left0 + 200)
    exact = "%s:%d-%d" % (a_ref, left0 + 1, right0 + 1)
    beyond = "%s:%d-%d" % (a_ref, left0 + 2, right0)                      # one base beyond each: both records fall out
    slots = [(0, a_ref), (1, loci[1].ref_allele), (2, loci[2].ref_allele), (1, "NOBODY*BACKBONE"), (0, a_ref), (0, exact), (0, beyond)]
    regions = [r for _, r in slots]
    want = route_ref.route(paths, regions)
    in_exact, in_beyond = [set(want[k][0]) for k in (5, 6)]
    assert in_beyond < in_exact and len(in_exact - in_beyond) >= 2                                              # (the case is what it is meant to be)
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths).route(regions) as aset:
            assert aset.resident
            assert aset.kept == [[len(v) for v in row] for row in want]
            assert aset.kept[1][1] == 0 and aset.kept[3] == [0, 0] and aset.kept[0] == aset.kept[4]
            assert sum(map(sum, aset.kept[:3])) < aset.n_records            # decoy and unmapped records: in no slot
            for slot, (k, region) in enumerate(slots):
                got = engine.ManyBatch.from_set(pls[k], aset, slot)
                assert engine.front_last() == (2, 0), (slot, engine.front_last())
                same_many(got, engine.ManyBatch.from_files(pls[k], paths, regions=[region] * 2))
                if slot in (1, 3, 5):
                    same_many(got, _host_many(pls[k], paths, region))
                if slot == 3:
                    assert got.task_reads == [0, 0] and got.n_pairs == 0
                    assert [r.num_reads for r in htyping.type_many(pls[k], got)] == [0, 0]


def _pool_lines():
    """Records of loci A and B, two of one then two of the other."""
    a, b = (_sams()[0][k].splitlines() for k in (0, 1))
    out = []
    for i in range(0, min(len(a), len(b)) - 1, 2):
        out += a[i:i + 2] + b[i:i + 2]
    return out


def _many_regions(n):
    loci = _loci()
    regions = [loci[0].ref_allele, loci[1].ref_allele]
    k = 0
    while len(regions) < n:
        regions.append("%s:%d-%d" % (loci[k % 2].ref_allele, 1 + 45 * k, 420 + 45 * k))
        k += 1
    return regions[:n]


@pytest.mark.parametrize("sizes", ["T-1", "T", "T+1", "2T+1"])
def test_partition_edges(tmp_path, sizes):
    """Sets of T - 1, T, T + 1 and 2 T + 1 records (T = the partition kernels' records per workgroup), a change of file exactly at a
    tile boundary, 1, 2 and 64 slots; 65 slots are more than the mask holds: every slot goes per path."""
    capi.set_device(0)
    T = engine.AlignmentSet([]).route_tile
    assert T >= 64
    split = {"T-1": [T // 3, T - 1 - T // 3], "T": [T // 4, T - T // 4], "T+1": [T, 1], "2T+1": [T, T + 1]}[sizes]
    lines = _pool_lines()
    assert len(lines) >= 2 * T + 1
    paths, at = [], 0
    for f, n in enumerate(split):
        paths.append(str(tmp_path / ("f%d.bam" % f)))
        bamio.write_bam_native(paths[-1], ("\n".join(lines[at:at + n]) + "\n").encode(), _refs(), sort_by_coordinate=(f == 1))
        at += n
    pls = [hl.PackedLocus.from_synth(loc) for loc in _loci()[:2]]
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths) as aset:
            assert aset.resident and aset.n_records == sum(split) and aset.max_loci == 64
            for n_slots in (1, 2, 64, 65):
                regions = _many_regions(n_slots)
                aset.route(regions)
                if n_slots == 65:
                    assert aset.kept is None
                else:
                    assert aset.kept == route_ref.kept_counts(paths, regions), n_slots
                for slot in sorted({0, n_slots // 2, n_slots - 1}):
                    pl = pls[0] if regions[slot].startswith("A*") else pls[1]
                    got = engine.ManyBatch.from_set(pl, aset, slot)
                    assert engine.front_last() == (2, 0), engine.front_last()
                    assert (engine.front_last_bytes() == 0) == (n_slots <= 64)      # (65 slots: the per-path call sends the files again)
                    same_many(got, engine.ManyBatch.from_files(pl, paths, regions=[regions[slot]] * len(paths)))
                    if n_slots <= 2:
                        same_many(got, _host_many(pl, paths, regions[slot]))


def test_read_once(panel):
    capi.set_device(0)
    paths, pls, regions = panel
    per_locus_bytes = 0
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(paths).route(regions) as aset:
            tables = aset.block_table_bytes
            assert 0 < tables < aset.bytes_to_device <= sum(os.path.getsize(p) for p in paths) + tables
            assert aset.bytes_to_device < aset.stream_bytes / 2             # the files travel deflated
            for slot, pl in enumerate(pls):
                engine.ManyBatch.from_set(pl, aset, slot)
                assert engine.front_last() == (2, 0) and engine.front_last_bytes() == 0
            for pl, region in zip(pls, regions):
                engine.ManyBatch.from_files(pl, paths, regions=[region] * N_FILES)
                assert engine.front_last() == (2, 0)
                per_locus_bytes += engine.front_last_bytes()
            # today's path sends every file once per locus
            assert per_locus_bytes >= 3 * (aset.bytes_to_device - tables)


def test_slots_side_by_side_from_threads(panel):
    capi.set_device(0)
    paths, pls, regions = panel
    out, errs = {}, []
    with engine.AlignmentSet(paths).route(regions) as aset:
        assert aset.resident                                                 # (9 MB of stream: above the size gate without a switch)
        sequential = [engine.ManyBatch.from_set(pl, aset, slot) for slot, pl in enumerate(pls)]

        def work(slot):
            try:
                capi.set_device(0)
                capi.set_stream_slot(("alignment set test", slot))
                st = capi.get_stream(2)
                out[slot] = engine.ManyBatch.from_set(pls[slot], aset, slot, stream=st)
                assert engine.front_last() == (2, 0)
                capi.sync(st)
            except BaseException as e:      # noqa: BLE001 (reported below)
                errs.append((slot, e))
        ths = [threading.Thread(target=work, args=(slot,)) for slot in range(len(pls))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        for slot in range(len(pls)):
            same_many(out[slot], sequential[slot])


def test_fallbacks_give_the_same_batch_or_the_same_error(panel, tmp_path):
    capi.set_device(0)
    paths, pls, regions = panel
    pl, region = pls[1], regions[1]
    host = _host_many(pl, paths, region)
    with engine.test_switches(front="host"):
        with engine.AlignmentSet(paths).route(regions) as aset:
            assert not aset.resident and aset.kept is None
            got = engine.ManyBatch.from_set(pl, aset, 1)
            assert engine.front_last() == (0, -1), engine.front_last()
    same_many(got, host)
    # one member is SAM text
    sam_path = str(tmp_path / "sample1.sam")
    with open(sam_path, "w") as f:
        f.write("".join("@SQ\tSN:%s\tLN:%d\n" % r for r in _refs()) + "\n".join(bamio.read_bam(paths[1])) + "\n")
    mixed = [paths[0], sam_path, paths[2]]
    with engine.test_switches(front="device"):
        with engine.AlignmentSet(mixed).route(regions) as aset:
            assert not aset.resident
            got = engine.ManyBatch.from_set(pl, aset, 1)
    same_many(got, host)
    # below the size gate, no switch
    small = []
    for f in range(2):
        small.append(str(tmp_path / ("small%d.bam" % f)))
        text = "".join("\n".join(_sams()[f][k].splitlines()[:120]) + "\n" for k in range(3))
        bamio.write_bam_native(small[-1], text.encode(), _refs())
    with engine.AlignmentSet(small).route(regions) as aset:
        assert not aset.resident
        got = engine.ManyBatch.from_set(pl, aset, 1)
        assert engine.front_last() == (0, 6), engine.front_last()
    same_many(got, _host_many(pl, small, region))
    with engine.test_switches(front="device"):
        with pytest.raises(capi.HgxError):
            with engine.AlignmentSet([paths[0], str(tmp_path / "missing.bam")]).route(regions) as aset:
                engine.ManyBatch.from_set(pl, aset, 1)
        # a file cut inside its last BGZF block (the 28-byte end-of-file block and 100 bytes more are gone)
        cut = str(tmp_path / "cut.bam")
        data = open(paths[1], "rb").read()
        open(cut, "wb").write(data[:-128])
        with pytest.raises(Exception) as per_locus:
            engine.ManyBatch.from_files(pl, [paths[0], cut], regions=[region] * 2)
        with pytest.raises(Exception) as from_set:
            with engine.AlignmentSet([paths[0], cut]).route(regions) as aset:
                assert not aset.resident
                engine.ManyBatch.from_set(pl, aset, 1)
        assert from_set.type is per_locus.type and str(from_set.value) == str(per_locus.value)


def test_run_panel_many_from_per_sample_files(panel, tmp_path):
    """run_panel(many=True) on tasks that name the three sample files for three genes: one AlignmentSet, the results of today's
    grouping -- compared with the one-by-one form."""
    capi.set_device(0)
    paths, _, _ = panel
    ix_dir = str(tmp_path / "ix")
    synth.write_index(_loci(), ix_dir, "hla")
    ix = indexio.load_index(ix_dir, "hla")
    tasks = [(f, loc.gene, paths[f]) for loc in _loci() for f in range(N_FILES)]
    opened = []
    real = engine.AlignmentSet

    class Counting(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            opened.append(self)
    engine.AlignmentSet = Counting
    try:
        batched = hgx.run_panel(tasks, ix, "hla", many=True, ix_dir=ix_dir)
    finally:
        engine.AlignmentSet = real
    assert len(opened) == 1 and opened[0].resident and opened[0].paths == paths
    one_by_one = hgx.run_panel(tasks, ix, "hla", many=False, ix_dir=ix_dir)
    assert set(batched) == set(one_by_one) == {(f, loc.gene) for loc in _loci() for f in range(N_FILES)}
    for key, res in one_by_one.items():
        b = batched[key]
        assert (b.num_reads, b.num_pairs) == (res.num_reads, res.num_pairs), key
        assert b.gene_prob == res.gene_prob and b.em == res.em and b.counts_sorted == res.counts_sorted, key
