"""BASELINE.json configs at their stated sizes on the GPU ("configs not exercised").

  configs[1]  HLA-A, 1 M simulated 2x150 bp reads (500 000 pairs), 7 000 alleles: size-independent properties, and (round 5) the whole
              sample `==` the oracle chain at its stated size (classes, counts, EM iteration counts, order; abundances <= 1e-9)
  configs[3]  full HLA panel (A/B/C/DRB1/DQA1/DQB1, 500 ... 8 000 alleles) x 64 synthetic samples through run_panel:
              8 samples x 6 loci against the oracle (counts exact, EM iteration counts, allele order, abundances), the other
              336 tasks through properties
  configs[4]  CODIS STR panel, 13 loci, 500 k reads in total: BIT-EXACT against the oracle (class tables, counts, EM floats)

The oracle (pyref front-end + C oracle, tests/oracle_util.py) runs in a spawn-ed process pool on the host cores beside the
GPU work; everything it is compared with went through the C-ABI (libhgx)."""
import os
import sys

import numpy as np
import pytest

import hisatgenotype_amd as hgx
from hisatgenotype_amd import indexio, locus as hl, synth

import oracle_util as ou

pytestmark = pytest.mark.gpu

EM_TOL = 1e-5          # north_star: EM float weights within 1e-5 of the reference
TIGHT = 1e-9           # what this implementation holds on every case seen so far


def _counts_dict(res):
    return {a: c for a, c in res.counts_sorted}


def _check_against_oracle(res, exp, names):
    assert (res.num_reads, res.num_pairs) == (exp["num_reads"], exp["num_pairs"])
    cnt = {n: int(c) for n, c in zip(names, exp["gene_counts"]) if c}
    assert _counts_dict(res) == cnt                                   # integer compatibility counts: bit-exact
    # print order of the counts: descending, ties in first-counted order (core:1650-1651)
    order = sorted(cnt, key=lambda n: (-cnt[n], int(exp["first_pair"][names.index(n)]), names.index(n)))
    assert [a for a, _ in res.counts_sorted] == order
    assert [(e["n_classes"], e["n_iter"]) for e in res.em] == [(c, it) for c, it, _ in exp["em"]]
    # EMs of up to 4096 classes run in the reference's own order of operations (k_emx, round 3): the same doubles, not close ones
    exact = all(e["n_classes"] <= 4096 for e in res.em)
    for got, (c, it, r) in zip(res.em, exp["em"]):
        assert [a for a, _ in got["result"]] == [a for a, _ in r]
        for (a, p), (_, q) in zip(got["result"], r):
            assert abs(p - q) <= EM_TOL and abs(p - q) <= TIGHT, (a, p, q)
            if got["use_length"] or got["n_classes"] <= 4096:
                assert p == q, (a, repr(p), repr(q))
    assert [a for a, _ in res.gene_prob] == [a for a, _ in exp["gene_prob"]]
    for (a, p), (_, q) in zip(res.gene_prob, exp["gene_prob"]):
        assert abs(p - q) <= TIGHT
        if exact:
            assert p == q, (a, repr(p), repr(q))


# ---------------------------------------------------------------------------------------------------------------------
# configs[1]
# ---------------------------------------------------------------------------------------------------------------------
def test_config1_one_million_reads_properties():
    """configs[1] at its full size: 500 000 pairs = 1 M reads, 7 000 alleles (the workload bench.py times).  No oracle
    finishes this in seconds; the domain's size-independent properties do."""
    from hisatgenotype_amd import engine
    loc = synth.make_hla_like_locus(n_alleles=7000, n_vars=2500, seed=101)
    sample = synth.pick_sample(loc, 101)
    sam = synth.simulate_sam_fast(loc, sample, 500000, err_rate=0.002, seed=100)
    pl = hl.PackedLocus.from_synth(loc)
    batch = pl.parse_sam(sam)
    assert batch.n_reads >= 990000 and batch.n_pairs >= 499000 and batch.n_refs > batch.n_pieces
    db = engine.DeviceBatch(batch)
    bufs = engine.ScoreBuffers(pl, db)
    engine.score_pairs(pl, db, bufs)
    for rows, hashes in ((bufs.gene_bits, bufs.gene_hash), (bufs.exon_bits, bufs.exon_hash)):
        cl = engine.Classes.dedup(rows, db.n_pairs, pl.a_pad, hashes=hashes)
        bits, cnt, first = cl.to_host()
        assert cnt.sum() == batch.n_pairs                      # every pair lands in exactly one class
        assert np.all(np.diff(first) > 0)                      # classes come out in first-seen order
        assert len({r.tobytes() for r in bits}) == len(bits)   # and are distinct
        # idempotence: the class matrix deduplicated again with its counts as weights is itself
        d_w = engine.DevArray.from_host(cnt)
        b_ptr, _, _ = cl.device_ptrs()
        again = engine.Classes.dedup(engine._RawDev(b_ptr), cl.n_classes, pl.a_pad, weights=d_w)
        b2, c2, _ = again.to_host()
        assert np.array_equal(b2, bits) and np.array_equal(c2, cnt)
        # Gene_counts = column sums of the weighted class matrix (checksum of checksums)
        ac, fc = cl.allele_counts()
        col = np.zeros(pl.a_pad, np.float64)                   # exact: every partial sum is an integer < 2^53
        firstc = np.full(pl.a_pad, -1, np.int64)
        for c0 in range(0, len(cnt), 4096):
            u = np.unpackbits(bits[c0:c0 + 4096].view(np.uint8), axis=1, bitorder="little")
            col += cnt[c0:c0 + 4096].astype(np.float64) @ u.astype(np.float64)
            new = (firstc < 0) & u.any(axis=0)
            firstc[new] = c0 + u[:, new].argmax(axis=0)
        assert np.array_equal(ac, col.astype(np.int64)) and ac.max() <= batch.n_pairs
        assert np.array_equal(fc[firstc >= 0], firstc[firstc >= 0])           # first class containing each allele
        again.close()
        cl.close()
    # the grouped exon-level form (what typing uses) gives the same class table as the per-pair form
    res = hgx.type_locus(pl, sam, keep_classes=True)
    ecl = engine.Classes.dedup(bufs.exon_bits, db.n_pairs, pl.a_pad, hashes=bufs.exon_hash)
    eb, ec, _ = ecl.to_host()
    assert np.array_equal(res.exon_classes[0], eb) and np.array_equal(res.exon_classes[1], ec)
    # the whole path: abundances are a distribution and the two true alleles win with about half each
    assert abs(sum(p for _, p in res.gene_prob) - 1.0) < 1e-9
    assert [a for a, _ in sorted(res.gene_prob[:2])] == sorted(sample)
    assert all(0.45 < p < 0.55 for _, p in res.gene_prob[:2])
    assert res.num_reads == batch.n_reads and res.num_pairs == batch.n_pairs
    # determinism: a second run is identical, bit for bit
    res2 = hgx.type_locus(pl, sam)
    assert res2.gene_prob == res.gene_prob and res2.em == res.em and res2.counts_sorted[:50] == res.counts_sorted[:50]


def test_config1_one_million_reads_equals_the_oracle():
    """configs[1] AT ITS STATED SIZE against the oracle, `==` (VERDICT r4 #1c) -- the workload bench.py times: HLA-A-like, 7 000
    alleles, 500 000 pairs = 1 M reads.  The oracle chain (oracle/pyref.py front end -> oracle/hgx_oracle.c add_count / add_stat /
    class dicts / single_abundance / hand-off, every step in the reference's own order) runs shard by shard on the host cores
    (oracle_util.oracle_type_sharded; tests/test_oracle_sharded.py pins the sharded form to the one-process form).  The product
    side is ONE hgx_type_* call per variant, through the DEVICE front end (asserted): record fields, filters, pileup, decode,
    piece table, pair protocol, scoring, dedup, Gene_counts, both EMs, hand-off.
      integer work   read / pair counts, Gene_counts of all 7 000 alleles and their print order, the exon-level and the gene-level
                     class tables (bit rows, pair counts, dict order)                                               ==
      EM, default    (table-lookup mat-vecs for the 16 098-class EM #1) iteration counts ==, allele order ==, abundances <= 1e-9
      EM, em_fast=-1 (the reference's order at every size) every abundance the same IEEE double                     =="""
    from hisatgenotype_amd import engine
    loc = synth.make_hla_like_locus(n_alleles=7000, n_vars=2500, seed=101)
    sample = synth.pick_sample(loc, 101)
    sam = synth.simulate_sam_fast(loc, sample, 500000, err_rate=0.002, seed=100)
    names = [n for n in loc.allele_names if "BACKBONE" not in n]
    import threading
    box = {}

    def oracle():
        try:
            box["exp"] = ou.oracle_type_sharded(loc, sam)
        except BaseException as e:                                     # re-raised on the test's thread
            box["err"] = e
    th = threading.Thread(target=oracle)
    th.start()
    try:
        pl = hl.PackedLocus.from_synth(loc)
        n_rerun = engine.em_tie_reruns()
        res = hgx.type_locus(pl, sam, keep_classes=True)
        print("configs[1] default path: %d exact re-run(s) of an EM" % (engine.em_tie_reruns() - n_rerun))
        assert engine.front_last() == (2, 0), engine.front_last()          # the kernels took the records themselves
        res_x = hgx.type_locus(pl, sam, em_fast=-1)
        assert engine.front_last() == (2, 0)
    finally:
        th.join()
    if "err" in box:
        raise box["err"]
    exp = box["exp"]
    assert res.num_pairs >= 499000 and res.num_reads >= 990000
    _check_against_oracle(res, exp, names)
    for got, want in ((res.gene_classes, exp["gene_classes"]), (res.exon_classes, exp["exon_classes"])):
        bits, cnt = got
        ob, oc = want
        w = ob.shape[1]
        assert len(cnt) == len(oc) and np.array_equal(cnt, oc)
        assert np.array_equal(bits[:, :w], ob) and not bits[:, w:].any()
    assert len(exp["exon_classes"][1]) > 4096                          # EM #1 is the large problem
    assert sorted(a for a, _ in res.gene_prob[:2]) == sorted(sample) == sorted(a for a, _ in exp["gene_prob"][:2])
    # the reference's order of operations at every size: the same doubles
    assert [(e["n_classes"], e["n_iter"]) for e in res_x.em] == [(c, it) for c, it, _ in exp["em"]]
    for got, (_, _, r) in zip(res_x.em, exp["em"]):
        assert [(a, p) for a, p in got["result"]] == [(a, p) for a, p in r]
    assert [(a, p) for a, p in res_x.gene_prob] == [(a, p) for a, p in exp["gene_prob"]]
    assert res_x.counts_sorted == res.counts_sorted
    # the default path's report: the reference's text, line for line (res_x is the reference's, bit for bit)
    assert hgx.report_lines(res) == hgx.report_lines(res_x)


# ---------------------------------------------------------------------------------------------------------------------
# configs[3]
# ---------------------------------------------------------------------------------------------------------------------
PANEL = [  # gene, alleles, backbone length, variant sites (six loci, A from 500 to 8 000)
    ("A", 7000, 3569, 2500), ("B", 8000, 4081, 2800), ("C", 7000, 4305, 2600),
    ("DRB1", 3000, 3800, 1800), ("DQA1", 500, 3300, 600), ("DQB1", 2000, 3600, 1400)]
N_SAMPLES = 64
N_ORACLE_SAMPLES = 8
PAIRS_PER_TASK = 1500


def test_config3_full_panel_64_samples(tmp_path):
    """configs[3]: six HLA loci x 64 synthetic samples = 384 independent (sample, locus) tasks from index files through
    run_panel, split over two ranks (no communication) and with three tasks in flight per GPU.  Samples 0-7 (48 tasks) are
    compared with the oracle; all 384 must call the two true alleles, conserve their pairs and be identical between the
    sharded and the concurrent run."""
    loci = [synth.make_hla_like_locus(gene=g, n_alleles=a, length=ln, n_vars=v, seed=500 + i, var_id_base=10000 * i)
            for i, (g, a, ln, v) in enumerate(PANEL)]
    ix_dir = str(tmp_path / "ix")
    synth.write_index(loci, ix_dir, "hla")
    ix = indexio.load_index(ix_dir, "hla")
    tasks, truth, weights = [], {}, []
    for s in range(N_SAMPLES):
        for k, loc in enumerate(loci):
            sample = synth.pick_sample(loc, 1000 * s + k)
            sam = synth.simulate_sam_fast(loc, sample, PAIRS_PER_TASK, err_rate=0.002, seed=100 * s + k)
            tasks.append((s, loc.gene, sam))
            truth[(s, loc.gene)] = sorted(sample)
            weights.append(len(loc.allele_names))
    # oracle for the first samples, on the host cores, while the GPU works
    by_gene = {loc.gene: loc for loc in loci}
    ex = ou.pool(N_ORACLE_SAMPLES * len(loci))
    fut = {(s, g): ex.submit(ou.oracle_type, by_gene[g].to_json(), sam) for s, g, sam in tasks if s < N_ORACLE_SAMPLES}
    try:
        got = {}
        for rank in range(2):
            part = hgx.run_panel(tasks, ix, "hla", rank=rank, world=2, weights=weights, ix_dir=ix_dir)
            assert not set(part) & set(got)
            got.update(part)
        assert set(got) == set(truth)
        conc = hgx.run_panel(tasks, ix, "hla", inflight=3, weights=weights, ix_dir=ix_dir)
        assert set(conc) == set(got)
        # ... and with all the tasks of a locus behind ONE launch chain (hgx_type_many): `==` on every field of all 384 results
        batched = hgx.run_panel(tasks, ix, "hla", many=True, weights=weights, ix_dir=ix_dir)
        assert set(batched) == set(got)
        for key, res in got.items():
            b = batched[key]
            assert b.num_reads == res.num_reads and b.num_pairs == res.num_pairs
            assert b.gene_prob == res.gene_prob and b.em == res.em and b.counts_sorted == res.counts_sorted, key
        for key, res in got.items():
            assert 0.99 * PAIRS_PER_TASK <= res.num_pairs <= PAIRS_PER_TASK and res.num_reads > 1.9 * PAIRS_PER_TASK
            assert max(c for _, c in res.counts_sorted[:1]) <= res.num_pairs
            assert abs(sum(p for _, p in res.gene_prob) - 1.0) < 1e-9
            assert sorted(a for a, _ in res.gene_prob[:2]) == truth[key], (key, res.gene_prob[:3], truth[key])
            c = conc[key]
            assert c.gene_prob == res.gene_prob and c.em == res.em and c.counts_sorted == res.counts_sorted
        for (s, g), f in fut.items():
            names = [n for n in by_gene[g].allele_names if "BACKBONE" not in n]
            _check_against_oracle(got[(s, g)], f.result(), names)
    finally:
        ex.shutdown(cancel_futures=True)


# ---------------------------------------------------------------------------------------------------------------------
# configs[4]
# ---------------------------------------------------------------------------------------------------------------------
CODIS13 = [  # the 13 CODIS core loci: repeat unit, largest / smallest repeat count of the allele ladder
    ("CSF1PO", "AGAT", 15, 6), ("FGA", "CTTT", 30, 16), ("TH01", "AATG", 12, 4), ("TPOX", "AATG", 13, 6),
    ("VWA", "TCTA", 21, 11), ("D3S1358", "TCTA", 19, 12), ("D5S818", "AGAT", 16, 7), ("D7S820", "GATA", 14, 6),
    ("D8S1179", "TCTA", 19, 7), ("D13S317", "TATC", 15, 8), ("D16S539", "GATA", 15, 5), ("D18S51", "AGAA", 22, 9),
    ("D21S11", "TCTA", 38, 24)]
CODIS_READS = 500000


def test_config4_codis_500k_reads_bit_exact():
    """configs[4]: 13 STR loci, 500 k reads in total (19 231 pairs of 2x100 bp per locus), integer / indexing path.
    Every locus against the oracle, BIT-EXACT: the gene-level class table (bit rows, pair counts, dict order), Gene_counts
    and their print order, and -- these EMs run on one wavefront in the reference's own order of operations -- the
    abundances as the same IEEE doubles."""
    pairs = CODIS_READS // 2 // len(CODIS13) + 1
    loci, sams, samples = [], [], []
    for k, (gene, unit, mx, mn) in enumerate(CODIS13):
        loc = synth.make_str_like_locus(gene=gene, unit=unit, max_repeats=mx, min_repeats=mn, flank=200, seed=900 + k,
                                        var_id_base=100 * k)
        sample = ["%s*%d" % (gene, mn + 1 + k % 3), "%s*%d" % (gene, mx - 1 - k % 4)]
        loci.append(loc)
        samples.append(sample)
        sams.append(synth.simulate_sam_fast(loc, sample, pairs, read_len=100, frag_len=(230, 270), err_rate=0.002, seed=40 + k))
    ex = ou.pool(len(loci))
    fut = [ex.submit(ou.oracle_type, loc.to_json(), sam) for loc, sam in zip(loci, sams)]
    total_reads = 0
    try:
        for loc, sam, sample, f, (_, unit, mx, _) in zip(loci, sams, samples, fut, CODIS13):
            pl = hl.PackedLocus.from_synth(loc)
            res = hgx.type_locus(pl, sam, keep_classes=True)
            exp = f.result()
            total_reads += res.num_reads
            names = [n for n in loc.allele_names if "BACKBONE" not in n]
            _check_against_oracle(res, exp, names)
            bits, cnt = res.gene_classes
            ob, oc = exp["gene_classes"]
            w = ob.shape[1]
            assert np.array_equal(bits[:, :w], ob) and not bits[:, w:].any() and np.array_equal(cnt, oc)
            for got, (c, it, r) in zip(res.em, exp["em"]):
                assert [(a, p) for a, p in got["result"]] == [(a, p) for a, p in r]       # the same doubles
            if mx * len(unit) <= 70:                 # a 100-bp read can span the whole array: the call must be right too
                assert sorted(a for a, _ in res.gene_prob[:2]) == sorted(sample)
            pl.close()
    finally:
        ex.shutdown(cancel_futures=True)
    assert total_reads >= 0.99 * CODIS_READS
