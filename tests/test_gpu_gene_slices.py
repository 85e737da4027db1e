"""The sliced launches of the gene side (csrc/hgx_dedup.hip: insert, exact check, gather; csrc/hgx_counts.hip: Gene_counts) against
the Python-dict reference (tests/dedup_ref.py) and against the whole launches.  `gene_slices` = N forces N launches of each kernel
at the C entry points; N = 1 is the whole launch.  Hand-built rows put what can go wrong with a cut where it would show: a class
spread over all slices, classes founded by the first and by the last row of a slice, an allele whose first class lies in the last
slice only, and a forged key collision whose odd row is checked in another slice than the one that founded its slot.  Integers and
bit rows only: every comparison is `==`."""
import numpy as np
import pytest

import dedup_ref as dr
import golden_util as gu
import hisatgenotype_amd as hgx
from hisatgenotype_amd import engine, locus as hl

pytestmark = pytest.mark.gpu

SLICES = [1, 2, 3, 7, 1000]            # 1000: more slices than workgroups at every size below (4097 rows = 257 check workgroups)
ROWS = [1, 1023, 1024, 1025, 4097]     # a slice end inside, at and just past an insert workgroup (1024 rows) and a scan tile (4096)
W64 = [8, 72]
ODD_KEY = 0x9E3779B97F4A7C15


def _bounds(n_wg, per_wg, n, slices):
    """row ranges of the launches: <= `slices` consecutive non-empty ranges of the n_wg workgroups (hgx_for_slices)"""
    s = max(1, min(slices, n_wg))
    cut = [k * n_wg // s for k in range(s + 1)]
    return [(cut[k] * per_wg, min(n, cut[k + 1] * per_wg)) for k in range(s) if cut[k + 1] > cut[k]]


def _case(n, w64):
    """-> (rows, keys): rows with the textures of the module docstring; keys honest (None) except for the forged pair.
    Labels: 0 = the hot class (every fifth row: in every slice of every N), 1.. = classes founded at the first / last row of every
    slice of N = 2, 3, 7 (insert and check granularity), the rest distinct rows or repeats of earlier ones."""
    rng = np.random.RandomState(n * 131 + w64)
    rows = rng.randint(0, 256, size=(n, 8 * w64)).astype(np.uint8).view(np.uint64).reshape(n, w64)       # all distinct to begin with
    rows[:, w64 - 1] &= np.uint64(0x7FFFFFFFFFFFFFFF)       # allele 64 * w64 - 1: set below, in the last class only
    rows[:, 0] &= ~np.uint64(2)                             # allele 1: in no class
    edge = set()
    for N in (2, 3, 7):
        for per, wg in ((1024, (n + 1023) // 1024), (16, (n + 15) // 16)):
            for r0, r1 in _bounds(wg, per, n, N):
                edge.update((r0, r1 - 1))
    hot = rows[0].copy()
    for i in range(0, n, 5):
        if i not in edge or i == 0:
            rows[i] = hot
    for i in range(n):                                      # a third of the other rows repeat an earlier row (classes across slices)
        if i % 5 and i not in edge and i % 3 == 0 and i > 7:
            rows[i] = rows[rng.randint(0, i)]
    if n > 1:
        rows[n - 1, w64 - 1] |= np.uint64(1) << np.uint64(63)       # the last row founds the last class, the only one with this allele
    return rows


def _run(rows, keys, n_slices):
    """dedup + Gene_counts with `gene_slices` forced -> (bits, counts, first rows, Gene_counts, first classes)"""
    n, w64 = rows.shape
    with engine.test_switches(gene_slices=n_slices):
        d_rows = engine.DevArray.from_host(rows)
        d_keys = engine.DevArray.from_host(keys) if keys is not None else None
        cl = engine.Classes.dedup(d_rows, n, 64 * w64, hashes=d_keys)
        out = cl.to_host()
        cnt, first = cl.allele_counts() if cl.n_classes else (np.zeros(64 * w64, np.int64), np.full(64 * w64, -1, np.int32))
        cl.close()
    return out + (cnt, first.astype(np.int64))


def _check(rows, keys):
    want = dr.dedup_ref(rows)
    want_c, want_f = dr.counts_ref(want[0], want[1])
    whole = None
    for N in SLICES:
        got = _run(rows, keys, N)
        for name, g, w in zip(("class rows", "counts", "first rows", "Gene_counts", "first classes"), got, want + (want_c, want_f)):
            assert g.shape == w.shape and np.array_equal(g, w), (name, N)
        if whole is None:
            whole = got
        for name, g, w in zip(("class rows", "counts", "first rows", "Gene_counts", "first classes"), got, whole):
            assert np.array_equal(g, w), (name, N, "against N = 1")
    return want, want_f


@pytest.mark.parametrize("w64", W64)
@pytest.mark.parametrize("n_rows", ROWS)
def test_sliced_dedup_and_counts_equal_the_reference_and_the_whole_launch(n_rows, w64):
    rows = _case(n_rows, w64)
    (bits, cnt, first), first_class = _check(rows, None)
    if n_rows >= 1023:
        assert cnt[0] >= n_rows // 5 - 40                    # the hot class: a fifth of the rows
        for N in (2, 3, 7):                                  # ... with rows in every slice of both granularities
            for per in (1024, 16):
                for r0, r1 in _bounds((n_rows + per - 1) // per, per, n_rows, N):
                    assert r1 - r0 < 5 or np.any(np.all(rows[r0:r1] == rows[0], axis=1)), (N, per, r0)
                    assert r0 in first and (r1 - 1 in first or r1 - 1 == n_rows - 1)       # classes founded at both ends of a slice
        a = 64 * w64 - 1
        assert first_class[a] == len(cnt) - 1 and first[-1] == n_rows - 1     # an allele first seen in the last class (last slice)
        assert first_class[1] == -1


@pytest.mark.parametrize("w64", W64)
@pytest.mark.parametrize("n_rows", [1025, 4097])
def test_forged_collision_across_slices(n_rows, w64):
    """Two DIFFERENT contents under one supplied key: the majority founds the slot at row 2 (the first slice of every N), the odd
    row is the last one (the last slice of every N > 1): its check reads a first row that another slice's insert wrote, and the
    whole dedup goes through the re-keying rounds."""
    rows = _case(n_rows, w64)
    keys = np.arange(1, n_rows + 1).astype(np.uint64) * np.uint64(0x2545F4914F6CDD1D)      # honest: distinct rows, distinct keys ...
    _, inv = np.unique(rows, axis=0, return_inverse=True)
    first_of = {}
    for i, c in enumerate(inv.ravel().tolist()):
        first_of.setdefault(c, i)
        keys[i] = keys[first_of[c]]                                                      # ... equal rows, equal keys
    assert dr.EMPTY not in keys.tolist()
    odd = n_rows - 1
    assert first_of[int(inv.ravel()[odd])] == odd and first_of[int(inv.ravel()[2])] == 2      # distinct from all rows before them
    members = np.all(rows == rows[2], axis=1)
    keys[members] = np.uint64(ODD_KEY)
    keys[odd] = np.uint64(ODD_KEY)
    _check(rows, keys)


def test_gather_in_slices_beyond_the_one_round_trip_size():
    """Above 65 536 rows the class rows are gathered per class (k_ht_gather), the launch that is cut over class ranges."""
    rows, _, _, _ = dr.make("random", 70001, 8, seed=3)
    _check(rows, None)


def test_type_locus_with_five_slices_equals_the_default():
    """A golden HLA fixture large enough for the gene side to run beside EM #1: every result array with gene_slices = 5 equals the
    default's."""
    fx = gu.load("hla_7000_10k")
    o = fx["options"]
    pl = hl.PackedLocus.from_synth(fx["_locus"])

    def run():
        return hgx.type_locus(pl, fx["sam"], num_editdist=o["num_editdist"], error_correction=o["error_correction"],
                              allow_discordant=o["allow_discordant"], remove_low_abundance_alleles=o["remove_low"],
                              simulation=o["simulation"], keep_classes=True)
    base = run()
    with engine.test_switches(gene_slices=5):
        got = run()
    assert (got.num_reads, got.num_pairs) == (base.num_reads, base.num_pairs)
    assert np.array_equal(got.counts, base.counts) and np.array_equal(got.counts_order, base.counts_order)
    for g, b in ((got.exon_classes, base.exon_classes), (got.gene_classes, base.gene_classes)):
        assert (g is None) == (b is None)
        if g is not None:
            assert np.array_equal(g[0], b[0]) and np.array_equal(g[1], b[1])
    assert got.em == base.em and got.gene_prob == base.gene_prob
