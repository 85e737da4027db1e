"""The plain-Python statement of the pair-aware placement (tests/align_pair_ref.py) pinned: on hand-made families against records
written down by hand, against the independent statement (tests/align_ref.py) where the rule must not change anything, and with
prune=True against prune=False.  No GPU, no native code."""
import pytest

import align_cases
import align_pair_cases
import align_pair_ref
import align_ref

HAND = {c[0]: c for c in align_pair_cases.hand_cases()}


@pytest.mark.parametrize("key", align_pair_cases.HAND_IDS)
def test_hand_cases(key):
    _, loci, m1, m2, frag, expected = HAND[key]
    reads = [[(n, s, None) for n, s in m] for m in (m1, m2)]
    text = align_pair_ref.align_text(loci, reads, 2, frag)
    assert align_pair_cases.fields(text) == expected
    assert text.encode() == align_pair_cases.ref_text(key)
    assert align_pair_ref.counters(loci, reads, 2, frag) == align_pair_cases.HAND_COUNTERS[key]


def test_what_the_independent_placement_writes_on_the_two_confirmed_cases():
    """The records the pair rule is there to change: NH 2 on the ambiguous mate, DP on the rescued pair."""
    _, loci, m1, m2, frag, _ = HAND["ambiguous"]
    text = align_ref.align_text(loci, [[(n, s, None) for n, s in m] for m in (m1, m2)], 2, frag)
    assert align_pair_cases.fields(text) == [(99, "P*BACKBONE", 1101, 0, 2, "CP"), (147, "P*BACKBONE", 1501, 0, 1, "CP")]
    _, loci, m1, m2, frag, _ = HAND["rescue"]
    text = align_ref.align_text(loci, [[(n, s, None) for n, s in m] for m in (m1, m2)], 2, frag)
    assert align_pair_cases.fields(text) == [(97, "Q*BACKBONE", 401, 0, 1, "DP"), (145, "P*BACKBONE", 1501, 0, 1, "DP")]


def test_below_the_fragment_edge_the_records_are_the_independent_ones():
    _, loci, m1, m2, frag, _ = HAND["edge-below"]
    reads = [[(n, s, None) for n, s in m] for m in (m1, m2)]
    assert align_pair_ref.align_text(loci, reads, 2, frag) == align_ref.align_text(loci, reads, 2, frag)
    assert align_pair_ref.align_text(loci, reads, 2, frag + 1) != align_ref.align_text(loci, reads, 2, frag + 1)


def test_many_placements_count_the_copies_inside_the_fragment_limit():
    loci, w, m2 = align_pair_cases.many(30, 28)
    reads = [[("m", w, None)], [("m", m2, None)]]
    assert align_ref.align_read(loci, w, 2)[2] == 30
    for frag, nh in ((39, 1), (39 * 2, 2), (39 * 28, 28), (39 * 28 - 1, 27), (5000, 28)):       # copy j: 39 * (28 - j) <= max_fragment
        got = align_pair_cases.fields(align_pair_ref.align_text(loci, reads, 2, frag))
        assert [g[4] for g in got] == [nh, nh] and got[0][5] == "CP", (frag, got)


def test_the_triangle_of_placement_pairs():
    """Both mates are the word that stands 40 times: (copy j1, copy j2) is concordant iff 0 <= j2 - j1 <= 9."""
    got = align_pair_cases.fields(align_pair_cases.ref_text("triangle"))
    nh = sum(1 for a in range(40) for b in range(40) if 0 <= b - a <= 9)
    assert got == [(99, "R1*BACKBONE", 24, 0, nh, "CP"), (147, "R1*BACKBONE", 24, 0, nh, "CP")]


def test_single_end_input_is_untouched():
    d, texts, me, frag = align_pair_cases.inputs()["mixed-single"]
    loci = align_ref.loci_from_dicts(*d)
    reads = [align_ref.read_records(t) for t in texts]
    assert align_pair_cases.ref_text("mixed-single").decode() == align_ref.align_text(loci, reads, me, frag)
    assert align_pair_cases.ref_counters("mixed-single") == (0, 0, 0)


def test_one_mate_pairs_beside_rescued_ones():
    got = align_pair_cases.fields(align_pair_cases.ref_text("mixed"))
    P = "P*BACKBONE"
    assert got == [(99, P, 1101, 1, 1, "CP"), (147, P, 1501, 0, 1, "CP"), (153, P, 1501, 0, 1, "UP"),
                   (99, P, 1101, 1, 1, "CP"), (147, P, 1701, 0, 1, "CP"), (73, P, 1101, 0, 1, "UP"),
                   (99, P, 1151, 0, 1, "CP"), (147, P, 1501, 0, 1, "CP")]
    assert align_pair_cases.ref_counters("mixed") == (3, 3, 2)


PAIRED = align_pair_cases.PAIRED


def test_these_are_the_paired_inputs():
    assert PAIRED == [k for k in align_cases.INPUT_IDS if len(align_cases.inputs()[k][1]) == 2]


@pytest.mark.parametrize("key", PAIRED)
def test_pairs_the_rule_must_leave_alone(key):
    """Every paired input of the independent suites: a pair whose two independent NH are 1 is written as before; and where the
    independent picks are already concordant the pair's alignment is those picks (only NH can change)."""
    d, texts, me = align_cases.inputs()[key]
    loci = align_ref.loci_from_dicts(*d)
    reads = [align_ref.read_records(t) for t in texts]
    assert len(reads) == 2
    n_both_unique = 0
    for k, (alns, placed) in enumerate(align_pair_ref.align_pairs(loci, reads, me)):
        ind = [align_ref.align_read(loci, reads[m][k][1], me) for m in range(2)]
        if ind[0] is None or ind[1] is None:
            assert list(alns) == ind and not placed
            continue
        if ind[0][2] == 1 and ind[1][2] == 1:
            n_both_unique += 1
            assert list(alns) == ind, (key, k)
        if align_pair_ref.concordant(ind[0][0], ind[0][1], ind[1][0], ind[1][1], 1000):
            assert placed and [a[:2] for a in alns] == [a[:2] for a in ind], (key, k)
    if key.startswith("pairs-"):
        assert n_both_unique == 6 and align_pair_ref.align_text(loci, reads, me).encode() == align_cases.ref_text(key)
    assert n_both_unique > 0 or key == "empty-pair"


@pytest.mark.parametrize("key", align_pair_cases.INPUT_IDS)
def test_the_pruned_statement_is_the_exhaustive_one(key):
    d, texts, me, frag = align_pair_cases.inputs()[key]
    loci = align_ref.loci_from_dicts(*d)
    reads = [align_ref.read_records(t) for t in texts]
    assert align_pair_ref.align_text(loci, reads, me, frag, prune=True).encode() == align_pair_cases.ref_text(key)
