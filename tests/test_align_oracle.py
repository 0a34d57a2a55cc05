"""The plain-Python oracle of the banded alignment (tests/align_oracle.py) held to the rule of include/mitofilter.h: hand-worked cases
whose traceback is written out here, band 0 against the verification oracle, the row-at-a-time restatement against the cell-at-a-time
one, the theorem that one indel of g <= W bases costs at most g edits on the longer side's diagonal, and -- for the inputs the GPU tests
use -- that placement's oracle places the simulated indel reads."""
import random

import numpy as np
import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import place_oracle as po
from tests import verify_oracle as vo

M, D, I = ao.DIAG, ao.DEL, ao.INS


def cigar(steps):
    out = []
    for mv, _, _ in steps:
        if out and out[-1][0] == mv:
            out[-1][1] += 1
        else:
            out.append([mv, 1])
    return "".join("%d%s" % (n, mv) for mv, n in out)


def both(x, rec, start, W):
    a, b = ao.align(x, rec, start, W), ao.align_fast(x, rec, start, W)
    assert a == b
    return a


def counts(a):
    return a["compared"], a["mismatches"], a["insertions"], a["deletions"], a["ref_begin"], a["ref_end"]


def test_a_deletion_inside_a_homopolymer_goes_to_its_first_position():
    rec = "CGTC" + "AAAAAAAA" + "GCTG"
    x = "CGTC" + "AAAAAAA" + "GCTG"                                # one A fewer
    a = both(x, rec, 0, 2)
    # from (15, 16) the diagonal reproduces every cell down to (5, 6); at (4, 5) C on A does not, the deletion from (4, 4) does
    assert cigar(a["steps"]) == "4M1D11M"
    assert a["steps"][4] == (D, 4, 4)                               # bait position 4, the first A, in row 4
    assert a["steps"][3] == (M, 3, 3) and a["steps"][5] == (M, 4, 5) and a["steps"][-1] == (M, 14, 15)
    assert counts(a) == (15, 0, 0, 1, 0, 16)


def test_an_insertion_in_a_dinucleotide_repeat_goes_to_its_first_unit():
    rec = "GATC" + "TATATATA" + "CGGA"
    x = "GATC" + "TATATATATA" + "CGGA"                             # one TA more
    a = both(x, rec, 0, 2)
    # the end cell is (18, 16); the diagonal holds down to (6, 4), where A on C does not and (5, 4) + 1 does; (5, 4) likewise from (4, 4)
    assert cigar(a["steps"]) == "4M2I12M"
    assert a["steps"][4:6] == [(I, 4, 4), (I, 5, 4)]                # read bases 4 and 5 between bait positions 3 and 4
    assert a["steps"][6] == (M, 6, 4) and a["steps"][-1] == (M, 17, 15)
    assert counts(a) == (16, 0, 2, 0, 0, 16)
    assert ao.insertion_runs(a["steps"]) == [(4, 2)]


def test_an_indel_within_the_band_of_a_read_end_ties_with_mismatches_and_the_diagonal_wins():
    rec = "GCTAGGATCCATGCAAGTCTAGACCGTTAGACGTTCAGGA"
    assert rec[30:32] == "AC" and rec[32:34] == "GT"
    x = rec[0:30] + rec[32:34]                                      # two bases deleted two bases before the read's end
    a = both(x, rec, 0, 4)
    # D(32, 34) = 2 by two deletions and D(32, 32) = 2 by two mismatches: the end cell is the one on the placement's diagonal
    assert cigar(a["steps"]) == "32M" and counts(a) == (32, 2, 0, 0, 0, 32)
    # the same at the read's begin: x = rec[8:10] + rec[12:40] placed by its longer side at 10; (2, 12) is 2 by the diagonal, taken first
    assert rec[8:10] == "CC" and rec[10:12] == "AT"
    x = rec[8:10] + rec[12:40]
    a = both(x, rec, 10, 4)
    assert cigar(a["steps"]) == "30M" and counts(a) == (30, 2, 0, 0, 10, 40)
    # one base more of read behind the deletion and the gap is cheaper than the mismatches
    assert rec[32:35] == "GTT" and rec[30:33] == "ACG"
    x = rec[0:30] + rec[32:35]
    a = both(x, rec, 0, 4)
    assert cigar(a["steps"]) == "30M2D3M" and counts(a) == (33, 0, 0, 2, 0, 35)
    assert a["steps"][30:32] == [(D, 30, 30), (D, 30, 31)]


def test_a_read_over_both_record_ends_compares_only_inside():
    rec = "ACGGTCATTGCAAGCTTAGC"
    x = "TTGCA" + rec + "GGACT"
    a = both(x, rec, -5, 3)
    assert cigar(a["steps"]) == "30M" and counts(a) == (20, 0, 0, 0, -5, 25)
    # an N in the read and one in the record are not compared either
    a = both("TTGCA" + rec[:7] + "N" + rec[8:] + "GGACT", rec[:3] + "N" + rec[4:], -5, 3)
    assert cigar(a["steps"]) == "30M" and counts(a) == (18, 0, 0, 0, -5, 25)


def test_the_fast_restatement_is_the_plain_one():
    rng = random.Random(3)
    for _ in range(150):
        rec = "".join(rng.choices("ACGTN" if rng.random() < 0.2 else "ACGT", k=rng.randint(30, 120)))
        L = rng.randint(5, 90)
        a = rng.randrange(-10, max(len(rec) - L // 2, 1))
        x = "".join(rec[c] if 0 <= c < len(rec) and rng.random() < 0.9 else rng.choice("ACGTN") for c in range(a, a + L))
        if rng.random() < 0.6:
            x = ad.with_indel(rng, x, rng.randrange(L), rng.randint(1, 5), rng.random() < 0.5)
        both(x, rec, a, rng.choice((0, 1, 2, 4, 8, 31)))


def test_one_indel_of_g_bases_costs_at_most_g_edits():
    rng = random.Random(11)
    W = 8
    for _ in range(300):
        rec = "".join(rng.choices("ACGT", k=400))
        L, g = rng.randint(60, 200), rng.randint(1, W)
        a = rng.randrange(20, 150)
        at = L // 3 if rng.random() < 0.5 else L - L // 3
        insert = rng.random() < 0.5
        x = ad.with_indel(rng, rec[a:a + L + 10], at, g, insert)[:L]
        # the longer side's diagonal: the part before the indel when it lies behind the middle, else the part behind it
        start = a if at > L // 2 else (a - g if insert else a + g)
        al = ao.align_fast(x, rec, start, W)
        assert al["mismatches"] + al["insertions"] + al["deletions"] <= g, (L, g, at, insert, counts(al))


@pytest.fixture(scope="module")
def placed():
    text, parts = ad.align_bait()
    seqs, groups = ad.ragged_reads(parts)
    o = po.PlaceOracle(text, 31)
    return o, seqs, groups, o.tally(seqs)


def test_band_0_is_the_verification_oracle(placed):
    o, seqs, groups, tallies = placed
    A, V = ao.AlignOracle(o), vo.VerifyOracle(o)
    for max_permille in (1000, 30, 0):
        got, want = A.run(seqs, tallies, 1, max_permille, 0), V.verify(seqs, tallies, 1, max_permille)
        assert np.array_equal(got["aligns"][:, :2], want["scores"]) and not got["aligns"][:, 2:4].any()
        on = got["rows"][:, 0] < po.AMBIGUOUS
        assert np.array_equal(got["aligns"][on, 4:], got["rows"][on, 2:4])
        for f in ("passes", "rows", "accepted", "depth", "place_rec", "counts"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["align_rec"][:, [0, 1, 2, 3]], want["score_rec"][:, :4]) and np.array_equal(got["align_rec"][:, 7:], want["score_rec"][:, 4:])
        assert not got["indels"].any() and not got["align_rec"][:, 4:7].any() and got["unplaced"] == want["unplaced"]


def test_the_oracle_places_the_simulated_indel_reads(placed):
    o, seqs, groups, tallies = placed
    for k in (21, 31, 41):
        ok = po.PlaceOracle(ad.align_bait()[0], k) if k != 31 else o
        lo, hi = groups["indel"]
        rows = ok.place(ok.tally(seqs[lo:hi]), 1)[1]
        assert (rows[:, 0] < po.AMBIGUOUS).mean() >= 0.9, k


def test_the_band_recovers_the_indel_reads(placed):
    o, seqs, groups, tallies = placed
    lo, hi = groups["indel"]
    part, gs = ad.indel_reads(ad.align_bait()[1], 500, 8)
    assert part == seqs[lo:hi]
    A = ao.AlignOracle(o)
    rows = o.place(tallies[lo:hi], 1)[1]
    n = 0
    for seq, row, g in zip(part, rows, gs):
        a = A.align_row(seq, row, 8)
        if a is not None:
            n += 1
            assert a["mismatches"] + a["insertions"] + a["deletions"] <= g
    assert n >= 450
