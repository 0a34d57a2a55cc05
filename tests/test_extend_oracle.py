"""The oracle of the extended records (tests/extend_oracle.py) against hand-worked cases, written out column by column from the rule in
include/mitofilter.h, and against the rule's invariant on the `ends` set.  No device."""
import numpy as np
import pytest

from tests import align_oracle as ao
from tests import extend_data as xd
from tests import extend_oracle as xo
from tests import place_oracle as po

#      0         1         2         3
#      0123456789012345678901234567890123456789
REC = "ACGGTCATTGCAAGCTTAGCCATGACCTAGGATCCGTATC"
A, C, G, T = 0, 1, 2, 3


def piled(reads, E, W=0):
    """the reads (oriented sequence, start) aligned to REC and piled: -> (ext int[1, 2, E, 4], their alignments)"""
    ext = np.zeros((1, 2, E, 4), np.int64)
    als = []
    for x, start in reads:
        a = ao.align(x, REC, start, W)
        xo.pile_steps(ext, x, a["steps"], 0, len(REC), E)
        als.append(a)
    return ext, als


# three reads on the 40-base record.  Their columns, record coordinate above oriented read base:
#   read 1, start -3      c  -3 -2 -1  0  1 ..  9          begin offsets 2, 1, 0: T, T, G
#                            T  T  G  A  C ..  G
#   read 2, start 32      c  32 .. 39 40 41                end offsets 0, 1: A, C
#                            T ..  C  A  C
#   read 3, start -2      c  -2 -1  0 .. 11                begin offset 1: an N, nowhere; offset 0: G
#                            N  G  A ..  A
THREE = (("TTG" + REC[:10], -3), (REC[32:] + "AC", 32), ("NG" + REC[:12], -2))


def test_three_reads_on_a_40_base_record():
    assert len(REC) == 40
    ext, als = piled(THREE, 4)
    assert [(a["ref_begin"], a["ref_end"]) for a in als] == [(-3, 10), (32, 42), (-2, 12)]
    want = np.zeros((1, 2, 4, 4), np.int64)
    want[0, xo.BEGIN, 0, G] = 2
    want[0, xo.BEGIN, 1, T] = 1
    want[0, xo.BEGIN, 2, T] = 1
    want[0, xo.END, 0, A] = 1
    want[0, xo.END, 1, C] = 1
    assert np.array_equal(ext, want)
    body = REC.lower().encode()                                    # (a gapped consensus below min_depth: the bait's letters in lower case)
    assert xo.call(body, [0, 40], ext, 1) == (b"TTG" + body + b"AC", [0, 45], [[45, 3, 2, 4, 2]])
    assert xo.call(body, [0, 40], ext, 2) == (b"G" + body, [0, 41], [[41, 1, 0, 4, 2]])          # the begin stops at its second column, the end at its first
    assert xo.call(body, [0, 40], ext, 3) == (body, [0, 40], [[40, 0, 0, 4, 2]])


def test_extend_1_and_2_drop_the_farther_columns():
    e1, _ = piled(THREE, 1)
    assert e1.shape == (1, 2, 1, 4) and e1[0, xo.BEGIN, 0].tolist() == [0, 0, 2, 0] and e1[0, xo.END, 0].tolist() == [1, 0, 0, 0]
    body = REC.encode()
    assert xo.call(body, [0, 40], e1, 1) == (b"G" + body + b"A", [0, 42], [[42, 1, 1, 2, 1]])
    e2, _ = piled(THREE, 2)
    assert int(e2.sum()) == 5 and xo.call(body, [0, 40], e2, 1)[0] == b"TG" + body + b"AC"


def test_extend_larger_than_any_overhang():
    e4, _ = piled(THREE, 4)
    big, _ = piled(THREE, 4096)
    assert np.array_equal(big[:, :, :4], e4) and not big[:, :, 4:].any()
    body = REC.encode()
    assert xo.call(body, [0, 40], big, 1) == xo.call(body, [0, 40], e4, 1)


def test_a_tie_stops_the_end_and_emits_nothing():
    reads = ((REC[30:] + "ACG", 30), (REC[30:] + "ATG", 30))
    ext, _ = piled(reads, 8)
    assert ext[0, xo.END, :3].tolist() == [[2, 0, 0, 0], [0, 1, 0, 1], [0, 0, 2, 0]]
    body = REC.encode()
    assert xo.call(body, [0, 40], ext, 1) == (body + b"A", [0, 41], [[41, 0, 1, 0, 6]])          # no N, and the G behind the tie is not reached
    assert xo.call_end(ext[0, xo.END], 2) == "A" and xo.call_end(ext[0, xo.END], 3) == ""


def test_an_insertion_inside_the_end_moves_the_overhang_to_another_diagonal():
    """band 2: two bases inserted 5 positions inside the record's end; the four overhanging bases lie on the diagonal two below the
    placement's, at end offsets 0 .. 3, and the inserted bases and a deletion outside the record add nowhere"""
    x = REC[20:35] + "AA" + REC[35:] + "ACGT"
    ext, (a,) = piled(((x, 20),), 8, W=2)
    assert (a["insertions"], a["deletions"], a["mismatches"], a["ref_begin"], a["ref_end"]) == (2, 0, 0, 20, 44)
    assert [(c, x[i]) for mv, i, c in a["steps"] if mv == ao.DIAG and c >= 40] == [(40, "A"), (41, "C"), (42, "G"), (43, "T")]
    assert ext[0, xo.END, :5].tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]] and not ext[0, xo.BEGIN].any()
    # at band 0 the same read lies on the placement's diagonal throughout: the overhang is two columns shorter and other letters
    ext0, (a0,) = piled(((x, 20),), 8, W=0)
    assert a0["ref_end"] == 46 and ext0[0, xo.END].sum() == 6
    # steps that are no diagonal step add nowhere, wherever they lie
    ext = np.zeros((1, 2, 4, 4), np.int64)
    xo.pile_steps(ext, "ACGT", [(ao.INS, 0, -1), (ao.DEL, 1, -2), (ao.INS, 1, 41), (ao.DEL, 2, 41), (ao.DIAG, 2, 41), (ao.DIAG, 3, 44)], 0, 40, 4)
    assert int(ext.sum()) == 1 and ext[0, xo.END, 1, G] == 1                                       # (41 -> offset 1; 44 -> offset 4, not below E)


def test_a_base_beyond_a_record_s_end_stays_with_that_record():
    """records adjacent in global positions: what hangs over record 0's end is not record 1's begin"""
    text, recs, flanks = xd.ends_bait()
    o = po.PlaceOracle(text, 21)
    read = recs[0][-60:] + flanks[0][1][:10]
    X = xo.ExtendOracle(o)
    want = X.run([read], o.tally([read]), 1, 1000, 0, 1, 16)
    assert want["accepted"].all() and int(want["ext_pile"][0, xo.END].sum()) == 10 and int(want["ext_pile"].sum()) == 10
    assert want["extend_records"] == [[310, 0, 10, 0, 10], [200, 0, 0, 0, 0], [400, 0, 0, 0, 0]]
    assert want["extended"][300:310].decode() == flanks[0][1][:10] and want["extended_starts"] == [0, 310, 510, 910]
    assert want["counts"][300:].sum() == 0                         # nothing of it is piled on record 1


@pytest.mark.parametrize("k,band", [(21, 0), (21, 4), (31, 8), (41, 31)])
@pytest.mark.parametrize("E", [1, 16, 64, 4096])
def test_the_invariant(k, band, E):
    text, recs, _ = xd.ends_bait()
    seqs, groups = xd.ends_reads()
    o = po.PlaceOracle(text, k)
    want = xo.ExtendOracle(o).run(seqs, o.tally(seqs), 1, xd.CUT, band, 3, E)
    got, bound = want["ext_pile"].sum(axis=3), xo.overhang_bounds(o, want, E)
    assert got.shape == (3, 2, E) and (got <= bound).all() and int(got.sum()) > 0
    # equal where no overhanging base is an N: without the reads of the `n` group
    clean = [s for i, s in enumerate(seqs) if not groups["n"][0] <= i < groups["n"][1]]
    w2 = xo.ExtendOracle(o).run(clean, o.tally(clean), 1, xd.CUT, band, 3, E)
    assert np.array_equal(w2["ext_pile"].sum(axis=3), xo.overhang_bounds(o, w2, E))
    for r, g in zip(want["extend_records"], want["gapped_records"]):
        assert r[0] == g[0] + r[1] + r[2] and r[1] <= E and r[2] <= E
    assert np.diff(want["extended_starts"]).tolist() == [r[0] for r in want["extend_records"]]
