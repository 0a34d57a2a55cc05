"""The gapped consensus' oracle (tests/gapped_oracle.py) on hand-worked cases, its identities, and the wrapper's restatement of the call
rule over numpy arrays (mitofilter.gapped_consensus), which needs no device, against it."""
import functools

import numpy as np
import pytest

from tests import align_oracle as ao
from tests import gapped_data as gd
from tests import gapped_oracle as go
from tests import pileup_oracle as pio
from tests import place_oracle as po

CONS = b"ACGTAC"


def one_record(depth=4, span=4):
    return np.full(6, depth, np.int64), np.zeros(6, np.int64), np.zeros((6, span, 4), np.int64)


def wrapper_call(depth, dels, pile, min_depth, starts=(0, 6), cons=CONS):
    from mitoflex_amd import mitofilter as mf
    indels = np.zeros(len(depth), dtype=mf.INDEL)
    indels["del"] = dels
    ins = np.zeros(pile.shape[:2], dtype=mf.PILEUP)
    for i, f in enumerate("acgt"):
        ins[f] = pile[:, :, i]
    g, s, r = mf.gapped_consensus(np.array(starts, np.uint64), depth.astype(np.uint32), indels, ins, np.frombuffer(cons, np.uint8), min_depth)
    return bytes(g), [int(v) for v in s], [[int(r[f][j]) for f in ("length", "deleted", "insertions", "inserted_bases")] for j in range(len(r))]


def both(depth, dels, pile, min_depth=1, starts=(0, 6), cons=CONS):
    want = go.call(list(starts), depth, dels, cons, pile, min_depth)
    assert wrapper_call(depth, dels, pile, min_depth, starts, cons) == want
    for (length, deleted, _, inserted), lo, hi in zip(want[2], starts[:-1], starts[1:]):
        assert length == (hi - lo) - deleted + inserted
    return want


# ------------------------------------------------------------------ the call, hand-worked
@pytest.mark.parametrize("carriers,called", [(4, True), (2, False), (3, True), (1, False)])
def test_an_insertion_needs_more_than_half_of_the_covering_reads(carriers, called):
    depth, dels, pile = one_record()
    pile[2, 0, 2] = pile[2, 1, 3] = carriers                       # "GT" behind position 2
    g, starts, recs = both(depth, dels, pile)
    assert g == (b"ACGGTTAC" if called else b"ACGTAC") and starts == [0, len(g)]
    assert recs == [[8, 0, 1, 2] if called else [6, 0, 0, 0]]


def test_two_letters_tied_at_one_offset_give_n():
    depth, dels, pile = one_record()
    pile[2, 0, 0] = pile[2, 0, 1] = 2                               # 2 A and 2 C: all four reads insert, no letter leads
    pile[2, 1, 3], pile[2, 1, 0] = 3, 1
    assert both(depth, dels, pile)[0] == b"ACGNTTAC"


def test_emission_stops_at_the_first_column_that_is_not_carried():
    depth, dels, pile = one_record()
    pile[2, 0, 2], pile[2, 1, 2], pile[2, 2, 2] = 4, 2, 4
    g, _, recs = both(depth, dels, pile)
    assert g == b"ACGGTAC" and recs == [[7, 0, 1, 1]]


@pytest.mark.parametrize("dels_at_3,deleted", [(2, False), (3, True), (4, True)])
def test_a_deletion_at_exactly_half_is_not_called(dels_at_3, deleted):
    depth, dels, pile = one_record()
    dels[3] = dels_at_3
    g, _, recs = both(depth, dels, pile)
    assert g == (b"ACGAC" if deleted else b"ACGTAC") and recs[0][1] == int(deleted)


def test_an_insertion_behind_a_deleted_position():
    depth, dels, pile = one_record()
    dels[2] = 4
    pile[2, 0, 3] = 4
    g, _, recs = both(depth, dels, pile)
    assert g == b"ACTTAC" and recs == [[6, 1, 1, 1]]


def test_nothing_is_called_below_min_depth_and_two_records_keep_their_offsets():
    depth, dels, pile = one_record(depth=2)
    dels[1] = 2
    pile[4, 0, 0] = 2
    assert both(depth, dels, pile, min_depth=3, cons=b"acgtac")[0] == b"acgtac"
    g, starts, recs = both(depth, dels, pile, min_depth=2, starts=(0, 2, 6), cons=b"ACGTAC")
    assert g == b"AGTAAC" and starts == [0, 1, 6] and recs == [[1, 1, 0, 0], [5, 0, 1, 1]]


def test_band_0_has_no_column_and_deletes_nothing():
    depth, dels, _ = one_record()
    dels[:] = 4
    g, starts, recs = both(depth, dels, np.zeros((6, 0, 4), np.int64))
    assert g == CONS and starts == [0, 6] and recs == [[6, 0, 0, 0]]


# ------------------------------------------------------------------ the pile, hand-worked over steps
def test_an_inserted_n_keeps_its_offset_and_counts_nowhere():
    pile = np.zeros((10, 4, 4), np.int64)
    steps = [(ao.DIAG, 0, 4), (ao.INS, 1, 5), (ao.INS, 2, 5), (ao.INS, 3, 5), (ao.DIAG, 4, 5)]
    go.pile_steps(pile, "ACNTG", steps, 0, 10, 4)
    assert pile.sum() == 2 and pile[4, 0, 1] == 1 and pile[4, 2, 3] == 1 and not pile[4, 1].any()


def test_runs_behind_the_last_position_count_and_before_the_first_do_not():
    pile = np.zeros((12, 2, 4), np.int64)                           # a record of 5 positions at s0 = 3 of the bait
    steps = [(ao.INS, 0, 0), (ao.DIAG, 1, 0), (ao.DIAG, 2, 4), (ao.INS, 3, 5), (ao.INS, 4, 5), (ao.DIAG, 5, 5), (ao.INS, 6, 6)]
    go.pile_steps(pile, "TACGGAT", steps, 3, 5, 2)
    assert pile.sum() == 2 and pile[7, 0, 2] == 1 and pile[7, 1, 2] == 1          # only the run between positions 4 and 5 (column 5)


def test_a_deletion_between_two_insertions_makes_two_runs():
    pile = np.zeros((10, 2, 4), np.int64)
    steps = [(ao.INS, 0, 3), (ao.DEL, 1, 3), (ao.INS, 1, 4), (ao.DIAG, 2, 4)]
    go.pile_steps(pile, "ACG", steps, 0, 10, 2)
    assert pile[2, 0, 0] == 1 and pile[3, 0, 1] == 1 and pile.sum() == 2


# ------------------------------------------------------------------ through the alignment oracle
@functools.lru_cache(maxsize=None)
def reconstructed(k, band):
    bait, sample, reads = gd.reconstruction(band)
    o = po.PlaceOracle(">g\n" + bait + "\n", k)
    return bait, sample, reads, o, go.GappedOracle(o).run(reads, o.tally(reads), 1, 1000, band, 3)


def test_the_oracle_reconstructs_the_sample():
    from mitoflex_amd import mitofilter as mf
    bait, sample, reads, o, want = reconstructed(31, 8)
    assert want["accepted"].all()
    g = want["gapped"].decode()
    assert g.upper() == sample and want["gapped_starts"] == [0, len(sample)]
    # (the five inserted bases may lie behind more than one position: a chance match inside the stretch is a diagonal step)
    length, deleted, insertions, inserted = want["gapped_records"][0]
    assert (length, deleted, inserted) == (len(sample), 3, 5) and 1 <= insertions <= 5
    assert (want["ins_pile"].sum(axis=(1, 2)) == want["indels"][:, 2]).all()          # no inserted base is an N
    depth, indels, ins = gd.structured(mf, want, 8)
    cons, _ = pio.PileupOracle(o).call(want["counts"], 3)
    got = mf.gapped_consensus(np.array(o.starts, np.uint64), depth, indels, ins, cons, 3)
    assert bytes(got[0]) == want["gapped"] and got[1].tolist() == want["gapped_starts"]
    assert [[int(got[2][f][0]) for f in ("length", "deleted", "insertions", "inserted_bases")]] == want["gapped_records"]
    # band 0: the pile-up oracle's consensus
    w0 = go.GappedOracle(o).run(reads, o.tally(reads), 1, 1000, 0, 3)
    assert w0["gapped"] == bytes(pio.PileupOracle(o).call(w0["counts"], 3)[0]) and w0["gapped_starts"] == [int(s) for s in o.starts]


def test_stacks_carried_by_half_and_by_one_more():
    from mitoflex_amd import mitofilter as mf
    bait = gd.stack_bait()
    o = po.PlaceOracle(">s\n" + bait + "\n", 31)
    G = go.GappedOracle(o)
    for carriers, called in ((250, False), (251, True)):
        reads = gd.stack_reads(bait, carriers, 250)
        want = G.run(reads, o.tally(reads), 1, 1000, 8, 1)
        assert want["accepted"].all()
        assert want["gapped_records"] == [[604, 0, 1, 4] if called else [600, 0, 0, 0]]
        assert want["gapped"].decode().upper() == (bait[:250] + "TCCT" + bait[250:] if called else bait)
        depth, indels, ins = gd.structured(mf, want, 8)
        got = mf.gapped_consensus(np.array(o.starts, np.uint64), depth, indels, ins, pio.PileupOracle(o).call(want["counts"], 1)[0], 1)
        assert bytes(got[0]) == want["gapped"]
    reads = gd.stack_reads(bait, 250, 0, other="TGCT", n_other=250)
    want = G.run(reads, o.tally(reads), 1, 1000, 8, 1)
    assert want["gapped"].decode().upper() == bait[:250] + "TNCT" + bait[250:]
