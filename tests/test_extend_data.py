"""The inputs of the extended-record tests (tests/extend_data.py) held to their conditions from the plain-Python oracle alone, without a
device: the three reconstruction shapes grow the bait into the genome's flanks, and every group of the `ends` set does what it is there
for."""
import functools

import numpy as np
import pytest

from tests import extend_data as xd
from tests import extend_oracle as xo
from tests import place_oracle as po


@pytest.mark.parametrize("shape", xd.SHAPES, ids=lambda s: "k%d_band%d_E%d" % s[:3])
def test_reconstruction_grows_into_the_flanks(shape):
    k, band, E, min_depth, read_len, step = shape
    genome, bait, reads = xd.reconstruction(read_len, step)
    assert bait == genome[xd.BAIT_LO:xd.BAIT_HI] and len(genome) == 1200
    o = po.PlaceOracle(">g\n" + bait + "\n", k)
    want = xo.ExtendOracle(o).run(reads, o.tally(reads), 1, 1000, band, min_depth, E)
    length, nb, ne, _, _ = want["extend_records"][0]
    # the oracle's extension equals the genome's flanks
    assert want["extended"].decode().upper() == genome[xd.BAIT_LO - nb:xd.BAIT_HI + ne] and length == 200 + nb + ne
    assert want["extended"][:nb].isupper() and want["extended"][len(want["extended"]) - ne:].isupper()
    assert min(nb, ne) >= (16 if E == 16 else 32)
    for side, n in ((xo.BEGIN, nb), (xo.END, ne)):
        depth = want["ext_pile"][0, side].sum(axis=1)
        assert depth[n - 1] >= min_depth and (n == E or depth[n] < min_depth)
    if shape == xd.SHAPES[0]:
        assert (len(reads), int(want["accepted"].sum()), nb, ne) == (126, 60, 60, 60)
    # the invariant, with equality: no read holds an N
    assert np.array_equal(want["ext_pile"].sum(axis=3), xo.overhang_bounds(o, want, E))


@functools.lru_cache(maxsize=None)
def ends(k, band, E, uniform=None):
    text, recs, _ = xd.ends_bait()
    seqs, groups = xd.ends_reads(uniform=uniform)
    o = po.PlaceOracle(text, k)
    return recs, seqs, groups, o, xo.ExtendOracle(o).run(seqs, o.tally(seqs), 1, xd.CUT, band, xd.MIN_DEPTH, E)


def test_ends_records_are_adjacent_and_sized():
    text, recs, flanks = xd.ends_bait()
    assert [len(r) for r in recs] == [300, 200, 400] and all(200 <= len(r) <= 400 for r in recs)
    o = po.PlaceOracle(text, 31)
    assert [int(s) for s in o.starts] == [0, 300, 500, 900]          # adjacent in global positions


@pytest.mark.parametrize("k,band", [(21, 0), (31, 8), (41, 31)])
def test_every_group_of_the_ends_set_does_its_work(k, band):
    E = 64
    recs, seqs, groups, o, want = ends(k, band, E)
    rows, al, acc = want["rows"], want["aligns"], want["accepted"]
    lens = [len(r) for r in recs]
    sel = lambda g: range(*groups[g])
    over_b = lambda i: -int(al[i][4])
    over_e = lambda i: int(al[i][5]) - lens[int(rows[i][0])]
    # over: accepted reads overhang every open end on each strand
    for j, side in xd.OPEN_ENDS:
        for strand in (0, 1):
            assert sum(1 for i in sel("over") if acc[i] and int(rows[i][0]) == j and int(rows[i][1]) == strand and (over_b(i), over_e(i))[side] > 0) >= 2, (j, side, strand)
    # far: an overhang beyond E
    assert sum(1 for i in sel("far") if acc[i] and max(over_b(i), over_e(i)) > E) >= 4
    # n: accepted, and the invariant is strict somewhere because of them
    assert sum(1 for i in sel("n") if acc[i]) >= 8
    bound = xo.overhang_bounds(o, want, E)
    got = want["ext_pile"].sum(axis=3)
    assert (got <= bound).all() and int((bound - got).sum()) >= 8
    # tie: emission stops at the tied column although deeper columns follow
    j, side = xd.TIE_END
    table = want["ext_pile"][j, side]
    assert sorted(table[xd.TIE_AT].tolist()) == [0, 0, xd.MIN_DEPTH, xd.MIN_DEPTH] and int(table[xd.TIE_AT + 1].sum()) == 2 * xd.MIN_DEPTH
    assert want["extend_records"][j][1 + side] == xd.TIE_AT
    # depth: exactly min_depth on 20 columns, one less on the next 20
    j, side = xd.DEPTH_END
    depth = want["ext_pile"][j, side].sum(axis=1)
    assert depth[:20].tolist() == [xd.MIN_DEPTH] * 20 and depth[20:40].tolist() == [xd.MIN_DEPTH - 1] * 20 and not depth[40:].any()
    assert want["extend_records"][j][1 + side] == 20
    # diverged: none is accepted; those that keep a whole k-mer are placed and rejected (six differences in 95 bases leave few at k = 41)
    assert sum(1 for i in sel("diverged") if rows[i][0] < po.AMBIGUOUS and not acc[i]) >= (8 if k <= 31 else 1)
    assert not any(acc[i] for i in sel("diverged"))
    # indel: with a band, accepted reads whose overhang lies on another diagonal than the placement's
    if band >= 4:
        shifted = [i for i in sel("indel") if acc[i] and (al[i][2] or al[i][3])
                   and ((over_b(i) > 0 and int(al[i][4]) != int(rows[i][2])) or (over_e(i) > 0 and int(al[i][5]) != int(rows[i][3])))]
        assert len(shifted) >= 10
    # short and random: nothing of them is placed
    assert all(rows[i][0] >= po.AMBIGUOUS for g in ("short", "random") for i in sel(g)) and len(seqs[groups["short"][0]]) < 21
    # something is emitted at every end
    assert all(r[1] > 0 and r[2] > 0 for r in want["extend_records"])


@pytest.mark.parametrize("L", [64, 100])
def test_uniform_ends_sets_extend(L):
    recs, seqs, groups, o, want = ends(31, 8, 16, L)
    assert {len(s) for s in seqs} == {L} and int(want["accepted"].sum()) >= 40
    assert sum(r[1] + r[2] for r in want["extend_records"]) >= 40
