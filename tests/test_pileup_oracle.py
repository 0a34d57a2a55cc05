"""PileupOracle.call_fast -- the array form of the call that the tests on baits of a million positions use -- against the plain call(),
exactly: the consensus bytes and the records' six sums, on counts that hold ties, positions without a base and bases on invalid bait
letters.  No GPU."""
import numpy as np
import pytest

from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests.report_data import mutate
from tests.scale_data import scale_bait, scale_reads
from tests.test_gpu_place import place_bait, place_reads


def engineered(P, counts, seed):
    """counts with more put on top: exact ties of two, three and four letters, single bases on positions that had none, and all of these
    on invalid bait letters too; every tenth position of the rest is left as the reads piled it"""
    rng = np.random.default_rng(seed)
    c = counts.copy()
    n = len(c)
    invalid = np.array([ch == "N" for ch in P.bait])
    assert invalid.any()
    at = rng.permutation(n)
    for i, p in enumerate(at[:n // 2]):
        kind = i % 5
        if kind == 0:                                        # a tie of the top two
            a, b = rng.choice(4, 2, replace=False)
            c[p, a] = c[p, b] = c[p].max() + 1
        elif kind == 1:                                      # three equal, the fourth smaller
            c[p] = c[p].max() + 2
            c[p, rng.integers(4)] -= 1
        elif kind == 2:                                      # all four equal (depth 0 where nothing was piled)
            c[p] = c[p].max()
        elif kind == 3:                                      # one base of another letter than the bait's
            c[p, rng.integers(4)] += 1
        else:
            c[p] = 0
    for i, p in enumerate(np.nonzero(invalid)[0][:200]):     # every kind on invalid letters as well
        c[p] = [(3, 3, 0, 0), (0, 0, 0, 0), (0, 2, 0, 0), (1, 1, 1, 1), (0, 0, 5, 4)][i % 5]
    d = c.sum(axis=1)
    top = (c == c.max(axis=1)[:, None]).sum(axis=1)
    assert (d == 0).sum() > 10 and ((top > 1) & (d > 0)).sum() > 10 and (invalid & (d > 0)).sum() > 0 and (invalid & (d == 0)).sum() > 0
    return c


def both(P, counts, min_depth):
    cons, rec = P.call(counts, min_depth)
    fcons, frec = P.call_fast(counts, min_depth)
    assert fcons.dtype == cons.dtype and frec.dtype == rec.dtype and fcons.shape == cons.shape and frec.shape == rec.shape
    bad = np.nonzero(fcons != cons)[0]
    assert bad.size == 0, [(int(p), chr(fcons[p]), chr(cons[p]), counts[p].tolist()) for p in bad[:10]]
    assert np.array_equal(frec, rec), np.nonzero((frec != rec).any(axis=1))[0][:10]
    return cons, rec


@pytest.mark.parametrize("k", [21, 32])
def test_call_fast_equals_call_on_the_placement_bait(k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    P = pio.PileupOracle(o)
    _, seqs = place_reads(text, parts, k, 600, seed=40 + k, uniform=False)
    seqs = seqs + [mutate(parts["g"], 0.02, 3)[a:a + 120] for a in range(0, 2800, 37)]
    counts = P.pile(seqs, o.place(o.tally(seqs), 1)[1])
    assert counts.sum() > 0
    for c in (counts, engineered(P, counts, k)):
        for min_depth in (1, 3):
            cons, rec = both(P, c, min_depth)
    assert int(rec[:, 4].sum()) > 0 and int(rec[:, 5].sum()) > 0 and b"n" in bytes(cons) and b"N" in bytes(cons)


def test_call_fast_equals_call_on_a_small_bait_of_the_scale_shape():
    """runs of tiny and empty records at the front, in the middle and as the last records; k = 13, so that records of 13 .. 15 positions
    take reads"""
    k = 13
    text, parts = scale_bait(k, n_block=140, front=1500, back=900, gap=700)
    o = po.PlaceOracle(text, k)
    P = pio.PileupOracle(o)
    lens = o.lens
    assert lens[:6] == [5, 0, 15, 1, 0, 9] and lens[-5:] == [3, 0, 12, 14, 0] and len(parts["tiny_runs"]) >= 4
    seqs = scale_reads(parts, k, 900, seed=5, uniform=False, read_len=60) + scale_reads(parts, k, 300, seed=6, uniform=True, read_len=40)
    counts = P.pile(seqs, o.place(o.tally(seqs), 1)[1])
    tiny = [j for j, n in enumerate(lens) if 0 < n < 16 and counts[P.starts[j]:P.starts[j + 1]].sum() > 0]
    assert tiny, "no read on a record shorter than 16 positions"
    for c in (counts, engineered(P, counts, 1)):
        for min_depth in (1, 3):
            cons, rec = both(P, c, min_depth)
    # the last records, the empty one among them, hold what the plain call gives them
    assert rec[-1].tolist() == [0] * 6 and rec[-4].tolist() == [0] * 6 and int(rec[-2, 0]) == int(c[P.starts[-3]:P.starts[-2]].sum())
