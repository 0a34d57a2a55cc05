"""The pair kernels (mf_pairs.hip) where their code changes path, exactly against tests/pair_oracle.PairOracle -- placements, scores,
pairs, every record table, depth, pile-up, consensus, unplaced and the identities, through test_gpu_pairs.check: rescue targets on either
side of the longest read a wave stages (994 bases; beyond it the candidates are scored from the read stream), uniform-length target sets
with Ns on the edges of the ballot's words, bait Ns under the candidates, baits on either side of the pair counters' LDS limit (170
records), and more pairs than one turn of pair_list_kernel's grid.  The data is tests/pair_edge_data.py's; what it holds is checked in
tests/test_pair_edge_data.py without a device.  There is no tolerance anywhere."""
import collections
import re

import numpy as np
import pytest

from tests import pair_edge_data as pe
from tests import pair_oracle as pa
from tests import place_oracle as po
from tests.report_data import mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_pairs import PAIR_REC, check, first_bad
from tests.test_gpu_verify import rec_rows, rows_of

pytestmark = pytest.mark.gpu


def both_ways(mf, ks, r1, r2, P, want, n, window, rescue_permille, max_permille):
    """the call as the oracle saw the sets, and with the sets the other way round -> the first call's result"""
    lo, hi = window
    p = check(mf.place_pairs(ks, r1, r2, lo, hi, True, rescue_permille, 2, max_permille), P, want, n, 2)
    check(mf.place_pairs(ks, r2, r1, lo, hi, True, rescue_permille, 2, max_permille), P, want, n, 2, swapped=True)
    return p


# ------------------------------------------------------------------ 1. targets around the longest staged read
@pytest.mark.parametrize("k", [21, 41])
def test_long_targets_match_the_oracle(mf, ol, k):
    text, s1, s2, what = pe.long_targets(k)
    n = len(s1)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    assert r1.info.uniform_len == 150 and r2.info.uniform_len == 0
    t1, t2 = o.tally(s1), o.tally(s2)
    for max_permille in (1000, 30):
        want = P.pairs(s1, s2, t1, t2, 1, max_permille, pe.LONG_WINDOW[0], pe.LONG_WINDOW[1], 1, 100)
        p = both_ways(mf, ks, r1, r2, P, want, n, pe.LONG_WINDOW, 100, max_permille)
        rescued = collections.Counter(t[1:4] for i, t in enumerate(what) if t[0] != "filler" and p.pairs["kind"][i] == mf.PAIR_RESCUED_2
                                      and p.place2["votes"][i] == 0 and p.place2["record"][i] < mf.PLACE_AMBIGUOUS)
        assert all(rescued[(L, strand, form)] >= 2 for L in (995, 1200) for strand in (0, 1) for form in (0, 1, 2)), rescued
        assert sum(rescued.values()) == sum(t[0] != "filler" for t in what)
    # once more on the same handles, both ways round: the buffers the first set's handle keeps are in use again
    both_ways(mf, ks, r1, r2, P, want, n, pe.LONG_WINDOW, 100, 30)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 2. both sets of one length, Ns in the targets
@pytest.mark.parametrize("L", [150, 995])
def test_uniform_target_sets_with_ns(mf, ol, L):
    k = 31
    text, s1, s2, what = pe.uniform_targets(L, k)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    assert r1.info.uniform_len == 150 and r2.info.uniform_len == L
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, pe.LONG_WINDOW[0], pe.LONG_WINDOW[1], 1, 100)
    p = both_ways(mf, ks, r1, r2, P, want, len(s1), pe.LONG_WINDOW, 100, 1000)
    with_n = [i for i, t in enumerate(what) if t[0] == "uniform" and t[2] and p.pairs["kind"][i] == mf.PAIR_RESCUED_2]
    assert len(with_n) >= 20 and all(int(p.score2["compared"][i]) == L - len(what[i][2]) for i in with_n)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 3. bait positions that are not valid under a candidate
@pytest.mark.parametrize("k", [21, 31])
def test_bait_ns_under_the_candidates(mf, ol, k):
    text, s1, s2, what = pe.bait_n_targets(k)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, pe.BAIT_N_WINDOW[0], pe.BAIT_N_WINDOW[1], 1, 100)
    p = both_ways(mf, ks, r1, r2, P, want, len(s1), pe.BAIT_N_WINDOW, 100, 1000)
    held = set()
    for i, t in enumerate(what):
        if t[0] == "run":
            assert p.pairs["kind"][i] == mf.PAIR_RESCUED_2 and int(p.score2["compared"][i]) == t[3] - t[4]          # the clipped length less the bait's Ns
            held.add(t[4])
    assert {0, 1, 16, 33} < held
    short, exact = [i for i, t in enumerate(what) if t[0] == "edge"]
    assert p.pairs["kind"][short] == mf.PAIR_SINGLE_1 and p.place2["record"][short] == mf.PLACE_NONE
    assert p.pairs["kind"][exact] == mf.PAIR_RESCUED_2 and int(p.score2["compared"][exact]) == k and p.place2["start"][exact] == k + 1 - 150
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 4. the pair counters on either side of their LDS limit
@pytest.mark.parametrize("n_rec", [170, 171])
def test_pair_counters_at_the_lds_limit(mf, ol, n_rec):
    k = 21
    text, s1, s2, what = pe.many_record_pairs(n_rec)
    n = len(s1)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    assert len(ks.record_starts) - 1 == n_rec
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    t1, t2 = o.tally(s1), o.tally(s2)
    lo, hi = pe.MANY_WINDOW
    rejected = {}
    for max_permille in (1000, 30):
        want = P.pairs(s1, s2, t1, t2, 1, max_permille, lo, hi, 1, 100)
        p = check(mf.place_pairs(ks, r1, r2, lo, hi, True, 100, 2, max_permille), P, want, n, 2)
        got = rec_rows(p.pair_records, PAIR_REC)
        assert got.shape == (n_rec, 6) and not first_bad(got, want["pair_rec"]), first_bad(got, want["pair_rec"])
        assert int(got[:, :5].sum()) + p.pairs_none == n and p.pairs_none == want["none"] >= 20
        assert np.all(got[n_rec - 6:, :5] >= 3) and np.all(got[:, :5].sum(axis=1) >= 1)
        rejected[max_permille] = int(p.score_records["rejected"].sum())
    assert rejected[1000] == 0 and rejected[30] >= 15
    check(mf.place_pairs(ks, r1, r2, lo, hi, True, 100, 2, 30), P, want, n, 2)          # and warm
    r1.close(); r2.close(); ks.close()


def copies_want(P, a, b, idx, lo, hi):
    """what the oracle gives for the pairs (a[i], b[i]) for i in idx: each pair of the pool alone; the set's per-pair arrays are the pool's
    rows by index, its sums the pool's times the copies (depth unclamped)"""
    o = P.o
    one = [P.pairs([x], [y], o.tally([x]), o.tally([y]), 1, 1000, lo, hi, 1, 100) for x, y in zip(a, b)]
    mult = np.bincount(idx, minlength=len(a))
    want = {f: np.concatenate([w[f] for w in one])[idx] for f in ("passes1", "passes2", "rows1", "rows2", "scores1", "scores2", "pairs")}
    for f in ("depth", "counts", "place_rec", "score_rec", "pair_rec"):
        want[f] = sum(int(m) * w[f].astype(np.int64) for m, w in zip(mult, one))
    for j in range(len(o.recs)):
        want["place_rec"][j, 4] = int((want["depth"][int(o.starts[j]):int(o.starts[j + 1])] > 0).sum())
    for f in ("place_rec", "score_rec", "pair_rec"):
        want[f] = want[f].astype(np.uint64)
    want["none"] = sum(int(m) * w["none"] for m, w in zip(mult, one))
    want["unplaced"] = [sum(int(m) * w["unplaced"][i] for m, w in zip(mult, one)) for i in (0, 1)]
    return want


# ------------------------------------------------------------------ 5. more pairs than one turn of pair_list_kernel's grid
def test_more_pairs_than_one_turn_of_the_list_grid(mf, ol):
    k = 21
    text, a, b, what = pe.turn_pool()
    turn = int(re.search(r"(\d+) CUs", mf.device_name(0)).group(1)) * 8 * 256          # the pairs the capped grid takes at once
    n = turn + 3 * 256 + 77
    idx = pe.copies(a, b, n, 3)
    lo, hi = pe.TURN_WINDOW
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    want = copies_want(P, a, b, idx, lo, hi)
    mult = np.bincount(idx, minlength=len(a))
    assert mult.min() >= 1
    assert int(want["depth"].max()) < po.CLAMP
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, [a[i] for i in idx]), upload(mf, ol, [b[i] for i in idx])
    p = check(mf.place_pairs(ks, r1, r2, lo, hi, True, 100, 2), P, want, n, 2)
    # the pairs of the second turn: a partly filled last wave, every kind among them
    assert np.array_equal(rows_of(p.place1)[turn:], want["rows1"][turn:]) and np.array_equal(rows_of(p.place2)[turn:], want["rows2"][turn:])
    assert np.array_equal(p.pairs["kind"][turn:].astype(np.int64), want["pairs"][turn:, 0]) and np.array_equal(p.pairs["insert"][turn:].astype(np.int64), want["pairs"][turn:, 1])
    assert set(p.pairs["kind"][turn:].tolist()) == set(range(7)) and (n - turn) % 64 != 0
    assert p.pairs_none == want["none"] >= turn // 16
    r1.close(); r2.close(); ks.close()
