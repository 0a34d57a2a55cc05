"""The builders of tests/pair_data.py give what the GPU tests of pair-aware placement rely on, evaluated with the oracle alone (no
device): in the main set every pair kind occurs at least 20 times; both kinds of rescued mate occur -- one that did not pass, one that
passed and was ambiguous --; at least 20 targets are refused for a tie, 20 for the cut and 20 because no candidate compares k bases;
some rescued mate hangs over each end of a record; a rejected mate is never rescued; the neighbour pairs are what they say."""
import collections

import numpy as np
import pytest

from tests import pair_data as pd
from tests import pair_oracle as pa
from tests import place_oracle as po


@pytest.fixture(scope="module")
def main_set():
    text, recs, sample = pd.pair_bait()
    s1, s2, what = pd.pair_set()
    o = po.PlaceOracle(text, 31)
    P = pa.PairOracle(o)
    return o, P, s1, s2, what, o.tally(s1), o.tally(s2)


def test_the_bait_is_what_the_builders_say():
    text, recs, sample = pd.pair_bait()
    assert [len(r) for r in recs] == [900, 650, 820] and all(600 <= len(r) <= 900 for r in recs)
    assert recs[0][600:800] == recs[1][150:350]
    u = recs[2][360:420]
    assert recs[2][301:360] == u[1:] and recs[2][300] != u[0]
    s0 = sample[0][pd.FLANK:pd.FLANK + 900]
    diff = [i for i in range(900) if s0[i] != recs[0][i]]
    assert diff == list(range(307, 600, 20))
    assert all(sample[j][pd.FLANK:pd.FLANK + len(recs[j])] == recs[j] for j in (1, 2))


def test_the_sets_are_uniform_and_ragged():
    s1, s2, what = pd.pair_set()
    assert {len(s) for s in s1} == {150}
    lens = [len(s) for s in s2]
    assert min(lens) >= 40 and max(lens) <= 151 and len(set(lens)) > 60
    assert sum("N" in s for s in s2) >= 20 and not any("N" in s for s in s1)
    starts = np.cumsum([0] + lens[:-1])
    assert set(int(b) % 16 for b in starts) == set(range(16))


def test_every_kind_and_every_refusal_occurs_in_the_main_set(main_set):
    o, P, s1, s2, what, t1, t2 = main_set
    lo, hi = pd.WINDOW
    w = P.pairs(s1, s2, t1, t2, 1, 1000, lo, hi, 1, 60)
    kinds = collections.Counter(w["pairs"][:, 0].tolist())
    assert all(kinds[kind] >= 20 for kind in range(7)), kinds
    why = collections.Counter(x for x in w["why"] if x)
    assert why["tie"] >= 20 and why["cut"] >= 20 and why["short"] >= 20, why
    # both kinds of rescued mate: one that did not pass, one that passed and was ambiguous
    rescued = [(w["single"][1]["rows"][i], w["rows2"][i]) for i in np.nonzero(w["pairs"][:, 0] == pa.RESCUED_2)[0]]
    rescued += [(w["single"][0]["rows"][i], w["rows1"][i]) for i in np.nonzero(w["pairs"][:, 0] == pa.RESCUED_1)[0]]
    before = collections.Counter(int(b[0]) for b, _ in rescued)
    assert before[po.NONE] >= 20 and before[po.AMBIGUOUS] >= 20 and len(before) == 2
    assert all(a[4] == 0 and a[0] < po.AMBIGUOUS for _, a in rescued)
    # some rescued mate hangs over each end of a record
    assert sum(a[2] < 0 for _, a in rescued) >= 10 and sum(a[3] > o.lens[int(a[0])] for _, a in rescued) >= 10
    # cross pairs and both discordant ones
    assert int(w["pair_rec"][:, 2].sum()) >= 20 and int(w["pair_rec"][:, 1].sum()) >= 40
    d = w["pairs"][w["pairs"][:, 0] == pa.DISCORDANT, 1]
    assert (d == -1).sum() >= 40 and (d > hi).sum() >= 20
    assert int(w["pair_rec"][:, :5].sum()) + w["none"] == len(s1)


def test_the_cuts_move_what_they_should(main_set):
    o, P, s1, s2, what, t1, t2 = main_set
    lo, hi = pd.WINDOW
    by = {rp: P.pairs(s1, s2, t1, t2, 1, 1000, lo, hi, 1, rp) for rp in (0, 60, 1000)}
    n = {rp: int((by[rp]["pairs"][:, 0] == pa.RESCUED_1).sum() + (by[rp]["pairs"][:, 0] == pa.RESCUED_2).sum()) for rp in by}
    assert 20 <= n[0] < n[60] < n[1000]
    # a tie stays a tie whatever the cut
    assert sum(x == "tie" for x in by[1000]["why"]) >= 20
    off = P.pairs(s1, s2, t1, t2, 1, 1000, lo, hi, 0, 60)
    assert not any(off["why"]) and not np.isin(off["pairs"][:, 0], (pa.RESCUED_1, pa.RESCUED_2)).any()


def test_a_rejected_mate_is_never_rescued():
    text, recs, sample = pd.pair_bait()
    s1, s2, what = pd.pair_set()
    o = po.PlaceOracle(text, 21)
    P = pa.PairOracle(o)
    lo, hi = pd.WINDOW
    w = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 30, lo, hi, 1, 1000)
    light = [i for i, n in enumerate(what) if n == "light"]
    assert len(light) >= 20
    for i in light:
        assert w["rows2"][i][0] < po.AMBIGUOUS and w["rows2"][i][4] > 0 and not pa.vo.accepts(*w["scores2"][i], 30)
        assert w["pairs"][i].tolist() == [pa.SINGLE_1, -1] and w["why"][i] is None


@pytest.mark.parametrize("k", [21, 31, 41])
def test_the_neighbour_pairs(k):
    text, recs, sample = pd.pair_bait()
    s1, s2, inside = pd.neighbour_pairs(k)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    lo, hi = pd.WINDOW
    w = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, lo, hi, 1, 60)
    assert inside == [k - 1, k, k + 9, 100]
    assert all(r[0] >= po.AMBIGUOUS for r in w["single"][1]["rows"])          # the vote places none of them
    # k - 1 bases inside: the candidate at the mate's own place would pass the cut and is refused for what it compares; the candidates
    # further inside compare more and match nothing
    assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] == "cut"
    c, m = P.V.score(s2[0], (0, 1, 900 - (k - 1), 1050 - (k - 1), 0, 0))
    assert c == k - 1 and m * 1000 <= 60 * c
    for i in (1, 2, 3):
        assert w["pairs"][i][0] == pa.RESCUED_2
        assert w["rows2"][i].tolist()[:4] == [0, 1, 900 - inside[i], 1050 - inside[i]] and w["scores2"][i][0] == inside[i]
    # nothing of them lies on the neighbouring record
    assert int(w["depth"][900:].sum()) == 0 and int(w["counts"][900:].sum()) == 0
