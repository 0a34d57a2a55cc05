"""The builders of tests/pair_edge_data.py give what tests/test_gpu_pair_edges.py relies on, evaluated with the oracle alone (no
device), so that no GPU test there passes on data that never reaches the code path it is named for: the long targets are unplaced by
the vote -- ambiguous or not passing as designed --, rescued, and fill every (length, strand, N form) cell and every b0 mod 16 around
the staging limit; bait Ns lie under rescued candidates wholly and partly, and decide between k - 1 and k compared bases; the many
records hold every counted kind on either side of the LDS limit; the uniform sets are uniform and hold their Ns where they say."""
import collections

import numpy as np
import pytest

from tests import pair_edge_data as pe
from tests import pair_oracle as pa
from tests import place_oracle as po


def oracle_of(text, k, s1, s2, window, rescue_permille=100, max_permille=1000):
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    return o, P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, max_permille, window[0], window[1], 1, rescue_permille)


def test_the_long_bait_is_what_the_builder_says():
    for k in (21, 41):
        text, recs, sample, E = pe.long_bait(k)
        assert [len(recs[n]) for n in ("ends", "long", "other")] == [3100, 2300, 500] and E == k + 4
        long_, s = recs["long"], sample["long"][pe.FLANK:pe.FLANK + 2300]
        assert long_[pe.ECHO_AT:pe.ECHO_AT + E] == long_[pe.ECHO_FROM:pe.ECHO_FROM + E] == s[pe.ECHO_AT:pe.ECHO_AT + E]
        diff = [i for i in range(2300) if s[i] != long_[i]]
        assert diff[0] == 407 and diff[-1] == 1887 and all(400 <= i < 1900 for i in diff)
        # outside the echo no 21 bases in a row are the bait's; the positions next to the echo differ
        gaps = [b - a for a, b in zip(diff, diff[1:]) if not (a < pe.ECHO_AT + E and b >= pe.ECHO_AT)]
        assert max(gaps) <= 20 and pe.ECHO_AT - 1 in diff and pe.ECHO_AT + E in diff
        e, se = recs["ends"], sample["ends"][pe.FLANK:pe.FLANK + 3100]
        diff = [i for i in range(3100) if se[i] != e[i]]
        assert diff == list(range(7, 1300, 20)) + list(range(1807, 3100, 20))
        assert pe.STAGE_MAX == 16 * 64 - 30


@pytest.mark.parametrize("k", [21, 41])
def test_the_long_targets_are_unplaced_by_the_vote_and_rescued(k):
    text, s1, s2, what = pe.long_targets(k)
    o, w = oracle_of(text, k, s1, s2, pe.LONG_WINDOW)
    assert {len(s) for s in s1} == {150}
    before = w["single"][1]["rows"]
    cells, bmods = collections.Counter(), collections.defaultdict(set)
    starts = np.cumsum([0] + [len(s) for s in s2[:-1]])
    for i, t in enumerate(what):
        if t[0] == "filler":
            assert w["pairs"][i].tolist() == [pa.NONE, -1] and 21 <= len(s2[i]) <= 36
            continue
        kind, L, strand, form, bm, start = t
        assert len(s2[i]) == L and int(starts[i]) % 16 == bm and s2[i].count("N") == form
        # unplaced by the vote: the targets over the echo pass and are ambiguous, unless the N lies in it; those over an end of `ends` do not pass
        assert before[i][0] == (po.AMBIGUOUS if kind == "long" and form != 1 else po.NONE), (t, before[i])
        # and rescued where it lies
        assert w["pairs"][i][0] == pa.RESCUED_2 and pe.LONG_WINDOW[0] <= w["pairs"][i][1] <= pe.LONG_WINDOW[1], (t, w["pairs"][i], w["why"][i])
        assert w["rows2"][i].tolist()[:5] == [1 if kind == "long" else 0, strand, start, start + L, 0]
        c, m = w["scores2"][i]
        n_sub, n_rec = L // 20, o.lens[int(w["rows2"][i][0])]
        ns_inside = sum(0 <= (start + L - 1 - j if strand else start + j) < n_rec for j, ch in enumerate(s2[i]) if ch == "N")
        assert c == min(start + L, n_rec) - max(start, 0) - ns_inside and n_sub - 3 <= m <= n_sub + 3
        cells[(kind, L, strand, form)] += 1
        bmods[(kind, L, strand)].add(bm)
    for L in (994, 995):
        for strand in (0, 1):
            assert bmods[("long", L, strand)] == set(range(16))
    assert all(cells[("long", L, strand, form)] >= 2 for L in pe.LONG_LENGTHS for strand in (0, 1) for form in (0, 1, 2)), cells
    assert all(cells[("hang", L, strand, form)] == 2 for L in (994, 1200) for strand in (0, 1) for form in (0, 1, 2)), cells
    hang = [(t, w["rows2"][i]) for i, t in enumerate(what) if t[0] == "hang"]
    assert sorted({int(r[2]) for t, r in hang if t[2] == 0}) == [-37, -5]
    assert sorted({int(r[3]) - 3100 for t, r in hang if t[2] == 1}) == [5, 37]
    assert {pe.STAGE_MAX - 1, pe.STAGE_MAX, pe.STAGE_MAX + 1, 1200} == set(pe.LONG_LENGTHS)
    # the window's first and last insert both win somewhere
    won = set(w["pairs"][w["pairs"][:, 0] == pa.RESCUED_2, 1].tolist())
    assert pe.LONG_WINDOW[0] in won and pe.LONG_WINDOW[1] in won and pe.LONG_WINDOW[1] - pe.LONG_WINDOW[0] + 1 <= 32


@pytest.mark.parametrize("L", [150, 995])
def test_the_uniform_sets_are_uniform_and_hold_their_ns(L):
    k = 31
    text, s1, s2, what = pe.uniform_targets(L, k)
    assert {len(s) for s in s1} == {150} and {len(s) for s in s2} == {L}
    o, w = oracle_of(text, k, s1, s2, pe.LONG_WINDOW)
    targets = [i for i, t in enumerate(what) if t[0] == "uniform"]
    with_n = [i for i in targets if what[i][2]]
    assert 3 * len(with_n) >= len(targets)
    for i in targets:
        assert [j for j, c in enumerate(s2[i]) if c == "N"] == list(what[i][2])
        assert w["single"][1]["rows"][i][0] >= po.AMBIGUOUS
    for strand in (0, 1):
        seen = {what[i][2] for i in with_n if what[i][1] == strand and w["pairs"][i][0] == pa.RESCUED_2}
        assert {(x,) for x in pe.N_OFFSETS + (L - 1,)} <= seen
        if L == 150:
            assert set(pe.N_STRADDLES) <= seen
    rescued = [i for i in targets if w["pairs"][i][0] == pa.RESCUED_2]
    assert len(rescued) >= 20 and len([i for i in rescued if what[i][2]]) >= 20
    for i in rescued:
        assert w["scores2"][i][0] == L - len(what[i][2])
    kinds = collections.Counter(w["pairs"][:, 0].tolist())
    assert kinds[pa.SINGLE_1] >= 2 and kinds[pa.NONE] >= 2 and set(kinds) == {pa.RESCUED_2, pa.SINGLE_1, pa.NONE}


@pytest.mark.parametrize("k", [21, 31])
def test_bait_ns_lie_under_the_rescued_candidates(k):
    text, s1, s2, what = pe.bait_n_targets(k)
    text0, recs, sample = pe.bait_n_bait()
    for at, n in pe.BAIT_N_RUNS:
        assert recs[0][at - 1:at + n + 1] == recs[0][at - 1] + "N" * n + recs[0][at + n] and "N" not in recs[0][at - 1] + recs[0][at + n]
    assert [at % 32 for at, n in pe.BAIT_N_RUNS] == [0, 15, 31] and [n for at, n in pe.BAIT_N_RUNS] == [1, 16, 33]
    assert recs[0].count("N") == 1 + 16 + 33 + 1 and recs[0][pe.BAIT_N_EDGE] == "N"
    o, w = oracle_of(text, k, s1, s2, pe.BAIT_N_WINDOW)
    assert np.all(w["single"][1]["rows"][:, 0] >= po.AMBIGUOUS) and np.all(w["single"][0]["rows"][:, 0] == 0)
    held = collections.Counter()
    for i, t in enumerate(what):
        if t[0] != "run":
            continue
        kind, strand, start, L, n_held = t
        assert w["pairs"][i][0] == pa.RESCUED_2, (t, w["why"][i])
        assert w["rows2"][i].tolist()[:4] == [0, strand, start, start + L] and w["scores2"][i][0] == L - n_held >= k
        held[(strand, n_held)] += 1
    for strand in (0, 1):
        assert all(held[(strand, n)] >= 3 for n in (0, 1, 16, 33)), held
        partial = [n for (s, n) in held if s == strand and n not in (0, 1, 16, 17, 33, 34, 49, 50)]
        assert len(partial) >= 2, held
    # the N near r0's begin: k bases inside and k - 1 compared is refused as short; k + 1 inside and k compared is rescued
    i, j = [i for i, t in enumerate(what) if t[0] == "edge"]
    assert what[i] == ("edge", k, k - 1) and what[j] == ("edge", k + 1, k)
    assert w["pairs"][i].tolist() == [pa.SINGLE_1, -1] and w["why"][i] == "short"
    P = pa.PairOracle(o)
    assert P.V.score(s2[i], (0, 0, k - 150, k, 0, 0)) == (k - 1, 1)
    assert w["pairs"][j].tolist() == [pa.RESCUED_2, pe.BAIT_N_WINDOW[0]] and w["scores2"][j].tolist() == [k, 1]
    assert w["rows2"][j].tolist()[:4] == [0, 0, k + 1 - 150, k + 1]


@pytest.mark.parametrize("n_rec", [170, 171])
def test_the_many_records_hold_every_counted_kind(n_rec):
    assert 6 * 170 + 1 <= 1024 < 6 * 171 + 1
    k = 21
    text, s1, s2, what = pe.many_record_pairs(n_rec)
    assert all(40 <= len(s) <= 60 for s in s1 + s2) and pe.MANY_WINDOW[1] - pe.MANY_WINDOW[0] + 1 == 100
    o, w = oracle_of(text, k, s1, s2, pe.MANY_WINDOW)
    assert len(o.recs) == n_rec
    rec = w["pair_rec"].astype(np.int64)
    assert np.all(rec[:, :5].sum(axis=1) >= 1)
    assert np.all(rec[n_rec - 6:, :5] >= 3), rec[n_rec - 6:]
    assert np.all(rec[n_rec - 6:, 5] > 0) and w["none"] >= 20
    assert int(rec[:, :5].sum()) + w["none"] == len(s1)
    # every pair is of the kind it was drawn as
    kind_of = {"proper": (pa.PROPER,), "far": (pa.DISCORDANT,), "same_strand": (pa.DISCORDANT,), "cross": (pa.DISCORDANT,), "rescued": (pa.RESCUED_2,),
               "single": (pa.SINGLE_1,), "light": (pa.PROPER,), "none": (pa.NONE,)}
    for i, (kind, j) in enumerate(what):
        assert w["pairs"][i][0] in kind_of[kind], (i, kind, j, w["pairs"][i], w["why"][i])
    assert int(rec[:, 2].sum()) == sum(kind == "cross" for kind, j in what) and rec[n_rec - 1, 2] >= 3          # (mate 2 of the last record's lies on the first)
    # a cut of 30 rejects the light mates: placed and rejected, never rescued
    o, cut = oracle_of(text, k, s1, s2, pe.MANY_WINDOW, max_permille=30)
    light = [i for i, (kind, j) in enumerate(what) if kind == "light"]
    assert len(light) >= 15 and all(cut["pairs"][i].tolist() == [pa.SINGLE_1, -1] and cut["why"][i] is None for i in light)
    assert int(cut["score_rec"][:, 1].sum()) == len(light)


def test_the_turn_pool_and_its_copies():
    text, s1, s2, what = pe.turn_pool()
    assert 120 <= len(s1) <= 136 and all(len(s) == 40 for s in s1 + s2)
    o, w = oracle_of(text, 21, s1, s2, pe.TURN_WINDOW)
    kinds = collections.Counter(w["pairs"][:, 0].tolist())
    assert all(kinds[kind] >= 8 for kind in range(7)), kinds
    assert int(w["pair_rec"][:, 2].sum()) >= 8 and (w["pairs"][w["pairs"][:, 0] == pa.DISCORDANT, 1] > pe.TURN_WINDOW[1]).sum() >= 8
    n = 524288 + 3 * 256 + 77
    idx = pe.copies(s1, s2, n, 3)
    assert idx.shape == (n,) and idx.min() == 0 and idx.max() == len(s1) - 1
    assert set(idx[n - 1100:].tolist()) == set(range(len(s1))) and set(idx[n - 845:].tolist()) == set(range(len(s1)))
    assert np.array_equal(idx, pe.copies(s1, s2, n, 3))
