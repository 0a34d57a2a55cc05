"""Pairs with a band (mf_align_pairs / mf.align_pairs) against the plain-Python oracle of tests/pair_align_oracle.py, which is written from
the "pairs with a band" section of include/mitofilter.h: both sets' placements and alignments, the pairs, base depth, every record table,
the pile-up, the consensus, the indel table, the insertion pile and the gapped consensus, the extension pile and the extended records, and
unplaced are compared exactly, with the identities of the aligning and the pair sections over both sets' reads.  The data of the first
test is tests/pair_align_data.py's (what it holds is checked in tests/test_pair_align_data.py without a device); the others build the
few pairs they need and say with the oracle what those are.  There is no tolerance anywhere."""
import functools
import random
import re

import numpy as np
import pytest

from tests import pair_align_data as pad
from tests import pair_align_oracle as pao
from tests import pair_data
from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests.pair_data import _rand, substituted
from tests.report_data import fasta, mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_align import ALIGN_FIELDS, PILE_REC, PLACE_FIELDS, PLACE_REC, align_rows, first_bad, identities, table
from tests.test_gpu_extend import check_extended
from tests.test_gpu_gapped import check_gapped
from tests.util_data import bits_to_bool, revcomp

pytestmark = pytest.mark.gpu

PAIR_REC = ("proper", "discordant", "cross", "rescued", "single", "insert_sum")
LO, HI = pad.WINDOW


def check(p, P, want, n, min_depth, band, swapped=False):
    """what an aligning paired call gave against what the oracle gave (swapped: the call took the sets the other way round)"""
    one, two = ("2", "1") if swapped else ("1", "2")
    for bits, place, align, m in ((p.bits1, p.place1, p.align1, one), (p.bits2, p.place2, p.align2, two)):
        assert np.array_equal(bits_to_bool(bits, n), want["passes" + m])
        got = table(place, PLACE_FIELDS)
        assert np.array_equal(got, want["rows" + m]), first_bad(got, want["rows" + m])
        got = table(align, ALIGN_FIELDS)
        assert np.array_equal(got, want["aligns" + m]), first_bad(got, want["aligns" + m])
    wp = want["pairs"].copy()
    if swapped:          # mate 1 of the call is the oracle's mate 2
        for a, b in ((pao.RESCUED_1, pao.RESCUED_2), (pao.SINGLE_1, pao.SINGLE_2)):
            wp[want["pairs"][:, 0] == a, 0] = b
            wp[want["pairs"][:, 0] == b, 0] = a
    got = table(p.pairs, ("kind", "insert"))
    assert np.array_equal(got, wp), first_bad(got, wp)
    got = table(p.pair_records, PAIR_REC).astype(np.uint64)
    if not swapped:          # (cross is counted at mate 1's record: the swapped call counts it at the other)
        assert np.array_equal(got, want["pair_rec"]), (got, want["pair_rec"])
    assert got.sum(axis=0).tolist() == want["pair_rec"].sum(axis=0).tolist()
    assert p.pairs_none == want["none"] and int(got[:, :5].sum()) + p.pairs_none == n
    assert np.array_equal(p.base_depth.astype(np.int64), np.minimum(want["depth"], po.CLAMP)), first_bad(p.base_depth.astype(np.int64), want["depth"])
    assert np.array_equal(table(p.place_records, PLACE_REC).astype(np.uint64), want["place_rec"]), (table(p.place_records, PLACE_REC), want["place_rec"])
    assert np.array_equal(align_rows(p.align_records), want["align_rec"]), (align_rows(p.align_records), want["align_rec"])
    got = table(p.indels, ("del", "ins", "ins_bases"))
    assert np.array_equal(got, want["indels"]), first_bad(got, want["indels"])
    assert p.unplaced.tolist() == want["unplaced"]
    if p.pileup is not None:
        got = table(p.pileup, ("a", "c", "g", "t"))
        assert np.array_equal(got, pio.clamped(want["counts"])), first_bad(got, want["counts"])
        cons, rec = pio.PileupOracle(P.o).call(want["counts"], min_depth)
        assert np.array_equal(p.consensus, cons)
        assert np.array_equal(table(p.pileup_records, PILE_REC).astype(np.uint64), rec)
    if p.gapped is not None:
        check_gapped(p, P.G, want, want["ins_pile"], min_depth, band)
    if p.extended is not None:
        E = p.ext_pile.shape[2]
        check_extended(p, P.X, want, want["ins_pile"], want["ext_pile"], min_depth, E)
    identities(p, want)
    return p


@functools.lru_cache(maxsize=None)
def data_oracle(k):
    text, recs, sample = pad.bait()
    o = po.PlaceOracle(text, k)
    s1, s2, what = pad.pair_set()
    return text, o, pao.PairAlignOracle(o), s1, s2, o.tally(s1), o.tally(s2)


# ------------------------------------------------------------------ 1. every output against the oracle
@pytest.mark.parametrize("band", [1, 8, "k-1"])
@pytest.mark.parametrize("k", [21, 31, 41])
def test_every_output_matches_the_oracle(mf, ol, k, band):
    band = min(31, k - 1) if band == "k-1" else band
    text, o, P, s1, s2, t1, t2 = data_oracle(k)
    n = len(s1)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    assert r1.info.uniform_len == 150 and r2.info.uniform_len == 0
    rescued = {}
    for max_permille in (1000, 30):
        for rescue_permille in (pad.RESCUE_PERMILLE, 0):
            want = P.pairs(s1, s2, t1, t2, 1, max_permille, band, LO, HI, 1, rescue_permille, 2, 8)
            for gapped in (False, True):
                for extend in (0, 8):
                    p = check(mf.align_pairs(ks, r1, r2, LO, HI, band, True, rescue_permille, 2, max_permille, gapped=gapped, extend=extend), P, want, n, 2, band)
                    assert (p.gapped is not None) == gapped and (p.extended is not None) == (extend > 0)
            rescued[(max_permille, rescue_permille)] = int(p.pair_records["rescued"].sum())
            votes0 = sum(int(((pl["votes"] == 0) & (pl["record"] < mf.PLACE_AMBIGUOUS)).sum()) for pl in (p.place1, p.place2))
            assert votes0 == rescued[(max_permille, rescue_permille)]
    assert rescued[(1000, pad.RESCUE_PERMILLE)] >= 100 > rescued[(1000, 0)]
    # the sets the other way round: the uniform set holds the settled mates' partners on the other side
    want = P.pairs(s1, s2, t1, t2, 1, 1000, band, LO, HI, 1, pad.RESCUE_PERMILLE, 2, 8)
    check(mf.align_pairs(ks, r2, r1, LO, HI, band, True, pad.RESCUE_PERMILLE, 2, 1000, gapped=True, extend=8), P, want, n, 2, band, swapped=True)
    # without the pile-up nothing else changes; threshold and mode are the aligning call's
    want3 = P.pairs(s1, s2, t1, t2, 3, 1000, band, LO, HI, 1, pad.RESCUE_PERMILLE, 2, 8)
    q = check(mf.align_pairs(ks, r1, r2, LO, HI, band, True, pad.RESCUE_PERMILLE, 2, 1000, pileup=False, threshold=3, mode=mf.MODE_EXHAUSTIVE), P, want3, n, 2, band)
    assert q.pileup is None and q.consensus is None and q.pileup_records is None and q.gapped is None
    r1.close(); r2.close(); ks.close()


def test_targets_from_both_sets_in_one_call(mf, ol):
    k, band = 21, 8
    text, o, P = data_oracle(k)[:3]
    s1, s2, what = pad.pair_set(mixed=True)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 30, band, LO, HI, 1, pad.RESCUE_PERMILLE, 2, 8)
    p = check(mf.align_pairs(ks, r1, r2, LO, HI, band, True, pad.RESCUE_PERMILLE, 2, 30, gapped=True, extend=8), P, want, len(s1), 2, band)
    assert int((p.pairs["kind"] == mf.PAIR_RESCUED_1).sum()) >= 50 and int((p.pairs["kind"] == mf.PAIR_RESCUED_2).sum()) >= 50
    # a warm call gives what the first gave
    check(mf.align_pairs(ks, r1, r2, LO, HI, band, True, pad.RESCUE_PERMILLE, 2, 30, gapped=True, extend=8), P, want, len(s1), 2, band)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 2. band 0 is mf_place_pairs
def test_band_0_is_place_pairs(mf, ol):
    text, recs, sample = pair_data.pair_bait()
    s1, s2, what = pair_data.pair_set()
    lo, hi = pair_data.WINDOW
    ks = mf.KmerSet.from_text(text, 31)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    for max_permille in (1000, 30):
        v = mf.place_pairs(ks, r1, r2, lo, hi, True, 60, 2, max_permille)
        a = mf.align_pairs(ks, r1, r2, lo, hi, 0, True, 60, 2, max_permille)
        assert int(v.pair_records["rescued"].sum()) >= 20
        for f in ("bits1", "bits2", "place1", "place2", "pairs", "pair_records", "base_depth", "place_records", "pileup", "consensus", "pileup_records", "unplaced"):
            assert np.array_equal(getattr(a, f), getattr(v, f)), f
        assert a.pairs_none == v.pairs_none
        for al, sc, pl in ((a.align1, v.score1, v.place1), (a.align2, v.score2, v.place2)):
            placed = pl["record"] < mf.PLACE_AMBIGUOUS
            assert np.array_equal(al["compared"], sc["compared"]) and np.array_equal(al["mismatches"], sc["mismatches"])
            assert not al["insertions"].any() and not al["deletions"].any()
            assert np.array_equal(al["ref_begin"][placed], pl["start"][placed]) and np.array_equal(al["ref_end"][placed], pl["end"][placed])
            assert not al["ref_begin"][~placed].any() and not al["ref_end"][~placed].any()
        for f in ("accepted", "rejected", "compared", "mismatches", "hist"):
            assert np.array_equal(a.align_records[f], v.score_records[f]), f
        assert not a.align_records["insertions"].any() and not a.align_records["gapped"].any() and not table(a.indels, ("del", "ins", "ins_bases")).any()
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 3. rescue=False is the two single calls added up
def test_without_rescue_every_shared_output_is_the_two_single_calls_added_up(mf, ol):
    k, band = 21, 8
    text = data_oracle(k)[0]
    s1, s2, what = pad.pair_set(mixed=True)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    for max_permille in (1000, 30):
        v1 = mf.align_reads(ks, r1, band, 2, max_permille, gapped=True, extend=8)
        v2 = mf.align_reads(ks, r2, band, 2, max_permille, gapped=True, extend=8)
        p = mf.align_pairs(ks, r1, r2, LO, HI, band, False, pad.RESCUE_PERMILLE, 2, max_permille, gapped=True, extend=8)
        assert np.array_equal(p.bits1, v1.bits) and np.array_equal(p.bits2, v2.bits)
        assert np.array_equal(p.place1, v1.place) and np.array_equal(p.place2, v2.place)
        assert np.array_equal(p.align1, v1.align) and np.array_equal(p.align2, v2.align)
        assert np.array_equal(p.base_depth, v1.base_depth + v2.base_depth)
        for f in ("forward", "reverse", "over_begin", "over_end", "base_sum"):
            assert np.array_equal(p.place_records[f], v1.place_records[f] + v2.place_records[f]), f
        for name, dtype in (("align_records", mf.ALIGN_RECORD), ("pileup", mf.PILEUP), ("indels", mf.INDEL), ("ins_pile", mf.PILEUP), ("ext_pile", mf.PILEUP)):
            for f in dtype.names:
                assert np.array_equal(getattr(p, name)[f], getattr(v1, name)[f] + getattr(v2, name)[f]), (name, f)
        for f in ("bases", "matches", "mismatches"):
            assert np.array_equal(p.pileup_records[f], v1.pileup_records[f] + v2.pileup_records[f]), f
        assert p.unplaced.tolist() == (v1.unplaced + v2.unplaced).tolist()
        assert not np.isin(p.pairs["kind"], (mf.PAIR_RESCUED_1, mf.PAIR_RESCUED_2)).any() and int(p.pair_records["rescued"].sum()) == 0
        assert int(p.align_records["gapped"].sum()) >= 20 and int(p.indels["del"].sum()) >= 20
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 4. where the aligning rescue's code path changes
EDGE_K, EDGE_WINDOW, EDGE_PERMILLE = 21, (1292, 1307), 400
EDGE_LENGTHS = (31, 32, 33, 63, 64, 65, 97, 994, 995)


def edge_bait():
    rng = random.Random(77)
    recs = [_rand(rng, 400), _rand(rng, 3000)]
    flank = [_rand(rng, 100), _rand(rng, 100)]
    return fasta([("small", recs[0]), ("long", recs[1])]), recs, flank


def edge_target(piece, n_at=None):
    """`piece` (one base more than the target) made a rescue target: another letter every 20 bases, so that no 21-mer of it is the
    bait's, and one base deleted nine bases from its end -- and, asked for, an N at offset n_at of the target"""
    t = substituted(piece, 20, 10)
    t = t[:len(t) - 10] + t[len(t) - 9:]
    return t if n_at is None else t[:n_at] + "N" + t[n_at + 1:]


@functools.lru_cache(maxsize=None)
def edge_pairs():
    """-> (text, seqs1, seqs2): on the long record (record 1) a clean forward 150-base mate 1 and a reverse target whose fragment ends
    1300 bases on, of every length of EDGE_LENGTHS; 97-base targets with an N at offsets 0, 31, 32, 63, 64 and L - 1; targets over the
    record's end by 5 and 37 bases, and -- mate 1 reverse, the target forward -- over its begin"""
    text, recs, flank = edge_bait()
    r = recs[1]
    whole = flank[0] + r + flank[1]
    at = lambda b, e: whole[100 + b:100 + e]
    s1, s2 = [], []
    for i, L in enumerate(EDGE_LENGTHS):
        a = 100 + 7 * i
        s1.append(at(a, a + 150)); s2.append(revcomp(edge_target(at(a + 1300 - L - 1, a + 1300))))
    for i, n_at in enumerate((0, 31, 32, 63, 64, 96)):
        a = 300 + 11 * i
        s1.append(at(a, a + 150)); s2.append(revcomp(edge_target(at(a + 1300 - 98, a + 1300), n_at)))
    for over in (5, 37):
        a = 3000 + over - 1300
        s1.append(at(a, a + 150)); s2.append(revcomp(edge_target(at(a + 1300 - 121, a + 1300))))
        s1.append(revcomp(at(1300 - over - 150, 1300 - over))); s2.append(edge_target(at(-over, -over + 121)))
    return text, s1, s2


def test_target_lengths_ns_and_overhangs_where_the_code_path_changes(mf, ol):
    text, s1, s2 = edge_pairs()
    o = po.PlaceOracle(text, EDGE_K)
    P = pao.PairAlignOracle(o)
    lo, hi = EDGE_WINDOW
    ks = mf.KmerSet.from_text(text, EDGE_K)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, 8, lo, hi, 1, EDGE_PERMILLE, 1, 64)
    gaps = want["aligns2"][:, 2] + want["aligns2"][:, 3]
    assert np.all(want["pairs"][:, 0] == pao.RESCUED_2) and int((gaps >= 1).sum()) >= 15 and np.all(gaps[3:9] >= 1)
    assert [len(s) for s in s2[:len(EDGE_LENGTHS)]] == list(EDGE_LENGTHS)
    p = check(mf.align_pairs(ks, r1, r2, lo, hi, 8, True, EDGE_PERMILLE, 1, 1000, gapped=True, extend=64), P, want, len(s1), 1, 8)
    assert int(p.extend_records["begin_piled"][1]) >= 5 + 37 - 2 and int(p.extend_records["end_piled"][1]) >= 5 + 37 - 2
    check(mf.align_pairs(ks, r2, r1, lo, hi, 8, True, EDGE_PERMILLE, 1, 1000, gapped=True, extend=64), P, want, len(s1), 1, 8, swapped=True)
    r1.close(); r2.close(); ks.close()


@functools.lru_cache(maxsize=None)
def long_target_pairs():
    """a uniform set of 150-base mates and a set whose one 1 200-base read is a rescue target (the others are 150-base proper mates): the
    rescue's work slice must go by the OTHER set's longest read"""
    text, recs, flank = edge_bait()
    r = recs[1]
    s1, s2 = [], []
    for i in range(6):
        a = 200 + 40 * i
        s1.append(r[a:a + 150]); s2.append(revcomp(r[a + 1300 - 150:a + 1300]))
    piece = r[100 + 1300 - 1201:100 + 1300]
    s1.append(r[100:250]); s2.append(revcomp(edge_target(piece)))
    return text, s1, s2


@pytest.mark.parametrize("swapped", [False, True])
def test_the_work_slice_goes_by_the_longer_set_s_longest_read(mf, ol, swapped):
    text, s1, s2 = long_target_pairs()
    o = po.PlaceOracle(text, EDGE_K)
    P = pao.PairAlignOracle(o)
    lo, hi = EDGE_WINDOW
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, 8, lo, hi, 1, EDGE_PERMILLE, 1, 8)
    assert want["pairs"][-1, 0] == pao.RESCUED_2 and len(s2[-1]) == 1200 and want["aligns2"][-1, 3] == 1
    ks = mf.KmerSet.from_text(text, EDGE_K)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    assert r1.info.uniform_len == 150
    a, b = (r2, r1) if swapped else (r1, r2)
    check(mf.align_pairs(ks, a, b, lo, hi, 8, True, EDGE_PERMILLE, 1, 1000, gapped=True, extend=8), P, want, len(s1), 1, 8, swapped=swapped)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 5. more targets than one turn of the rescue grid
@functools.lru_cache(maxsize=None)
def pool_pairs():
    """64 pairs of ragged reads of 33 .. 47 bases on record 1 of the edge bait; every other one a rescue target with a 1-base indel"""
    text, recs, flank = edge_bait()
    rng = random.Random(9)
    r = recs[1]
    pool = []
    for i in range(64):
        a, ins, L1, L2 = rng.randint(50, 1500), rng.randint(96, 104), rng.randint(33, 47), rng.randint(33, 47)
        m2 = r[a + ins - L2 - 1:a + ins]
        if i % 2:
            m2 = substituted(m2, 20, 10)
            m2 = (m2[:8] + m2[9:]) if i % 4 == 1 else (m2[2:8] + "ACGT"[rng.randrange(4)] + m2[8:])
        else:
            m2 = m2[1:]
        pool.append((r[a:a + L1], revcomp(m2)))
    return text, pool


def test_more_rescue_targets_than_one_turn_of_the_grid(mf, ol):
    text, pool = pool_pairs()
    k, band, lo, hi = 21, 8, 92, 107
    o = po.PlaceOracle(text, k)
    P = pao.PairAlignOracle(o)
    each = [P.pairs([a], [b], o.tally([a]), o.tally([b]), 1, 1000, band, lo, hi, 1, EDGE_PERMILLE, 1, 8) for a, b in pool]
    kinds = [int(w["pairs"][0, 0]) for w in each]
    assert kinds.count(pao.RESCUED_2) >= 24 and kinds.count(pao.PROPER) == 32
    assert sum(int(w["aligns2"][0, 2] + w["aligns2"][0, 3] > 0) for w, kd in zip(each, kinds) if kd == pao.RESCUED_2) >= 20
    assert {len(m) for pair in pool for m in pair} <= set(range(33, 48)) and len({len(b) for _, b in pool}) >= 10
    # the aligning rescue launches CUs * 32 waves at most, one listed target a wave a turn, and only half of the pool's pairs are targets:
    # three times that many pairs and 77 more list about one and a half turns of targets, so that a wave goes on to a second read of
    # another length in the slice its first one left
    waves = int(re.search(r"(\d+) CUs", mf.device_name(0)).group(1)) * 32
    n = 3 * waves + 77
    rng = random.Random(10)
    pick = np.array([rng.randrange(64) for _ in range(n)])
    times = np.bincount(pick, minlength=64)
    listed = sum(int(t) for t, w, kd in zip(times, each, kinds) if kd == pao.RESCUED_2 or w["why"][0] is not None)
    assert listed >= waves + waves // 4, (listed, waves)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, [pool[i][0] for i in pick]), upload(mf, ol, [pool[i][1] for i in pick])
    p = mf.align_pairs(ks, r1, r2, lo, hi, band, True, EDGE_PERMILLE, 1, 1000, gapped=True, extend=8)
    for name, got, fields in (("rows1", p.place1, PLACE_FIELDS), ("rows2", p.place2, PLACE_FIELDS), ("aligns1", p.align1, ALIGN_FIELDS), ("aligns2", p.align2, ALIGN_FIELDS),
                              ("pairs", p.pairs, ("kind", "insert"))):
        rows = np.stack([w[name][0] for w in each])
        assert np.array_equal(table(got, fields), rows[pick]), (name, first_bad(table(got, fields), rows[pick]))
    total = lambda name: sum(int(t) * np.asarray(w[name]).astype(np.int64) for t, w in zip(times, each))
    assert np.array_equal(p.base_depth.astype(np.int64), total("depth"))
    assert np.array_equal(table(p.indels, ("del", "ins", "ins_bases")), total("indels"))
    assert np.array_equal(table(p.pileup, ("a", "c", "g", "t")), total("counts"))
    assert np.array_equal(align_rows(p.align_records).astype(np.int64), total("align_rec"))
    assert np.array_equal(table(p.pair_records, PAIR_REC), total("pair_rec"))
    assert np.array_equal(np.stack([p.ins_pile[f].astype(np.int64) for f in "acgt"], axis=2), total("ins_pile"))
    assert np.array_equal(np.stack([p.ext_pile[f].astype(np.int64) for f in "acgt"], axis=3), total("ext_pile"))
    assert np.array_equal(table(p.place_records, PLACE_REC)[:, :4], total("place_rec")[:, :4])
    assert p.unplaced.tolist() == [sum(int(t) * w["unplaced"][q] for t, w in zip(times, each)) for q in (0, 1)]
    identities(p)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 6. more records than the pair list gathers in LDS
def test_more_than_170_records_pair_records_row_for_row(mf, ol):
    rng = random.Random(171)
    recs = [_rand(rng, 120) for _ in range(171)]
    text = fasta([("s%d" % j, r) for j, r in enumerate(recs)])
    k, band, lo, hi = 21, 4, 80, 110
    s1, s2 = [], []
    for j, r in enumerate(recs):
        for q in range(2 + j % 3):
            ins = rng.randint(lo - 6, hi + 4)
            m2 = r[max(ins - 40, 0):ins]
            if (j + q) % 4 == 0:
                m2 = m2[:15] + m2[17:]          # a deletion that the cut at 30 rejects ungapped
            elif (j + q) % 4 == 1:
                m2 = substituted(m2, 20, 10)          # a rescue target
            elif (j + q) % 7 == 2:
                m2 = recs[(j + 5) % 171][60:100]          # the other mate on another record
            s1.append(r[:40]); s2.append(revcomp(m2))
    o = po.PlaceOracle(text, k)
    P = pao.PairAlignOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    for max_permille in (1000, 30):
        want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, max_permille, band, lo, hi, 1, 200, 1, 8)
        assert (want["pair_rec"][:, :5].sum(axis=0) >= 20).all(), want["pair_rec"].sum(axis=0)
        check(mf.align_pairs(ks, r1, r2, lo, hi, band, True, 200, 1, max_permille, gapped=True, extend=8), P, want, len(s1), 1, band)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 7. what the feature buys
BUY_K, BUY_PERMILLE, BUY_DEL, BUY_INS = 31, 450, (360, 363), 460


@functools.lru_cache(maxsize=None)
def indel_sample():
    """-> (bait text, the bait's r0, the sample's r0 in its own coordinates, seqs1, seqs2): the bait and the sample of pair_data.pair_bait(),
    the sample with three bases of the diverged stretch deleted and two inserted behind BUY_INS, and 240 pairs with one mate in r0's own
    first bases and the other inside the stretch -- the only reads that cover it"""
    text, recs, sample = pair_data.pair_bait()
    rng = random.Random(12)
    s0 = sample[0][pair_data.FLANK:pair_data.FLANK + 900]
    own = s0[:BUY_DEL[0]] + s0[BUY_DEL[1]:BUY_INS] + "".join("ACGT"[("ACGT".index(c) + 1) % 4] for c in s0[BUY_INS - 2:BUY_INS]) + s0[BUY_INS:]
    s1, s2 = [], []
    for i in range(240):
        a, ins = rng.randint(140, 150), rng.randint(300, 345)          # (the mate begins at 290 or later: it holds no k-mer of the bait)
        s1.append(own[a:a + 150]); s2.append(revcomp(own[a + ins - 150:a + ins]))
    return text, recs[0], own, s1, s2


@functools.lru_cache(maxsize=None)
def window_pairs():
    """60 pairs with both mates in r2's own last bases, inserts 300 .. 345: the pairs the vote places, from which the window is estimated"""
    text, recs, sample = pair_data.pair_bait()
    rng = random.Random(13)
    r2 = recs[2]
    s1, s2 = [], []
    for i in range(60):
        a, ins = rng.randint(430, 470), rng.randint(300, 345)
        s1.append(r2[a:a + 150]); s2.append(revcomp(r2[a + ins - 150:a + ins]))
    return s1, s2


def test_the_rescued_mates_call_the_indels_of_a_diverged_stretch(mf, ol, tmp_path):
    from mitoflex_amd.bim import bim
    from tests.util_data import write_fastq
    text, r0, own, s1, s2 = indel_sample()
    lo, hi = pair_data.WINDOW
    bait, fq1, fq2, out = str(tmp_path / "bait.fa"), str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), str(tmp_path / "out.fa")
    open(bait, "w").write(text)
    write_fastq(fq1, s1, "p")
    write_fastq(fq2, s2, "p")
    record0 = lambda: "".join(open(out).read().split(">r1")[0].splitlines()[1:])
    a, b = 346, 470          # across both indels, inside what the mates cover
    # pairs with a band: the stretch is the SAMPLE's, letter for letter and in the sample's coordinates; the record has the sample's length
    bim.consensus_bait_pairs(bait, fq1, fq2, out, kmer=BUY_K, min_depth=2, band=8, gapped=True, min_insert=lo, max_insert=hi, rescue_permille=BUY_PERMILLE)
    both = record0()
    assert len(both) == len(own) == 899 and both[a:b] == own[a:b] and own[a:b] != r0[a:b]
    # the same with the window estimated: a first call without rescue over the pairs the vote places (here those of r2), then the rescue
    w1, w2 = window_pairs()
    write_fastq(str(tmp_path / "wa.fq"), s1 + w1, "p")
    write_fastq(str(tmp_path / "wb.fq"), s2 + w2, "p")
    bim.consensus_bait_pairs(bait, str(tmp_path / "wa.fq"), str(tmp_path / "wb.fq"), out, kmer=BUY_K, min_depth=2, band=8, gapped=True, rescue_permille=BUY_PERMILLE)
    estimated = record0()
    assert estimated[a:b] == own[a:b]          # (the window's quantiles leave a few mates out: the stretch is the sample's all the same)
    # pairs without a band: the rescued mates are there, on their diagonals: the bait's length, and wrong letters behind the deletion
    bim.consensus_bait(bait, fq1, fq2, out, kmer=BUY_K, min_depth=2, pairs=True, min_insert=lo, max_insert=hi, rescue_permille=BUY_PERMILLE)
    ungapped = record0()
    assert len(ungapped) == 900 and ungapped[a:BUY_DEL[0]].isupper()
    # (most of these mates have their longer side behind the deletion, where the sample's letters lie at the bait's coordinates again:
    # the seed lies there, and the bases before the deletion are piled three columns off)
    wrong = sum(x.upper() != y for x, y in zip(ungapped[BUY_DEL[0] - 40:BUY_DEL[0]], own[BUY_DEL[0] - 40:BUY_DEL[0]]))
    assert wrong >= 10 and both[BUY_DEL[0] - 40:BUY_DEL[0]] == own[BUY_DEL[0] - 40:BUY_DEL[0]], wrong
    # a band without pairs: no read is placed there, the stretch keeps the bait's letters in lower case
    bim.consensus_bait(bait, fq1, fq2, out, kmer=BUY_K, min_depth=2, band=8, gapped=True)
    alone = record0()
    assert len(alone) == 900 and alone[a:b].islower() and alone[a:b].upper() == r0[a:b]


# ------------------------------------------------------------------ 8. the CLI
def test_the_cli_writes_the_existing_formats_for_the_oracle_s_tables(mf, ol, tmp_path):
    import filecmp
    import os
    import subprocess
    from tests import align_text, extend_text, gapped_text
    from tests.util_data import write_fastq
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mitoflex_amd", "assemble", "fastfilter")
    k, band = 21, 8
    text, o, P = data_oracle(k)[:3]
    s1, s2, what = pad.pair_set(mixed=True)
    t = lambda n: str(tmp_path / n)
    open(t("bait.fa"), "w").write(text)
    write_fastq(t("a.fq"), s1, "p")
    write_fastq(t("b.fq"), s2, "p")
    names, starts = ["r0", "r1", "r2"], o.starts
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, band, LO, HI, 1, pad.RESCUE_PERMILLE, 2, 8)
    base = [cli, "pairs", "--bait", t("bait.fa"), "-k", str(k), "--fq1", t("a.fq"), "--fq2", t("b.fq"), "--min-insert", str(LO), "--max-insert", str(HI),
            "--min-depth", "2", "--rescue-permille", str(pad.RESCUE_PERMILLE)]
    r = subprocess.run(base + ["--band", str(band), "--indels", t("indels.tsv"), "--gapped-consensus", t("gapped.fa"), "--insertions", t("ins.tsv"), "--extend", "8",
                               "--extended-consensus", t("x.fa"), "--extension-report", t("x.tsv"), "--score-report", t("score.tsv"), "--consensus", t("cons.fa"),
                               "--pair-report", t("pairs.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == int(want["pair_rec"][:, 3].sum()) >= 100
    depth = np.minimum(want["depth"], po.CLAMP)
    assert open(t("score.tsv")).read() == align_text.align_report_text(names, starts, want["align_rec"])
    assert open(t("indels.tsv")).read() == align_text.indels_text(names, starts, depth, want["indels"]) and len(open(t("indels.tsv")).read().splitlines()) > 50
    assert open(t("gapped.fa")).read() == gapped_text.gapped_fasta(names, want["gapped_starts"], want["gapped"])
    assert open(t("ins.tsv")).read() == gapped_text.insertions_text(names, starts, depth, want["ins_pile"]) and len(open(t("ins.tsv")).read().splitlines()) > 20
    assert open(t("x.fa")).read() == extend_text.extended_fasta(names, want["extended_starts"], want["extended"])
    assert open(t("x.tsv")).read() == extend_text.extension_text(names, want["ext_pile"]) and len(open(t("x.tsv")).read().splitlines()) > 20
    assert open(t("cons.fa")).read() == mf.consensus_fasta(names, starts, pio.PileupOracle(o).call(want["counts"], 2)[0])
    # without --band the line makes mf_place_pairs' call and writes its files
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    v = mf.place_pairs(ks, r1, r2, LO, HI, True, pad.RESCUE_PERMILLE, 2)
    q = subprocess.run(base + ["--score-report", t("score0.tsv"), "--consensus", t("cons0.fa"), "--pair-report", t("pairs0.tsv")], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and int(q.stdout) == int(v.pair_records["rescued"].sum())
    assert open(t("score0.tsv")).read().startswith("record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tpermille\t")
    assert open(t("cons0.fa")).read() == mf.consensus_fasta(names, starts, v.consensus)
    z = subprocess.run(base + ["--band", "0", "--score-report", t("score1.tsv"), "--consensus", t("cons1.fa"), "--pair-report", t("pairs1.tsv")], capture_output=True, text=True, timeout=120)
    assert z.returncode == 0 and z.stdout == q.stdout and filecmp.cmp(t("cons0.fa"), t("cons1.fa"), shallow=False) and filecmp.cmp(t("pairs0.tsv"), t("pairs1.tsv"), shallow=False)
    # the bait subcommand's dependency rules
    for extra in (["--indels", t("no")], ["--gapped-consensus", t("no")], ["--extend", "8"], ["--band", "8", "--extended-consensus", t("no")], ["--band", "21"], ["--band", "32"]):
        e = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert e.returncode == 1 and e.stderr.startswith("error: ") and not os.path.exists(t("no")), extra
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 9. the refusals that need handles
def test_refusals_that_need_handles(mf, ol):
    text = data_oracle(21)[0]
    s1, s2, what = pad.pair_set()
    ks = mf.KmerSet.from_text(text, 21)
    r1, r2, r3 = upload(mf, ol, s1[:10]), upload(mf, ol, s2[:10]), upload(mf, ol, s2[:9])
    with pytest.raises(ValueError, match="length"):
        mf.align_pairs(ks, r1, r3, LO, HI)
    with pytest.raises(mf.MitoFilterError, match="band is 21"):
        mf.align_pairs(ks, r1, r2, LO, HI, band=21)
    L = mf.load()

    def raw(ks_h, a, b, band=8):
        return L.mf_align_pairs(ks_h, a, b, 1, 0, 1, 1000, band, 0, LO, HI, 1, 100, *([None] * 26))

    assert raw(ks._h, r1._h, r3._h) == -1 and b"mate" in L.mf_last_error()
    assert raw(ks._h, r1._h, r1._h) == -1 and b"one read set" in L.mf_last_error()
    assert raw(ks._h, r1._h, None) == -1 and b"NULL" in L.mf_last_error()
    assert raw(ks._h, r1._h, r2._h, 21) == -1 and b"below k" in L.mf_last_error()
    from tests.util_data import make_protein_bait
    pks = mf.KmerSet.protein_from_text(make_protein_bait()[0], 7, 5)
    assert raw(pks._h, r1._h, r2._h) == -1 and b"nucleotide" in L.mf_last_error()
    pks.close()
    # every output is optional; band k - 1 is the widest
    assert raw(ks._h, r1._h, r2._h) == 0 and raw(ks._h, r1._h, r2._h, 20) == 0
    r1.close(); r2.close(); r3.close(); ks.close()
