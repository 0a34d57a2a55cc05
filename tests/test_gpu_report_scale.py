"""The placement family (mf_place, mf_pileup, mf_verify, mf_filter_fastq_files_placed) and the assignment reports (mf_assign,
mf_assign_groups) on baits of the size the library is given, against the plain-Python oracles, exactly: a bait of more than 256 scan tiles
and more than 2048 records (tests/scale_data.py), and baits whose record count puts the gathered counters just below and just above the
LDS histogram's limit.  What the bait and the reads are built to reach is asserted from the oracle's results before the device is asked.

Two things are not as the issue that asked for these tests words them:
- No read can lie on a record shorter than 16 positions at k = 31 (such a record holds no window, so no anchor).  test_pileup_at_scale
  therefore also runs a small bait of the same shape at k = 13, where records of 13 .. 15 positions take reads.
- place_kernel launches min(32 waves a CU, reads) waves, so with a few thousand reads every wave places ONE read, and neither the run
  in GatheredCounts::bump nor the packed sums of a run of accepted reads ever hold more than one read.  A wave takes the listed reads
  i, i + waves, i + 2 waves, ..: test_verify_at_scale and test_place_at_scale therefore also run 65 536 copies of a few reads in blocks
  long enough that every wave meets each pattern at any stride up to 8 192 waves (256 CUs).  Their oracle results are those of the
  distinct reads times their copies: every output but `covered` is a sum over the reads."""
import time

import numpy as np
import pytest

from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests import verify_oracle as vo
from tests.report_data import mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.scale_data import (TILE, WAVE_SPAN, THREAD_SPAN, bound_carry_read, many_segment_read, scale_bait, scale_reads, short_record_bait,
                              short_record_reads)
from tests.test_gpu_assign import oracle_assign, owners
from tests.test_gpu_place import check as check_place
from tests.test_gpu_place import in_memory, rec_rows, rows_of, summed
from tests.test_gpu_verify import PILE_REC, PLACE_REC, counts_of, identities, score_rows, substituted
from tests.test_gpu_verify import rec_rows as rec_rows_of
from tests.util_data import bits_to_bool, revcomp, write_fastq

pytestmark = pytest.mark.gpu

K = 31
HIST_MAX = 8192                  # mf_tally_dev.h: counters up to this gather in LDS
SCORE_GATHERED = 33              # mf_placelayout.h: rejected and the 32 bins of every record
MAX_WAVES = 8192                 # 32 waves a CU on 256 CUs
EDGE = 256 * TILE                # the first position of the scan's second turn over the tile sums


# ------------------------------------------------------------------ the scale bait, its oracles and its reads: once
class Scale:
    def __init__(self):
        t0 = time.time()
        self.text, self.parts = scale_bait(K)
        self.o = po.PlaceOracle(self.text, K)
        self.V = vo.VerifyOracle(self.o)
        self.P = self.V.P
        self.starts = np.asarray(self.o.starts, np.int64)
        self.lens = np.asarray(self.o.lens, np.int64)
        self.total, self.R = int(self.starts[-1]), len(self.o.recs)
        self._tally = {}
        p = self.parts
        left, right, sc = p["seqs"][p["left"]], p["seqs"][p["right"]], p["seqs"][p["scaffold"]]
        rng = np.random.default_rng(3)
        rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
        rec_k = next(s for s in p["seqs"] if len(s) == K)
        rec_64 = p["seqs"][p["quiet"]]
        a, b = left[100:250], right[200:350]
        self.special = {
            "over_both": rnd(30) + left + rnd(30),
            "junction": left[-80:] + right[:70],
            "over_begin": rnd(40) + right[:100],
            "over_end": revcomp(right[-90:] + rnd(50)),
            "scaffold_end": sc[-100:] + rnd(45),
            "whole_k_record": rnd(50) + rec_k + rnd(50),
            # two reads that differ in one letter and nothing else on the spot: exact ties in a record of 64 positions, behind and in front
            # of the 256th tile
            "tie_64_1": rnd(20) + rec_64 + rnd(20), "tie_64_2": revcomp(rnd(20) + substituted(rec_64, (5,)) + rnd(20)),
            "tie_left_1": left[300:450], "tie_left_2": revcomp(substituted(left[300:450], (70,))),
            "tie_front_1": sc[1000:1150], "tie_front_2": substituted(sc[1000:1150], (5, 140)),
        }
        # (verification) runs, alternations and rejected reads in read order, from copies of a few reads
        a1, rej_a, rej_b = substituted(a, (77,)), substituted(a, range(5, 55, 5)), substituted(b, range(100, 150, 5))
        self.pattern = [a, a1, a] * 100 + [a, b] * 150 + [a, rej_a, b, rej_b] * 100 + [revcomp(b)] * 50
        self.pattern_at = len(self.special)
        self.sets = {"ragged": list(self.special.values()) + self.pattern + scale_reads(p, K, 3000, seed=11, uniform=False),
                     "uniform": scale_reads(p, K, 2600, seed=12, uniform=True)}
        self.tallies = {n: self.tally(s) for n, s in self.sets.items()}
        # the copies in blocks (see the module's text): accepted on `left`, rejected on `left`, accepted on `left`, on `right`, rejected there
        self.block_uniq = [a, a1, rej_a, b, substituted(b, (3, 90)), rej_b]
        n, mix = MAX_WAVES, lambda m: np.array([0, 1, 0])[np.arange(m) % 3]
        self.block_idx = np.concatenate([mix(3 * n), np.full(n, 2), mix(n), 3 + mix(2 * n), np.full(n, 5)])
        assert len(self.block_idx) == 65536          # (one workgroup of the list kernel: the list is in read order)
        self.seconds = time.time() - t0

    def tally(self, seqs):
        for s in seqs:
            if s not in self._tally:
                self._tally[s] = self.o.votes(s) + (len(s),)
        return [self._tally[s] for s in seqs]


@pytest.fixture(scope="module")
def scale():
    s = Scale()
    print("scale bait: %d positions, %d records; bait, oracles and tallies in %.1f s" % (s.total, s.R, s.seconds))
    return s


@pytest.fixture(scope="module")
def scale_ks(mf, scale):
    ks = mf.KmerSet.from_text(scale.text, K)
    assert np.array_equal(ks.record_starts, scale.o.starts)
    yield ks
    ks.close()


def per_record(starts, x):
    """the sum of x over every record's positions (empty records: 0)"""
    c = np.concatenate([[0], np.cumsum(np.asarray(x, np.int64))])
    return c[starts[1:]] - c[starts[:-1]]


def bait_facts(S):
    """what the bait is built to hold, from the oracle's record starts"""
    starts, lens, p = S.starts, S.lens, S.parts
    assert S.total > 257 * TILE and S.R >= 2100 and 4 * S.R + 1 > HIST_MAX
    inner = starts[1:-1][(lens[:-1] > 0) & (lens[1:] > 0)]          # a boundary of two records that both hold positions
    assert (inner % THREAD_SPAN == 0).any() and (inner % WAVE_SPAN == 0).any() and (inner % TILE == 0).any()
    for j, m in p["pads"]:
        assert starts[j + 1] % m == 0 and lens[j] > 0 and lens[j + 1] > 0
    runs = p["tiny_runs"]
    assert runs[0][0] == 0 and runs[-1][0] + runs[-1][1] == S.R and lens[-1] == 0 and len(runs) >= 5
    for j, n in runs:
        assert 3 <= n <= 6 and (lens[j:j + n] < 16).all() and (lens[j:j + n] == 0).any()
    assert any(0 < starts[j] % TILE < WAVE_SPAN and starts[j] > TILE for j, n in runs)          # a run in the first wave of a tile inside the bait
    for n in (0, 1, 5, 15, 16, 17, K - 1, K, K + 1, 64, 150):
        assert (lens == n).any(), n
    sc = p["scaffold"]
    assert starts[sc] + p["front"] < EDGE - 100 * TILE and starts[sc] + p["front"] + p["gap"] < EDGE < starts[sc + 1] - 10000 < starts[p["left"]]
    assert any("N" in S.o.recs[j] for j in range(sc)) and len(p["shared"]) >= 5


def place_facts(S, name, tallies, thr):
    """what the reads are drawn to reach, from the oracle's placement alone"""
    _, rows, depth, rec, _ = S.o.place(tallies, thr)
    starts, lens, p = S.starts, S.lens, S.parts
    placed = rows[:, 0] < po.AMBIGUOUS
    j = rows[placed, 0]
    assert len(np.unique(j)) >= (1000 if name == "uniform" else 500), len(np.unique(j))
    at = starts[j] + np.maximum(rows[placed, 2], 0)
    assert (at < EDGE).sum() >= 100 and (at >= EDGE).sum() >= 100, ((at < EDGE).sum(), (at >= EDGE).sum())
    last = (S.total - 1) // TILE
    for t in (0, 255, 256, last):
        assert depth[t * TILE:(t + 1) * TILE].any(), t
    behind = starts[j] >= EDGE
    assert (behind & (rows[placed, 2] < 0)).any() and (behind & (rows[placed, 3] > lens[j])).any()
    if name == "ragged":
        r = dict(zip(S.special, rows))
        L, Rt = p["left"], p["right"]
        assert r["junction"].tolist()[:4] == [L, 0, 520, 670] and starts[L] + 600 == starts[Rt] and starts[Rt] > EDGE       # its -1 on `right`'s first position
        assert r["over_both"].tolist()[:4] == [L, 0, -30, 630] and r["over_begin"].tolist()[:4] == [Rt, 0, -40, 100]
        assert r["over_end"].tolist()[:4] == [Rt, 1, 510, 650]
        assert r["scaffold_end"].tolist()[:2] == [p["scaffold"], 0] and r["scaffold_end"][3] == lens[p["scaffold"]] + 45
        if thr == 1:          # (one window: it passes at threshold 1 only)
            assert lens[r["whole_k_record"][0]] == K and r["whole_k_record"][2] == -50
    return rows, depth, rec


def copies_expected(S, uniq, idx, thr, max_permille):
    """the oracle's verification of uniq[idx[0]], uniq[idx[1]], ..: each distinct read verified alone, every sum times its copies"""
    one = [S.V.verify([s], S.tally([s]), thr, max_permille) for s in uniq]
    mult = np.bincount(idx, minlength=len(uniq))
    want = {f: np.concatenate([w[f] for w in one])[idx] for f in ("passes", "rows", "scores", "accepted")}
    for f in ("depth", "counts", "place_rec", "score_rec"):
        want[f] = sum(int(m) * w[f].astype(np.int64) for m, w in zip(mult, one))
    want["place_rec"][:, 4] = per_record(S.starts, want["depth"] > 0)
    want["place_rec"], want["score_rec"] = want["place_rec"].astype(np.uint64), want["score_rec"].astype(np.uint64)
    want["unplaced"] = [sum(int(m) * w["unplaced"][i] for m, w in zip(mult, one)) for i in (0, 1)]
    return want


def wave_patterns(want, stride):
    """(a run of three accepted reads on one record, a change of record between two accepted reads, accepted reads of a record in front of
    and behind rejected ones of it) among the reads i, i + stride, i + 2 stride that one wave takes"""
    rec, acc = want["rows"][:, 0], want["accepted"]
    placed = rec < po.AMBIGUOUS
    a, b, c = slice(0, -2 * stride), slice(stride, -stride), slice(2 * stride, None)
    run = acc[a] & acc[b] & acc[c] & (rec[a] == rec[b]) & (rec[b] == rec[c])
    change = acc[a] & acc[b] & (rec[a] != rec[b])
    rej = placed & ~acc
    between = (acc[a] & rej[b] & (rec[a] == rec[b])).any() and (rej[a] & acc[b] & (rec[a] == rec[b])).any()
    return bool(run.any()), bool(change.any()), bool(between)


# ------------------------------------------------------------------ a. placement
def test_place_at_scale(mf, ol, scale, scale_ks):
    S = scale
    bait_facts(S)
    spent = 0.0
    for name, seqs in S.sets.items():
        for thr in (1, 3):
            place_facts(S, name, S.tallies[name], thr)
        reads = upload(mf, ol, seqs)
        t0 = time.time()
        for thr in (1, 3):
            check_place(mf, scale_ks, reads, S.o, S.tallies[name], thr, mf.MODE_SCREENED)
        spent += time.time() - t0
        reads.close()
    # copies in blocks: every wave bumps runs of one record's counter, through the global branch of the gathered counts
    want = copies_expected(S, S.block_uniq, S.block_idx, 1, 1000)
    assert (want["rows"][:, 0] < po.AMBIGUOUS).all()
    for stride in (1, MAX_WAVES // 2, MAX_WAVES):
        assert wave_patterns(want, stride)[:2] == (True, True)
    reads = upload(mf, ol, [S.block_uniq[i] for i in S.block_idx])
    t0 = time.time()
    bits, place, base_depth, records, unpl = mf.place_reads(scale_ks, reads, 1)
    spent += time.time() - t0
    reads.close()
    assert bits_to_bool(bits, len(S.block_idx)).all() and np.array_equal(rows_of(place), want["rows"])
    assert np.array_equal(base_depth.astype(np.int64), want["depth"]) and np.array_equal(rec_rows(records), want["place_rec"])
    assert unpl.tolist() == [0, 0]
    print("test_place_at_scale: device calls %.2f s" % spent)


# ------------------------------------------------------------------ b. pile-up
def check_pileup(mf, ks, reads, P, n, want, thr, min_depth, call):
    passes, rows, unplaced, counts = want
    cons, rec = call(counts, min_depth)
    bits, pileup, consensus, records, unpl = mf.pileup_reads(ks, reads, thr, mf.MODE_SCREENED, min_depth)
    assert np.array_equal(bits_to_bool(bits, n), passes)
    got = np.stack([pileup[f].astype(np.int64) for f in ("a", "c", "g", "t")], axis=1)
    bad = np.nonzero((got != pio.clamped(counts)).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), counts[i].tolist()) for i in bad[:10]]
    bad = np.nonzero(consensus != cons)[0]
    assert bad.size == 0, [(int(i), chr(consensus[i]), chr(cons[i]), counts[i].tolist()) for i in bad[:10]]
    got = rec_rows_of(records, PILE_REC)
    bad = np.nonzero((got != rec).any(axis=1))[0]
    assert bad.size == 0, [(int(j), got[j].tolist(), rec[j].tolist()) for j in bad[:10]]
    assert unpl.tolist() == unplaced
    return cons, rec


def test_pileup_at_scale(mf, ol, scale, scale_ks):
    S = scale
    p = S.parts
    spent = 0.0
    for name, seqs in S.sets.items():
        reads = upload(mf, ol, seqs)
        for thr in (1, 3):
            passes, rows, _, _, unplaced = S.o.place(S.tallies[name], thr)
            counts = S.P.pile(seqs, rows)
            for min_depth in (1, 3):
                cons, rec = S.P.call_fast(counts, min_depth)
                if min_depth == 1:
                    ref = np.frombuffer(S.P.bait.encode(), np.uint8)
                    v = np.nonzero(np.isin(cons, list(b"ACGT")) & (ref != ord("N")) & (cons != ref))[0]
                    assert len(v) == int(rec[:, 5].sum()) and (v < EDGE).any() and (v >= EDGE).any()                 # variants on both sides of the 256th tile
                    assert (S.lens[np.nonzero(rec[:, 5])[0]] <= 64).any()                                             # and in a short record
                if name == "ragged" and min_depth == 1:
                    t = np.nonzero((cons == ord("N")) & (counts.sum(axis=1) > 0))[0]
                    assert (t < EDGE).any() and (t >= EDGE).any() and int(rec[p["quiet"], 4]) == 1                     # ties on both sides, one in a record of 64 positions
                gap0 = int(S.starts[p["scaffold"]]) + p["front"]
                inside = cons[gap0:gap0 + p["gap"]]
                assert p["gap"] > 500000 and (inside == ord("n")).all()                                                   # nothing is called inside the gap
                t0 = time.time()
                check_pileup(mf, scale_ks, reads, S.P, len(seqs), (passes, rows, unplaced, counts), thr, min_depth, S.P.call_fast)
                spent += time.time() - t0
        reads.close()
    # records shorter than 16 positions that take reads: a small bait of the same shape at k = 13, against the plain call
    k = 13
    text, parts = scale_bait(k, n_block=140, front=1500, back=900, gap=700)
    o = po.PlaceOracle(text, k)
    P = pio.PileupOracle(o)
    seqs = scale_reads(parts, k, 900, seed=5, uniform=False, read_len=60) + scale_reads(parts, k, 300, seed=6, uniform=True, read_len=40)
    tallies = o.tally(seqs)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    reads = upload(mf, ol, seqs)
    for min_depth in (1, 3):
        passes, rows, _, _, unplaced = o.place(tallies, 1)
        counts = P.pile(seqs, rows)
        _, rec = P.call(counts, min_depth)
        small = np.asarray(o.lens) < 16
        assert int((rec[small, 0] > 0).sum()) >= 3 and int(rec[small, 2].sum()) > 0          # bases, and mismatches, on records shorter than 16
        t0 = time.time()
        check_pileup(mf, ks, reads, P, len(seqs), (passes, rows, unplaced, counts), 1, min_depth, P.call)
        spent += time.time() - t0
    reads.close(); ks.close()
    print("test_pileup_at_scale: device calls %.2f s" % spent)


# ------------------------------------------------------------------ c. verification
def check_verify(mf, ks, reads, n, want, thr, min_depth, max_permille, call):
    v = mf.verify_reads(ks, reads, thr, mf.MODE_SCREENED, min_depth, max_permille)
    assert np.array_equal(bits_to_bool(v.bits, n), want["passes"])
    got = rows_of(v.place)
    bad = np.nonzero((got != want["rows"]).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["rows"][i].tolist()) for i in bad[:10]]
    got = np.stack([v.score["compared"], v.score["mismatches"]], axis=1).astype(np.int64)
    bad = np.nonzero((got != want["scores"]).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["scores"][i].tolist()) for i in bad[:10]]
    bad = np.nonzero(v.base_depth.astype(np.int64) != np.minimum(want["depth"], po.CLAMP))[0]
    assert bad.size == 0, [(int(i), int(v.base_depth[i]), int(want["depth"][i])) for i in bad[:10]]
    for got, exp in ((rec_rows_of(v.place_records, PLACE_REC), want["place_rec"]), (score_rows(v.score_records), want["score_rec"])):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, [(int(j), got[j].tolist(), exp[j].tolist()) for j in bad[:5]]
    got = counts_of(v.pileup)
    bad = np.nonzero((got != pio.clamped(want["counts"])).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["counts"][i].tolist()) for i in bad[:10]]
    cons, rec = call(want["counts"], min_depth)
    assert np.array_equal(v.consensus, cons)
    assert np.array_equal(rec_rows_of(v.pileup_records, PILE_REC), rec)
    assert v.unplaced.tolist() == list(want["unplaced"])
    identities(v, n)


def test_verify_at_scale(mf, ol, scale, scale_ks):
    S = scale
    seqs, tallies = S.sets["ragged"], S.tallies["ragged"]
    reads = upload(mf, ol, seqs)
    spent, cut = 0.0, {}
    for max_permille in (1000, 30, 0):
        want = S.V.verify(seqs, tallies, 1, max_permille)
        if max_permille == 30:
            # in read order: a long run of accepted reads on one record, alternations between two records, rejected reads among both
            lo, hi = S.pattern_at, S.pattern_at + len(S.pattern)
            rec, acc = want["rows"][lo:hi, 0], want["accepted"][lo:hi]
            L, Rt = S.parts["left"], S.parts["right"]
            assert (rec[:300] == L).all() and acc[:300].all() and len(set(map(tuple, want["scores"][lo:lo + 3]))) == 2
            assert rec[300:600].tolist() == [L, Rt] * 150 and acc[300:600].all()
            assert rec[600:1000].tolist() == [L, L, Rt, Rt] * 100 and acc[600:1000].tolist() == [True, False, True, False] * 100
            acc_all, rec_all = want["accepted"], want["rows"][:, 0]
            assert (acc_all & (S.starts[np.minimum(rec_all, S.R - 1)] < EDGE)).sum() > 100 and (~acc_all & (rec_all < po.AMBIGUOUS)).sum() > 200
        cut[max_permille] = int(want["score_rec"][:, 1].sum())
        t0 = time.time()
        check_verify(mf, scale_ks, reads, len(seqs), want, 1, 2, max_permille, S.P.call_fast)
        spent += time.time() - t0
    assert cut[1000] == 0 < cut[30] < cut[0]
    reads.close()
    # copies in blocks: what one wave takes holds the run, the change of record and the rejected read between, at any stride
    want = copies_expected(S, S.block_uniq, S.block_idx, 1, 30)
    for stride in (1, MAX_WAVES // 4, MAX_WAVES // 2, MAX_WAVES):
        assert wave_patterns(want, stride) == (True, True, True), stride
    assert len({tuple(s) for s in want["scores"][want["accepted"]]}) >= 3          # the sums of a run are of reads that differ
    reads = upload(mf, ol, [S.block_uniq[i] for i in S.block_idx])
    t0 = time.time()
    check_verify(mf, scale_ks, reads, len(S.block_idx), want, 1, 2, 30, S.P.call_fast)
    spent += time.time() - t0
    reads.close()
    print("test_verify_at_scale: device calls %.2f s" % spent)


# ------------------------------------------------------------------ d. the counters on either side of the LDS limit: placement, verification
@pytest.mark.parametrize("n_rec,verify", [(221, True), (222, True), (2047, False), (2048, False)])
def test_verify_counters_at_the_lds_limit(mf, ol, n_rec, verify):
    n_counters = (4 + (SCORE_GATHERED if verify else 0)) * n_rec + 1
    assert (n_counters <= HIST_MAX) == (n_rec in (221, 2047)) and abs(n_counters - HIST_MAX) <= 23
    text, recs = short_record_bait(n_rec, 60, seed=77)
    o = po.PlaceOracle(text, K)
    ks = mf.KmerSet.from_text(text, K)
    assert len(o.recs) == n_rec and np.array_equal(ks.record_starts, o.starts)
    # the last records above all: their counters are the ones beyond the limit
    seqs = short_record_reads(recs, K, 1100, seed=n_rec) + short_record_reads(recs, K, 400, seed=n_rec + 1, lo=n_rec - 40)
    tallies = o.tally(seqs)
    reads = upload(mf, ol, seqs)
    t0 = time.time()
    if verify:
        V = vo.VerifyOracle(o)
        for max_permille in (1000, 30):
            want = V.verify(seqs, tallies, 1, max_permille)
            assert len(np.unique(want["rows"][want["accepted"], 0])) > 150 and int(want["score_rec"][-40:, :2].sum()) > 300
            assert (max_permille == 1000) == (int(want["score_rec"][:, 1].sum()) == 0) and int(want["score_rec"][-1, 4:].sum()) > 0
            check_verify(mf, ks, reads, len(seqs), want, 1, 2, max_permille, V.P.call)
    else:
        for thr in (1, 3):
            rows = check_place(mf, ks, reads, o, tallies, thr, mf.MODE_SCREENED)
            placed = rows[rows[:, 0] < po.AMBIGUOUS]
            assert len(np.unique(placed[:, 0])) > 500 and (placed[:, 0] == n_rec - 1).any() and (placed[:, 2] < 0).any()
            assert (placed[placed[:, 0] == n_rec - 1, 3] > o.lens[-1]).any()          # over_end of the last record: the last counter but one
    print("test_verify_counters_at_the_lds_limit[%d]: oracle and device calls %.2f s" % (n_rec, time.time() - t0))
    reads.close(); ks.close()


# ------------------------------------------------------------------ e. the counters on either side of the LDS limit: assignment
@pytest.mark.parametrize("n_rec", [8191, 8192])
def test_assign_counters_at_the_lds_limit(mf, ol, n_rec):
    k = 21
    assert (n_rec + 1 <= HIST_MAX) == (n_rec == 8191)
    text, recs = short_record_bait(n_rec, 40, seed=78)
    seqs = short_record_reads(recs, k, 1500, seed=n_rec, sub_rate=0.01) + short_record_reads(recs, k, 500, seed=n_rec + 1, sub_rate=0.01, lo=8000)
    seqs += [recs[j][:30] + recs[j + 1][:30] for j in range(8100, 8120)]          # ten windows unique to each of two records: ambiguous
    passes, oassign, ocounts = oracle_assign(seqs, k, owners(text, k), 1, n_rec)
    assert int(((oassign >= 8000) & (oassign < n_rec)).sum()) > 300 and int(ocounts[n_rec - 1]) > 0 and int(ocounts[n_rec]) >= 10
    assert len(np.unique(oassign)) > 1000
    ks = mf.KmerSet.from_text(text, k)
    assert len(ks.record_names) == n_rec
    reads = upload(mf, ol, seqs)
    t0 = time.time()
    for thr in (1, 3):
        passes, oassign, ocounts = oracle_assign(seqs, k, owners(text, k), thr, n_rec)
        bits, assign, counts = mf.assign_reads(ks, reads, thr, mf.MODE_SCREENED)
        assert np.array_equal(bits_to_bool(bits, len(seqs)), passes)
        bad = np.nonzero(assign != oassign)[0]
        assert bad.size == 0, [(int(i), int(assign[i]), int(oassign[i])) for i in bad[:10]]
        bad = np.nonzero(counts != ocounts)[0]
        assert bad.size == 0, [(int(j), int(counts[j]), int(ocounts[j])) for j in bad[:10]]
        # identity groups: the group call gives the record call's results
        gbits, gassign, gcounts = mf.assign_groups(ks, reads, thr, mf.MODE_SCREENED)
        assert np.array_equal(gbits, bits) and np.array_equal(gassign, assign) and np.array_equal(gcounts, counts)
    print("test_assign_counters_at_the_lds_limit[%d]: device calls %.2f s" % (n_rec, time.time() - t0))
    assert ks.group_names == ks.record_names
    reads.close(); ks.close()


# ------------------------------------------------------------------ f. reads of many candidates
def vote_key(c):
    j, strand, start = c
    return ((j << 1 | strand) << 32) | (start & 0xFFFFFFFF)


def test_many_candidate_reads_at_scale(mf, ol, scale, scale_ks):
    S = scale
    p = S.parts
    sc = p["seqs"][p["scaffold"]]
    names, seqs = [], []
    for n_seg in (130, 200):                                 # three and four sweeps of a 64-entry map
        for where, long_at in (("first", 0), ("middle", n_seg // 2), ("last", n_seg - 1)):
            s = many_segment_read(sc, K, n_seg, seed=n_seg + long_at, long_at=long_at, span=p["front"])
            names += ["%d_%s" % (n_seg, where), "%d_%s_rc" % (n_seg, where)]
            seqs += [s, revcomp(s)]
    carry, m = bound_carry_read(p, K, seed=9)
    carry_wins, m2 = bound_carry_read(p, K, seed=10, wins=True)
    names += ["carry", "carry_wins"]; seqs += [carry, carry_wins]
    tallies = S.tally(seqs)
    for name, (hits, v, L) in zip(names[:-2], tallies):
        n_seg = int(name.split("_")[0])
        assert len(v) == n_seg and sorted(v.values())[-2:] == [1, 2] and sum(v.values()) == n_seg + 1, name
        assert {c[0] for c in v} == {p["scaffold"]} and {c[1] for c in v} == {int(name.endswith("_rc"))}
    # the carry: the 64 smallest keys of the read end with (m, forward, start -1), whose low word is all ones; the winner lies behind them
    v = tallies[-2][1]
    keys = sorted((vote_key(c), n) for c, n in v.items())
    assert len(keys) == 63 + 1 + 70 and sorted(n for _, n in keys)[-2:] == [1, 2]
    assert keys[63][0] == ((m << 1) << 32 | 0xFFFFFFFF) and (m, 0, -1) in v
    assert keys[64][0] >= ((m << 1) + 1) << 32 and [i for i, (_, n) in enumerate(keys) if n == 2][0] >= 64
    # the same with that candidate as the winner: a second sweep that began AT the first sweep's largest key would count it twice
    v = tallies[-1][1]
    keys = sorted((vote_key(c), n) for c, n in v.items())
    assert len(keys) == 63 + 1 + 70 and keys[63] == ((m2 << 1) << 32 | 0xFFFFFFFF, 2) and sorted(n for _, n in keys)[-2:] == [1, 2]
    assert keys[64][0] >= ((m2 << 1) + 1) << 32
    reads = upload(mf, ol, seqs)
    t0 = time.time()
    rows = check_place(mf, scale_ks, reads, S.o, tallies, 1, mf.MODE_SCREENED)
    print("test_many_candidate_reads_at_scale: device calls %.2f s" % (time.time() - t0))
    reads.close()
    for name, row, (hits, v, L) in zip(names, rows, tallies):
        (j, strand, start), n = v.most_common(1)[0]
        assert row.tolist() == [j, strand, start, start + L, 2, len(v) + 1], name
    assert rows[-2][0] > m and rows[-1].tolist()[:3] == [m2, 0, -1]


# ------------------------------------------------------------------ g. file level
def test_files_placed_at_scale(mf, ol, scale, scale_ks, tmp_path, monkeypatch):
    """several batches add into one counter array through the global branch of the gathered counts: nothing is lost"""
    S = scale
    monkeypatch.setenv("MF_INGEST", "device")
    monkeypatch.setenv("MF_BATCH_READS", "300")
    monkeypatch.setenv("MF_GZDEV_CHUNK_BYTES", "8192")
    monkeypatch.setenv("MF_GZDEV_SLAB_CHUNKS", "5")
    monkeypatch.setenv("MF_GZDEV_TEXT_PIECE", "100000")
    s1 = [s or "A" for s in scale_reads(S.parts, K, 1500, seed=21, uniform=False)]
    s2 = [s or "A" for s in scale_reads(S.parts, K, 1500, seed=22, uniform=False)]
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    out = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    t0 = time.time()
    kept0, total0 = mf.filter_fastq_files(scale_ks, fq1, fq2, out[0], out[1], 1, mf.PAIR_BOTH)
    kept, total, depth, records, unplaced = mf.filter_fastq_files_placed(scale_ks, fq1, fq2, out[2], out[3], 1, mf.PAIR_BOTH)
    assert mf.last_ingest_stats()["path"] == 1 and (kept, total) == (kept0, total0) and total == 1500
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        assert open(a, "rb").read() == open(b, "rb").read()
    wdepth, wrec, wunpl = summed([in_memory(mf, ol, scale_ks, s, 1) for s in (s1, s2)], scale_ks.record_starts)
    print("test_files_placed_at_scale: device calls %.2f s" % (time.time() - t0))
    assert np.array_equal(depth.astype(np.int64), wdepth)
    got = rec_rows(records)
    bad = np.nonzero((got != wrec).any(axis=1))[0]
    assert bad.size == 0, [(int(j), got[j].tolist(), wrec[j].tolist()) for j in bad[:10]]
    assert unplaced.tolist() == wunpl.tolist()
    placed = got[:, 0] + got[:, 1]
    assert int((placed > 0).sum()) > 500 and int(placed[S.parts["scaffold"]:].sum()) > 300          # many records' counters, on both sides of the 256th tile
