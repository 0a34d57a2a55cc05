"""Pair-aware placement (mf_place_pairs / mf.place_pairs) against the plain-Python oracle of tests/pair_oracle.py, which is written from
the "pairs" section of include/mitofilter.h: both sets' placements and scores, the pairs, base depth, every record table, the pile-up,
the consensus and unplaced are compared exactly, with the identities of the verification section over both sets' reads.  The data is
tests/pair_data.py's (what it holds is checked in tests/test_pair_data.py without a device).  There is no tolerance anywhere."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import pair_data as pd
from tests import pair_oracle as pa
from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests.report_data import mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_verify import PILE_REC, PLACE_REC, counts_of, identities, rec_rows, rows_of, score_rows
from tests.util_data import bits_to_bool, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")

PAIR_REC = ("proper", "discordant", "cross", "rescued", "single", "insert_sum")
LO, HI = pd.WINDOW


def first_bad(got, want):
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[0]
    return [(int(i), np.asarray(got)[i].tolist(), np.asarray(want)[i].tolist()) for i in bad[:8]]


def check(p, P, want, n, min_depth, swapped=False):
    """what a paired call gave against what the oracle gave (swapped: the call took the sets the other way round)"""
    one, two = ("2", "1") if swapped else ("1", "2")
    for got_bits, got_place, got_score, m in ((p.bits1, p.place1, p.score1, one), (p.bits2, p.place2, p.score2, two)):
        assert np.array_equal(bits_to_bool(got_bits, n), want["passes" + m])
        assert not first_bad(rows_of(got_place), want["rows" + m]), first_bad(rows_of(got_place), want["rows" + m])
        got = np.stack([got_score["compared"], got_score["mismatches"]], axis=1).astype(np.int64)
        assert not first_bad(got, want["scores" + m]), first_bad(got, want["scores" + m])
    wp = want["pairs"].copy()
    if swapped:          # mate 1 of the call is the oracle's mate 2
        for a, b in ((pa.RESCUED_1, pa.RESCUED_2), (pa.SINGLE_1, pa.SINGLE_2)):
            wp[want["pairs"][:, 0] == a, 0] = b
            wp[want["pairs"][:, 0] == b, 0] = a
    got = np.stack([p.pairs["kind"].astype(np.int64), p.pairs["insert"].astype(np.int64)], axis=1)
    assert not first_bad(got, wp), first_bad(got, wp)
    if not swapped:          # (cross is counted at mate 1's record: the swapped call counts it at the other)
        assert np.array_equal(rec_rows(p.pair_records, PAIR_REC), want["pair_rec"]), (rec_rows(p.pair_records, PAIR_REC), want["pair_rec"])
    assert rec_rows(p.pair_records, PAIR_REC).sum(axis=0).tolist() == want["pair_rec"].sum(axis=0).tolist()
    assert p.pairs_none == want["none"]
    assert int(rec_rows(p.pair_records, PAIR_REC)[:, :5].sum()) + p.pairs_none == n
    assert np.array_equal(p.base_depth.astype(np.int64), np.minimum(want["depth"], po.CLAMP))
    assert np.array_equal(rec_rows(p.place_records, PLACE_REC), want["place_rec"]), (rec_rows(p.place_records, PLACE_REC), want["place_rec"])
    assert np.array_equal(score_rows(p.score_records), want["score_rec"])
    assert p.unplaced.tolist() == want["unplaced"]
    if p.pileup is not None:
        assert not first_bad(counts_of(p.pileup), pio.clamped(want["counts"]))
        cons, rec = P.V.P.call(want["counts"], min_depth)
        assert np.array_equal(p.consensus, cons)
        assert np.array_equal(rec_rows(p.pileup_records, PILE_REC), rec)
    identities(p, 2 * n)
    return p


@pytest.fixture(scope="module")
def main():
    text, recs, sample = pd.pair_bait()
    s1, s2, what = pd.pair_set()
    return text, recs, s1, s2, what


# ------------------------------------------------------------------ 1. every output against the oracle
@pytest.mark.parametrize("k", [21, 31, 41])
def test_every_output_matches_the_oracle(mf, ol, main, k):
    text, recs, s1, s2, what = main
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    assert r1.info.uniform_len == 150 and r2.info.uniform_len == 0
    t1, t2 = o.tally(s1), o.tally(s2)
    n_rescued = {}
    for max_permille in (1000, 30):
        for rescue_permille in (0, 60, 1000):
            want = P.pairs(s1, s2, t1, t2, 1, max_permille, LO, HI, 1, rescue_permille)
            p = check(mf.place_pairs(ks, r1, r2, LO, HI, True, rescue_permille, 2, max_permille), P, want, len(s1), 2)
            n_rescued[(max_permille, rescue_permille)] = int(p.pair_records["rescued"].sum())
            assert int(((p.place1["votes"] == 0) & (p.place1["record"] < mf.PLACE_AMBIGUOUS)).sum()
                       + ((p.place2["votes"] == 0) & (p.place2["record"] < mf.PLACE_AMBIGUOUS)).sum()) == n_rescued[(max_permille, rescue_permille)]
    assert 20 <= n_rescued[(1000, 0)] < n_rescued[(1000, 60)] < n_rescued[(1000, 1000)]
    # the sets the other way round: the ragged set's mates are the settled ones' partners on the other side
    want = P.pairs(s1, s2, t1, t2, 1, 1000, LO, HI, 1, 60)
    check(mf.place_pairs(ks, r2, r1, LO, HI, True, 60, 2, 1000), P, want, len(s1), 2, swapped=True)
    # threshold and mode are the verifying call's; without the pile-up nothing else changes
    want3 = P.pairs(s1, s2, t1, t2, 3, 1000, LO, HI, 1, 60)
    q = check(mf.place_pairs(ks, r1, r2, LO, HI, True, 60, 2, 1000, pileup=False, threshold=3, mode=mf.MODE_EXHAUSTIVE), P, want3, len(s1), 2)
    assert q.pileup is None and q.consensus is None and q.pileup_records is None
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 2. rescue=False is the two single calls added up
def test_without_rescue_every_shared_output_is_the_two_single_calls_added_up(mf, ol, main):
    text, recs, s1, s2, what = main
    ks = mf.KmerSet.from_text(text, 31)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    for max_permille in (1000, 30):
        v1 = mf.verify_reads(ks, r1, 1, mf.MODE_SCREENED, 2, max_permille)
        v2 = mf.verify_reads(ks, r2, 1, mf.MODE_SCREENED, 2, max_permille)
        p = mf.place_pairs(ks, r1, r2, LO, HI, False, 60, 2, max_permille)
        assert np.array_equal(p.bits1, v1.bits) and np.array_equal(p.bits2, v2.bits)
        assert np.array_equal(p.place1, v1.place) and np.array_equal(p.place2, v2.place)
        assert np.array_equal(p.score1, v1.score) and np.array_equal(p.score2, v2.score)
        assert np.array_equal(p.base_depth, v1.base_depth + v2.base_depth)
        for f in ("forward", "reverse", "over_begin", "over_end", "base_sum"):
            assert np.array_equal(p.place_records[f], v1.place_records[f] + v2.place_records[f]), f
        for f in mf.SCORE_RECORD.names:
            assert np.array_equal(p.score_records[f], v1.score_records[f] + v2.score_records[f]), f
        for f in mf.PILEUP.names:
            assert np.array_equal(p.pileup[f], v1.pileup[f] + v2.pileup[f]), f
        for f in ("bases", "matches", "mismatches"):
            assert np.array_equal(p.pileup_records[f], v1.pileup_records[f] + v2.pileup_records[f]), f
        assert p.unplaced.tolist() == (v1.unplaced + v2.unplaced).tolist()
        assert not np.isin(p.pairs["kind"], (mf.PAIR_RESCUED_1, mf.PAIR_RESCUED_2)).any() and int(p.pair_records["rescued"].sum()) == 0
        # the insert of the pairs with both mates settled is pair_inserts' (no pair here is wider than its MAX_INSERT)
        both = np.isin(p.pairs["kind"], (mf.PAIR_PROPER, mf.PAIR_DISCORDANT))
        assert both.sum() >= 100
        assert np.array_equal(p.pairs["insert"][both].astype(np.int64), mf.pair_inserts(v1.place, v2.place)[both])
        assert np.all(p.pairs["insert"][~both] == -1)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 3. the neighbouring record
@pytest.mark.parametrize("k", [21, 41])
def test_a_mate_across_a_record_border_is_not_rescued_into_the_neighbour(mf, ol, k):
    text, recs, sample = pd.pair_bait()
    s1, s2, inside = pd.neighbour_pairs(k)
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    want = P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, 1000, LO, HI, 1, 60)
    p = check(mf.place_pairs(ks, r1, r2, LO, HI, True, 60), P, want, len(s1), 1)
    assert p.pairs["kind"].tolist() == [mf.PAIR_SINGLE_1, mf.PAIR_RESCUED_2, mf.PAIR_RESCUED_2, mf.PAIR_RESCUED_2]
    assert p.place2["record"].tolist()[1:] == [0, 0, 0] and p.score2["compared"].tolist()[1:] == inside[1:]
    assert p.place2["end"].tolist()[1:] == [1050 - n for n in inside[1:]]          # unclipped, beyond the record's 900 positions
    assert int(p.place_records["over_end"][0]) == 3
    assert int(p.base_depth[900:].sum()) == 0 and int(counts_of(p.pileup)[900:].sum()) == 0
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 4. the tandem copy
def test_a_target_inside_the_tandem_copy_ties_and_a_substitution_breaks_the_tie(mf, ol, main):
    text, recs, s1, s2, what = main
    k = 31
    tie = [i for i, n in enumerate(what) if n == "tandem"]
    first = [i for i, n in enumerate(what) if n == "tandem_first_base"]
    idx = tie + first
    a, b = [s1[i] for i in idx], [s2[i] for i in idx]
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, a), upload(mf, ol, b)
    want = P.pairs(a, b, o.tally(a), o.tally(b), 1, 1000, LO, HI, 1, 1000)
    p = check(mf.place_pairs(ks, r1, r2, LO, HI, True, 1000), P, want, len(a), 1)
    n = len(tie)
    # (a target with an N in its middle has no valid window and does not pass; the others pass and are ambiguous)
    assert n >= 20 and np.all(p.pairs["kind"][:n] == mf.PAIR_SINGLE_1) and np.all(p.place2["record"][:n] >= mf.PLACE_AMBIGUOUS)
    assert int((p.place2["record"][:n] == mf.PLACE_AMBIGUOUS).sum()) >= 15
    assert want["why"][:n] == ["tie"] * n
    assert np.all(p.pairs["kind"][n:] == mf.PAIR_RESCUED_2) and np.all(p.place2["start"][n:] == pd.UNIT_AT + pd.UNIT) and np.all(p.score2["mismatches"][n:] == 1)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 5. window widths, the true insert first and last
@pytest.mark.parametrize("width", [1, 64, 65, 4096])
def test_window_widths_with_the_true_insert_first_and_last(mf, ol, width):
    # a record long enough for an insert that a window of 4096 can end at
    rng = random.Random(31)
    rec = "".join(rng.choice("ACGT") for _ in range(4600))
    text = ">long\n%s\n" % rec
    k, ins = 31, 4200
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    # a forward mate 1 and a diverged reverse mate 2 of 90 bases that ends 4200 bases on; the same the other way round
    s1 = [rec[100:250], revcomp(rec[4150:4300])]
    s2 = [revcomp(pd.substituted(rec[4210:4300], 20, 4)), pd.substituted(rec[100:190], 20, 4)]
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    t1, t2 = o.tally(s1), o.tally(s2)
    for lo in (ins, ins - (width - 1)):
        want = P.pairs(s1, s2, t1, t2, 1, 1000, lo, lo + width - 1, 1, 100)
        p = check(mf.place_pairs(ks, r1, r2, lo, lo + width - 1, True, 100), P, want, 2, 1)
        assert p.pairs["kind"].tolist() == [mf.PAIR_RESCUED_2] * 2 and p.pairs["insert"].tolist() == [ins, ins]
        assert p.place2["start"].tolist() == [4210, 100] and p.place2["strand"].tolist() == [1, 0]
    if width < 4096:          # one insert short of the mate on either side: nothing to rescue
        for lo in (ins + 1, ins - width):
            p = mf.place_pairs(ks, r1, r2, lo, lo + width - 1, True, 100)
            assert p.pairs["kind"].tolist() == [mf.PAIR_SINGLE_1] * 2
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 6. a stack of identical pairs
def test_a_stack_of_identical_pairs_is_counted_exactly(mf, ol):
    text, recs, sample = pd.pair_bait()
    k, n = 31, 300
    r1seq = recs[1]
    s1 = [r1seq[350:500]] * n
    s2 = [revcomp(pd.substituted(r1seq[560:650], 20, 4))] * n
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    p = mf.place_pairs(ks, r1, r2, LO, HI, True, 100)
    assert np.all(p.pairs["kind"] == mf.PAIR_RESCUED_2) and np.all(p.pairs["insert"] == 300)
    assert np.all(p.place2["start"] == 560) and np.all(p.place2["votes"] == 0) and np.all(p.score2["compared"] == 90) and np.all(p.score2["mismatches"] == 5)
    start = int(ks.record_starts[1])
    depth = np.zeros(len(p.base_depth), np.int64)
    depth[start + 350:start + 500] += n
    depth[start + 560:start + 650] += n
    assert np.array_equal(p.base_depth.astype(np.int64), depth)
    assert p.pair_records["rescued"].tolist() == [0, n, 0] and p.pair_records["insert_sum"].tolist() == [0, 300 * n, 0]
    assert p.place_records["forward"].tolist() == [0, n, 0] and p.place_records["reverse"].tolist() == [0, n, 0]
    assert p.score_records["accepted"].tolist() == [0, 2 * n, 0] and p.score_records["mismatches"].tolist() == [0, 5 * n, 0]
    assert int(p.score_records["hist"][1][5]) == n and int(p.score_records["hist"][1][0]) == n
    assert counts_of(p.pileup)[start + 560:start + 650].sum(axis=1).tolist() == [n] * 90
    assert p.unplaced.tolist() == [0, 0]
    identities(p, 2 * n)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 7. more targets than the grid has waves
def test_more_rescue_targets_than_the_grid_has_waves(mf, ol):
    text, recs, sample = pd.pair_bait()
    k = 21
    waves = int(re.search(r"(\d+) CUs", mf.device_name(0)).group(1)) * 32          # the launch's waves at most
    n = waves + 777
    rng = random.Random(8)
    r0 = recs[0]
    # forty-base reads: mate 1 in r0's own bases, mate 2 diverged (three substitutions) 100 bases on; a 16-wide window
    spots = [(rng.randint(0, 150), rng.randint(96, 104)) for _ in range(64)]
    pool = [(r0[a:a + 40], revcomp(pd.substituted(r0[a + ins - 40:a + ins], 15, 5))) for a, ins in spots]
    pick = [rng.randrange(64) for _ in range(n)]
    s1, s2 = [pool[i][0] for i in pick], [pool[i][1] for i in pick]
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    w = P.pairs([a for a, _ in pool], [b for _, b in pool], o.tally([a for a, _ in pool]), o.tally([b for _, b in pool]), 1, 1000, 92, 107, 1, 100)
    assert np.all(w["pairs"][:, 0] == pa.RESCUED_2) and w["pairs"][:, 1].tolist() == [ins for _, ins in spots]
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    p = mf.place_pairs(ks, r1, r2, 92, 107, True, 100)
    assert np.array_equal(rows_of(p.place2), w["rows2"][pick]) and np.array_equal(p.pairs["insert"], w["pairs"][pick, 1])
    assert np.all(p.pairs["kind"] == mf.PAIR_RESCUED_2) and int(p.pair_records["rescued"][0]) == n
    depth = np.zeros(len(p.base_depth), np.int64)
    for i in pick:
        for row in (w["rows1"][i], w["rows2"][i]):
            depth[row[2]:row[3]] += 1
    assert np.array_equal(p.base_depth.astype(np.int64), depth)
    assert p.unplaced.tolist() == [0, 0]
    identities(p, 2 * n)
    r1.close(); r2.close(); ks.close()


# ------------------------------------------------------------------ 8. sequences of calls on one handle
def test_a_paired_call_between_single_calls_on_the_same_handles(mf, ol, main):
    text, recs, s1, s2, what = main
    k = 31
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    other = s2[::-1][:200]
    r1, r2, r3 = upload(mf, ol, s1), upload(mf, ol, s2), upload(mf, ol, other)
    t1, t2 = o.tally(s1), o.tally(s2)
    want = P.pairs(s1, s2, t1, t2, 1, 1000, LO, HI, 1, 60)
    before = mf.verify_reads(ks, r3, 1, mf.MODE_SCREENED, 2, 1000)
    check(mf.place_pairs(ks, r1, r2, LO, HI, True, 60, 2), P, want, len(s1), 2)
    after1 = mf.verify_reads(ks, r1, 1, mf.MODE_SCREENED, 2, 1000)
    after3 = mf.verify_reads(ks, r3, 1, mf.MODE_SCREENED, 2, 1000)
    v1 = want["single"][0]
    assert np.array_equal(rows_of(after1.place), v1["rows"]) and np.array_equal(after1.base_depth.astype(np.int64), v1["depth"])
    assert after1.unplaced.tolist() == v1["unplaced"]
    for f in ("place", "score", "base_depth", "place_records", "pileup", "consensus", "score_records", "unplaced"):
        assert np.array_equal(getattr(before, f), getattr(after3, f)), f
    # and once more: a warm paired call gives what the first gave
    check(mf.place_pairs(ks, r1, r2, LO, HI, True, 60, 2), P, want, len(s1), 2)
    r1.close(); r2.close(); r3.close(); ks.close()


# ------------------------------------------------------------------ 9. the refusals that need handles; an empty pair of sets
def test_refusals_that_need_handles(mf, ol, main):
    text, recs, s1, s2, what = main
    ks = mf.KmerSet.from_text(text, 31)
    r1, r2, r3 = upload(mf, ol, s1[:10]), upload(mf, ol, s2[:10]), upload(mf, ol, s2[:9])
    with pytest.raises(ValueError, match="length"):
        mf.place_pairs(ks, r1, r3, LO, HI)
    L = mf.load()

    def raw(ks_h, a, b):
        return L.mf_place_pairs(ks_h, a, b, 1, 0, 1, 1000, LO, HI, 1, 100, *([None] * 17))

    assert raw(ks._h, r1._h, r3._h) == -1 and b"mate" in L.mf_last_error()
    assert raw(ks._h, r1._h, r1._h) == -1 and b"one read set" in L.mf_last_error()
    assert raw(ks._h, r1._h, None) == -1 and b"NULL" in L.mf_last_error()
    from tests.util_data import make_protein_bait
    pks = mf.KmerSet.protein_from_text(make_protein_bait()[0], 7, 5)
    assert raw(pks._h, r1._h, r2._h) == -1 and b"nucleotide" in L.mf_last_error()
    pks.close()
    # every output is optional
    assert raw(ks._h, r1._h, r2._h) == 0
    r1.close(); r2.close(); r3.close(); ks.close()


# ------------------------------------------------------------------ 10. the entry points: the CLI's files, bim.consensus_bait(pairs=True)
def test_the_cli_and_bim_give_what_the_oracle_gives(mf, ol, main, tmp_path):
    from mitoflex_amd.bim import bim
    text, recs, s1, s2, what = main
    k = 31
    o = po.PlaceOracle(text, k)
    P = pa.PairOracle(o)
    t1, t2 = o.tally(s1), o.tally(s2)
    bait, fq1, fq2 = str(tmp_path / "bait.fa"), str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(bait, "w").write(text)
    write_fastq(fq1, s1, "p")
    write_fastq(fq2, s2, "p")
    names, starts = ["r0", "r1", "r2"], o.starts
    want = P.pairs(s1, s2, t1, t2, 1, 1000, LO, HI, 1, 100)
    cons, _ = P.V.P.call(want["counts"], 2)
    files = {n: str(tmp_path / n) for n in ("pairs.tsv", "place.tsv", "depth.tsv", "cons.fa", "score.tsv")}
    r = subprocess.run([CLI, "pairs", "--bait", bait, "-k", str(k), "--fq1", fq1, "--fq2", fq2, "--min-insert", str(LO), "--max-insert", str(HI), "--min-depth", "2",
                        "--pair-report", files["pairs.tsv"], "--place-report", files["place.tsv"], "--base-depth", files["depth.tsv"], "--consensus", files["cons.fa"],
                        "--score-report", files["score.tsv"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == int(want["pair_rec"][:, 3].sum()) > 100
    rows = [line.split("\t") for line in open(files["pairs.tsv"]).read().splitlines()]
    assert rows[0] == ["record", "name", "length", "proper", "discordant", "cross", "rescued", "single", "mean_insert"]
    for j in range(3):
        pr = want["pair_rec"][j]
        n_ins = int(pr[0] + pr[3])
        assert rows[1 + j] == [str(j), names[j], str(o.lens[j])] + [str(int(x)) for x in pr[:5]] + ["%.3f" % (int(pr[5]) / n_ins if n_ins else 0.0)]
    assert rows[4] == ["-", "*none*", str(want["none"])]
    assert open(files["cons.fa"]).read() == mf.consensus_fasta(names, starts, cons)
    depth = [int(line.split("\t")[2]) for line in open(files["depth.tsv"]).read().splitlines()]
    assert depth == want["depth"].tolist()
    placed = [line.split("\t") for line in open(files["place.tsv"]).read().splitlines()]
    assert [[int(x) for x in row[3:8]] for row in placed[1:4]] == want["place_rec"][:, :5].astype(np.int64).tolist() and placed[4][2] == str(want["unplaced"][0])
    scored = [line.split("\t") for line in open(files["score.tsv"]).read().splitlines()]
    assert [[int(x) for x in row[3:7]] for row in scored[1:4]] == want["score_rec"][:, :4].astype(np.int64).tolist()
    off = subprocess.run([CLI, "pairs", "--bait", bait, "-k", str(k), "--fq1", fq1, "--fq2", fq2, "--min-insert", str(LO), "--max-insert", str(HI), "--no-rescue"],
                         capture_output=True, text=True, timeout=120)
    assert off.returncode == 0 and int(off.stdout) == 0
    # bim: with the window given, and with the window it estimates from the pairs the vote places
    out = str(tmp_path / "polished.fa")
    bim.consensus_bait(bait, fq1, fq2, out, kmer=k, min_depth=2, pairs=True, min_insert=LO, max_insert=HI)
    assert open(out).read() == mf.consensus_fasta(names, starts, cons)
    first = P.pairs(s1, s2, t1, t2, 1, 1000, 1, pa.RESCUE_MAX, 0, 100)
    lo, hi = bim.rescue_window(first["pairs"][:, 1])
    assert 1 <= lo <= LO + 20 and HI - 20 <= hi <= 400
    auto = P.pairs(s1, s2, t1, t2, 1, 1000, lo, hi, 1, 100)
    bim.consensus_bait(bait, fq1, fq2, out, kmer=k, min_depth=2, pairs=True)
    assert open(out).read() == mf.consensus_fasta(names, starts, P.V.P.call(auto["counts"], 2)[0])
    # what the feature buys: the diverged stretch is called from the rescued mates; without pairs it keeps the old bait's letters
    polished = "".join(open(out).read().split(">r1")[0].splitlines()[1:])
    bim.consensus_bait(bait, fq1, fq2, out, kmer=k, min_depth=2)
    plain = "".join(open(out).read().split(">r1")[0].splitlines()[1:])
    a, b = pd.D[0] + 40, pd.D[0] + 140
    assert polished[a:b].isupper() and plain[a:b].islower() and plain[a:b].upper() == recs[0][a:b]
    sample0 = pd.pair_bait()[2][0][pd.FLANK:pd.FLANK + 900]
    assert polished[a:b] == sample0[a:b] != recs[0][a:b]
    for bad in (dict(band=4), dict(band=4, gapped=True), dict(band=0, extend=8)):
        with pytest.raises(ValueError):
            bim.consensus_bait(bait, fq1, fq2, out, kmer=k, pairs=True, **bad)
    with pytest.raises(ValueError):
        bim.consensus_bait(bait, fq1, None, out, kmer=k, pairs=True)
