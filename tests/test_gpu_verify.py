"""Verification of the placed reads (mf_verify, mf_filter_fastq_files_verified, `fastfilter bait --score-report / --max-mismatch`,
bim.consensus_bait(max_permille=..)) against the plain-Python oracle of tests/verify_oracle.py, which is written from the semantics in
include/mitofilter.h: per-read scores, the cut, and every placement and pile-up output of the accepted reads are compared exactly.
There is no tolerance anywhere."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests import verify_oracle as vo
from tests.report_data import fasta, mf, mutate, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_bim import _genome
from tests.test_gpu_place import place_bait, place_reads, special_reads
from tests.util_data import bits_to_bool, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
PLACE_FIELDS = ("record", "strand", "start", "end", "votes", "windows")
PLACE_REC = ("forward", "reverse", "over_begin", "over_end", "covered", "base_sum")
PILE_REC = ("bases", "matches", "mismatches", "called", "ambiguous", "variants")
LETTERS = ("a", "c", "g", "t")


def rows_of(place):
    return np.stack([place[f].astype(np.int64) for f in PLACE_FIELDS], axis=1)


def rec_rows(records, fields):
    return np.stack([records[f] for f in fields], axis=1).astype(np.uint64)


def score_rows(records):
    return np.concatenate([rec_rows(records, ("accepted", "rejected", "compared", "mismatches")), records["hist"].astype(np.uint64)], axis=1)


def counts_of(pileup):
    return np.stack([pileup[f].astype(np.int64) for f in LETTERS], axis=1)


def one_hot(text):
    out = np.zeros((len(text), 4), np.int64)
    out[np.arange(len(text)), ["ACGT".index(c) for c in text]] = 1
    return out


def drawn(s, n, seed, lo=100, hi=150):
    """n reads of lo .. hi bases from both strands of s"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        L = rng.randint(lo, hi)
        a = rng.randrange(0, len(s) - L + 1)
        out.append(s[a:a + L] if rng.random() < 0.5 else revcomp(s[a:a + L]))
    return out


def substituted(s, at):
    """s with another letter at every offset of `at`"""
    t = list(s)
    for i in at:
        t[i] = "CGTA"["ACGT".index(t[i])]
    return "".join(t)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def identities(v, n_reads):
    """the four identities of the header's verification section, on any result that holds a pile-up"""
    s, p = v.score_records, v.place_records
    assert np.array_equal(s["accepted"], p["forward"] + p["reverse"])
    assert np.array_equal(s["hist"].sum(axis=1), s["accepted"] + s["rejected"])
    assert int((p["forward"] + p["reverse"] + s["rejected"]).sum()) + int(v.unplaced[0]) + int(v.unplaced[1]) == n_reads
    if v.pileup_records is not None:
        assert np.array_equal(s["compared"], v.pileup_records["matches"] + v.pileup_records["mismatches"])
        assert np.array_equal(s["mismatches"], v.pileup_records["mismatches"])


def check(mf, ks, reads, V, seqs, want, thr, mode, min_depth, max_permille):
    """one mf_verify call against what the oracle gave for (thr, max_permille)"""
    return check_result(mf.verify_reads(ks, reads, thr, mode, min_depth, max_permille), V, seqs, want, min_depth)


def check_result(v, V, seqs, want, min_depth):
    """what a verifying call gave (with a keep mode or without) against what the oracle gave for its threshold and cut"""
    n = len(seqs)
    assert np.array_equal(bits_to_bool(v.bits, n), want["passes"])
    got = rows_of(v.place)
    bad = np.nonzero((got != want["rows"]).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["rows"][i].tolist()) for i in bad[:10]]
    got = np.stack([v.score["compared"], v.score["mismatches"]], axis=1).astype(np.int64)
    bad = np.nonzero((got != want["scores"]).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["scores"][i].tolist(), want["rows"][i].tolist()) for i in bad[:10]]
    bad = np.nonzero(v.base_depth.astype(np.int64) != np.minimum(want["depth"], po.CLAMP))[0]
    assert bad.size == 0, [(int(i), int(v.base_depth[i]), int(want["depth"][i])) for i in bad[:10]]
    assert np.array_equal(rec_rows(v.place_records, PLACE_REC), want["place_rec"]), (rec_rows(v.place_records, PLACE_REC), want["place_rec"])
    assert np.array_equal(score_rows(v.score_records), want["score_rec"]), (score_rows(v.score_records), want["score_rec"])
    got = counts_of(v.pileup)
    bad = np.nonzero((got != pio.clamped(want["counts"])).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), want["counts"][i].tolist()) for i in bad[:10]]
    cons, rec = V.P.call(want["counts"], min_depth)
    assert np.array_equal(v.consensus, cons)
    assert np.array_equal(rec_rows(v.pileup_records, PILE_REC), rec)
    assert v.unplaced.tolist() == want["unplaced"]
    identities(v, n)
    return v


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("k", [21, 31, 32, 41])
def test_verify_matches_oracle(mf, ol, k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    V = vo.VerifyOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    for uniform in (False, True):
        _, seqs = place_reads(text, parts, k, 1200, seed=1300 + k, uniform=uniform)
        seqs = seqs + drawn(mutate(parts["g"], 0.01, 77), 200, seed=79, lo=150 if uniform else 100)
        tallies = o.tally(seqs)
        reads = upload(mf, ol, seqs)
        cut = {}
        for thr in (1, 3):
            for max_permille in (1000, 20, 0):
                want = V.verify(seqs, tallies, thr, max_permille)
                for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                    check(mf, ks, reads, V, seqs, want, thr, mode, 2, max_permille)
                cut[(thr, max_permille)] = int(want["score_rec"][:, 1].sum())
        # the cuts cut: nothing at 1000, something at 20, more at 0
        assert cut[(1, 1000)] == 0 and 0 < cut[(1, 20)] < cut[(1, 0)]
        reads.close()
    ks.close()


# ------------------------------------------------------------------ 2. max_permille = 1000 is placement and pile-up as they are
def test_at_1000_every_shared_output_is_placement_s_and_the_pile_up_s(mf, ol):
    text, parts = place_bait()
    ks = mf.KmerSet.from_text(text, 31)
    _, seqs = place_reads(text, parts, 31, 1200, seed=1401, uniform=False)
    seqs = seqs + drawn(mutate(parts["g"], 0.02, 5), 200, seed=6)
    reads = upload(mf, ol, seqs)
    for thr in (1, 3):
        bits, place, base_depth, precs, unpl = mf.place_reads(ks, reads, thr)
        pbits, pileup, consensus, prec2, unpl2 = mf.pileup_reads(ks, reads, thr, mf.MODE_SCREENED, 2)
        v = mf.verify_reads(ks, reads, thr, mf.MODE_SCREENED, 2, 1000)
        w = mf.verify_reads(ks, reads, thr, mf.MODE_SCREENED, 2, 1000, pileup=False)
        for r in (v, w):
            assert np.array_equal(r.bits, bits) and np.array_equal(r.place, place) and np.array_equal(r.base_depth, base_depth)
            assert np.array_equal(r.place_records, precs) and r.unplaced.tolist() == unpl.tolist() == unpl2.tolist()
            assert int(r.score_records["rejected"].sum()) == 0
            identities(r, len(seqs))
        assert np.array_equal(v.pileup, pileup) and np.array_equal(v.consensus, consensus) and np.array_equal(v.pileup_records, prec2)
        assert w.pileup is None and w.consensus is None and w.pileup_records is None
        assert np.array_equal(w.score, v.score) and np.array_equal(w.score_records, v.score_records)
        placed = place["record"] < mf.PLACE_AMBIGUOUS
        assert np.all(v.score["compared"][placed] >= 31) and np.all(v.score["compared"][~placed] == 0) and np.all(v.score["mismatches"][~placed] == 0)
        assert int(v.score_records["mismatches"].sum()) > 0
    reads.close(); ks.close()


# ------------------------------------------------------------------ 3. special reads, one by one, without the oracle
@pytest.mark.parametrize("k", [21, 32])
def test_special_reads_one_by_one(mf, ol, k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    V = vo.VerifyOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    R = {n: j for j, n in enumerate(ks.record_names)}
    g = parts["g"]
    names, special = special_reads(parts, k)
    got = {}
    for name, seq in zip(names, special):
        reads = upload(mf, ol, [seq])
        want = V.verify([seq], o.tally([seq]), 1, 1000)
        got[name] = check(mf, ks, reads, V, [seq], want, 1, mf.MODE_SCREENED, 1, 1000)
        if name == "insertion":
            want50 = V.verify([seq], o.tally([seq]), 1, 50)
            cut = check(mf, ks, reads, V, [seq], want50, 1, mf.MODE_SCREENED, 1, 50)
        reads.close()
    score = lambda name: (int(got[name].score["compared"][0]), int(got[name].score["mismatches"][0]))
    assert score("over_begin") == (100, 0)
    assert score("over_end") == (90, 0)
    assert score("with_n") == (149, 0)
    seq = special[names.index("insertion")]
    mism = sum(a != b for a, b in zip(seq, g[1400:1556]))
    assert mism > 20 and score("insertion") == (156, mism)
    # rejected at 50 permille: it keeps its placement and its score and counts nowhere but in rejected and its bin
    assert rows_of(cut.place)[0].tolist()[:4] == [R["mito"], 0, 1400, 1556]
    assert (int(cut.score["compared"][0]), int(cut.score["mismatches"][0])) == (156, mism)
    assert int(cut.base_depth.sum()) == 0 and int(counts_of(cut.pileup).sum()) == 0
    assert int(rec_rows(cut.place_records, PLACE_REC).sum()) == 0 and int(rec_rows(cut.pileup_records, PILE_REC)[:, :3].sum()) == 0
    srec = score_rows(cut.score_records)
    assert int(srec[R["mito"], 1]) == 1 and int(srec[R["mito"], 4 + min(mism, 31)]) == 1 and int(srec.sum()) == 2
    assert cut.unplaced.tolist() == [0, 0]
    for name in ("scattered_first", "scattered_last"):
        seq = special[names.index(name)]
        row = rows_of(got[name].place)[0]
        assert len(seq) > 1400 and row[0] == R["mito"] and row[1] == (name == "scattered_last")
        assert score(name) == V.score(seq, row) and score(name)[0] > 64 * 4          # (check() compared it too; more than four rounds of lanes)
    for name in ("tie", "no_anchor"):
        assert score(name) == (0, 0) and got[name].unplaced.tolist() == [1, 0]
    ks.close()


# ------------------------------------------------------------------ 4. the alignment sweep on the device
def sweep_reads(g, starts_of):
    """512 reads of 60 bases, one for every (b0 mod 16, start mod 16, strand), each behind a filler read whose length brings the next
    read's first base to the wanted place in its word.  starts_of(sm, idx) -> the read's start.  -> (seqs, index of the test reads,
    their (b0 mod 16, start, strand))"""
    rng = random.Random(99)
    seqs, at, meta, b0 = [], [], [], 0
    for idx, (bm, sm, strand) in enumerate((bm, sm, strand) for bm in range(16) for sm in range(16) for strand in (0, 1)):
        fill = 21 + ((bm - b0 - 21) % 16)                      # a filler of 21 .. 36 random bases: it does not pass
        seqs.append("".join(rng.choices("ACGT", k=fill)))
        b0 += fill
        assert b0 % 16 == bm
        start = starts_of(sm, idx)
        lo, hi = max(start, 0), min(start + 60, len(g))
        fwd = "".join(rng.choices("ACGT", k=lo - start)) + g[lo:hi] + "".join(rng.choices("ACGT", k=start + 60 - hi))
        seqs.append(substituted(revcomp(fwd) if strand else fwd, (0, 30, 59)))
        at.append(len(seqs) - 1)
        meta.append((bm, start, strand))
        b0 += 60
    return seqs, at, meta


def test_alignment_sweep_on_the_device(mf, ol):
    g = _genome(3000, 41)
    ks = mf.KmerSet.from_text(">g\n" + g + "\n", 21)
    # inside the record: every residue of the read's place in its word, of the start and both strands
    seqs, at, meta = sweep_reads(g, lambda sm, idx: 48 + 16 * (idx % 170) + sm)
    assert len({(bm, s % 16, strand) for bm, s, strand in meta}) == 512
    reads = upload(mf, ol, seqs)
    v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 1, 1000)
    reads.close()
    rows = rows_of(v.place)[at]
    assert [(r[0], r[1], r[2]) for r in rows.tolist()] == [(0, strand, s) for _, s, strand in meta]
    assert v.score["compared"][at].tolist() == [60] * 512 and v.score["mismatches"][at].tolist() == [3] * 512
    assert int(v.score_records["hist"][0][3]) == 512 and int(v.score_records["compared"][0]) == 512 * 60
    # hanging over the begin (even b0 mod 16) or the end (odd) of the record by 1 .. 16: one planted mismatch hangs over with it
    over = lambda sm, idx: -(1 + sm) if (idx // 32) % 2 == 0 else 3000 - 60 + 1 + sm
    seqs, at, meta = sweep_reads(g, over)
    assert len({(bm, s % 16, strand, s < 0) for bm, s, strand in meta}) == 512
    reads = upload(mf, ol, seqs)
    v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 1, 1000)
    reads.close()
    rows = rows_of(v.place)[at]
    assert [(r[0], r[1], r[2]) for r in rows.tolist()] == [(0, strand, s) for _, s, strand in meta]
    hang = [(-s if s < 0 else s + 60 - 3000) for _, s, _ in meta]
    for begin in (True, False):
        assert sorted({h for h, (_, s, _) in zip(hang, meta) if (s < 0) == begin}) == list(range(1, 17))
    assert v.score["compared"][at].tolist() == [60 - h for h in hang] and v.score["mismatches"][at].tolist() == [2] * 512
    identities(v, len(seqs))
    ks.close()


# ------------------------------------------------------------------ 5. stacked reads
def test_stacked_reads(mf, ol):
    """thousands of copies of an accepted and of a rejected read on one start: the counts are exact, and the rejected copies appear
    nowhere but in rejected and the histogram"""
    text, parts = place_bait()
    ks = mf.KmerSet.from_text(text, 31)
    g = parts["g"]
    good = g[300:450]
    bad = substituted(good, range(5, 55, 5))                    # 10 of 150: 66.7 permille; the clean run behind offset 50 places it
    seqs = [good, bad] * 3000
    reads = upload(mf, ol, seqs)
    v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 3, 30)
    reads.close()
    j = ks.record_names.index("mito")
    at = int(ks.record_starts[j])
    assert rows_of(v.place)[:, :4].tolist() == [[j, 0, 300, 450]] * 6000
    assert v.score["compared"].tolist() == [150] * 6000 and v.score["mismatches"].tolist() == [0, 10] * 3000
    want_depth = np.zeros(len(v.base_depth), np.int64)
    want_depth[at + 300:at + 450] = 3000
    assert np.array_equal(v.base_depth.astype(np.int64), want_depth)
    want_counts = np.zeros((len(v.base_depth), 4), np.int64)
    want_counts[at + 300:at + 450] = 3000 * one_hot(good)
    assert np.array_equal(counts_of(v.pileup), want_counts)
    hist = [0] * 32
    hist[0], hist[10] = 3000, 3000
    want = np.zeros((len(ks.record_names), 36), np.uint64)
    want[j] = [3000, 3000, 3000 * 150, 0] + hist
    assert np.array_equal(score_rows(v.score_records), want)
    assert rec_rows(v.place_records, PLACE_REC)[j].tolist() == [3000, 0, 0, 0, 150, 3000 * 150]
    assert rec_rows(v.pileup_records, PILE_REC)[j].tolist() == [3000 * 150, 3000 * 150, 0, 150, 0, 0]
    assert v.unplaced.tolist() == [0, 0]
    identities(v, 6000)
    ks.close()


# ------------------------------------------------------------------ 6. the NUMT case, independent of the oracle
NUMT_LO, NUMT_HI = 1000, 1600


def numt_data():
    """a 3 000-base bait, ~400 error-free reads of it, ~300 reads of a copy of positions 1000 .. 1599 with every 25th base substituted"""
    g = _genome(3000, 11)
    at = [i for i in range(NUMT_HI - NUMT_LO) if i % 25 == 24]
    copy = substituted(g[NUMT_LO:NUMT_HI], at)
    return g, [NUMT_LO + i for i in at], drawn(g, 400, seed=13), drawn(copy, 300, seed=14)


def test_numt_reads_are_cut_and_the_consensus_is_the_bait_s(mf, ol):
    """A read of L bases of the copy holds floor(L / 25) or one more substitutions, at least 4 / 124 = 32.3 permille, and every clean
    run is 24 >= k, so every copy read is placed and, at 30 permille, rejected.  Run on the oracle alone on the CPU first
    (tests/verify_oracle.py on numt_data()): it satisfies the same properties -- 22 variants at 1000 permille, all at substituted
    positions, 0 at 30 permille, and 2 972 positions called both times."""
    g, subst, clean, copies = numt_data()
    seqs = clean + copies
    ks = mf.KmerSet.from_text(">g\n" + g + "\n", 21)
    reads = upload(mf, ol, seqs)
    all_in = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 3, 1000)
    cut = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 3, 30)
    reads.close()
    letters, starts = ks.bait_letters, ks.record_starts
    ks.close()
    assert np.all(all_in.place["record"] == 0) and np.array_equal(all_in.place, cut.place) and np.array_equal(all_in.score, cut.score)
    v = mf.pileup_variants(starts, letters, all_in.pileup, all_in.consensus)
    assert len(v) == int(all_in.pileup_records["variants"][0]) > 15
    assert all(int(r["pos"]) in subst for r in v)
    # exactly the copy reads are rejected
    s = cut.score
    accepted = s["mismatches"].astype(np.int64) * 1000 <= 30 * s["compared"].astype(np.int64)
    assert accepted.tolist() == [True] * len(clean) + [False] * len(copies)
    assert np.all(s["mismatches"][:len(clean)] == 0) and np.all(s["mismatches"][len(clean):] >= 4)
    assert (int(cut.score_records["accepted"][0]), int(cut.score_records["rejected"][0])) == (len(clean), len(copies))
    assert int(cut.score_records["mismatches"][0]) == 0 == int(cut.pileup_records["mismatches"][0])
    assert len(mf.pileup_variants(starts, letters, cut.pileup, cut.consensus)) == 0 == int(cut.pileup_records["variants"][0])
    cons = bytes(cut.consensus).decode()
    called = [p for p, ch in enumerate(cons) if ch in "ACGT"]
    assert all(cons[p] == g[p] for p in called) and "N" not in cons
    assert len(called) == int(cut.pileup_records["called"][0]) == int(all_in.pileup_records["called"][0]) > 2900
    identities(cut, len(seqs)); identities(all_in, len(seqs))


# ------------------------------------------------------------------ 7. file level
@pytest.fixture(scope="module")
def nuc_files():
    text, parts = place_bait()
    far = mutate(parts["g"], 0.03, 5)                           # reads of a copy that differs at 3 %: most of them fall to a 20 permille cut
    _, s1 = place_reads(text, parts, 31, 800, seed=61, uniform=False)
    _, s2 = place_reads(text, parts, 31, 800, seed=62, uniform=False)
    s1, s2 = [s or "A" for s in s1] + drawn(far, 150, seed=63), [s or "A" for s in s2] + drawn(far, 150, seed=64)
    return text, s1, s2[:len(s1)]


def in_memory(mf, ol, ks, seqs, thr, max_permille):
    reads = upload(mf, ol, seqs)
    v = mf.verify_reads(ks, reads, thr, mf.MODE_SCREENED, 1, max_permille)
    reads.close()
    return v


def summed(P, starts, parts, min_depth):
    """what the file-level call gives for the mates verified in memory: every count adds; covered and the calls come from the sums"""
    counts = sum(counts_of(p.pileup) for p in parts)
    depth = sum(p.base_depth.astype(np.int64) for p in parts)
    cons, pile_rec = P.call(counts, min_depth)
    place_rec = sum(rec_rows(p.place_records, PLACE_REC) for p in parts)
    place_rec[:, 4] = [int((depth[int(starts[j]):int(starts[j + 1])] > 0).sum()) for j in range(len(starts) - 1)]
    assert np.array_equal(pile_rec[:, :3], sum(rec_rows(p.pileup_records, PILE_REC) for p in parts)[:, :3])
    return {"counts": counts, "depth": depth, "consensus": cons, "pile_rec": pile_rec, "place_rec": place_rec,
            "score_rec": sum(score_rows(p.score_records) for p in parts), "unplaced": sum(p.unplaced for p in parts).tolist()}


def files_equal(want, base_depth, place_records, pileup, consensus, pileup_records, score_records, unplaced):
    assert np.array_equal(np.asarray(base_depth, np.int64), want["depth"])
    assert np.array_equal(np.asarray(place_records, np.uint64), want["place_rec"])
    assert np.array_equal(np.asarray(pileup, np.int64), want["counts"])
    assert bytes(consensus) == bytes(want["consensus"])
    assert np.array_equal(np.asarray(pileup_records, np.uint64), want["pile_rec"])
    assert np.array_equal(np.asarray(score_records, np.uint64), want["score_rec"])
    assert [int(x) for x in unplaced] == want["unplaced"]


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_verified_equal_the_mates_in_memory(mf, ol, nuc_files, tmp_path, monkeypatch, ingest):
    text, s1, s2 = nuc_files
    gz = ingest == "device-gz"
    monkeypatch.setenv("MF_INGEST", "device" if gz else "host")
    monkeypatch.setenv("MF_BATCH_READS", "300")
    monkeypatch.setenv("MF_GZDEV_CHUNK_BYTES", "8192")
    monkeypatch.setenv("MF_GZDEV_SLAB_CHUNKS", "5")
    monkeypatch.setenv("MF_GZDEV_TEXT_PIECE", "100000")
    ext = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
    write_fastq(fq1, s1, "a", gz=gz)
    write_fastq(fq2, s2, "b", gz=gz)
    ks = mf.KmerSet.from_text(text, 31)
    P = pio.PileupOracle(po.PlaceOracle(text, 31))
    out = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    for thr, min_depth, max_permille in ((1, 1, 20), (3, 2, 1000)):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, out[0], out[1], thr, mf.PAIR_BOTH)
        v = mf.filter_fastq_files_verified(ks, fq1, fq2, out[2], out[3], thr, mf.PAIR_BOTH, min_depth=min_depth, max_permille=max_permille)
        assert mf.last_ingest_stats()["path"] == (1 if gz else 0)
        assert (v.kept, v.total) == (kept0, total0) and v.bits is None and v.place is None and v.score is None
        assert md5(out[2]) == md5(out[0]) and md5(out[3]) == md5(out[1])
        want = summed(P, ks.record_starts, [in_memory(mf, ol, ks, s, thr, max_permille) for s in (s1, s2)], min_depth)
        files_equal(want, v.base_depth, rec_rows(v.place_records, PLACE_REC), counts_of(v.pileup), v.consensus, rec_rows(v.pileup_records, PILE_REC),
                    score_rows(v.score_records), v.unplaced)
        assert (int(want["score_rec"][:, 1].sum()) > 0) == (max_permille == 20)          # the cut cuts
        identities(v, 2 * len(s1))
        w = mf.filter_fastq_files_verified(ks, fq1, fq2, out[2], out[3], thr, mf.PAIR_BOTH, min_depth=min_depth, max_permille=max_permille, pileup=False)
        assert w.pileup is None and np.array_equal(w.base_depth, v.base_depth) and np.array_equal(w.score_records, v.score_records)
        assert np.array_equal(w.place_records, v.place_records) and w.unplaced.tolist() == v.unplaced.tolist()
    ks.close()


def test_files_verified_two_devices(mf, ol, nuc_files, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), on both ingest paths, in a child process"""
    text, s1, s2 = nuc_files
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    ks = mf.KmerSet.from_text(text, 31)
    P = pio.PileupOracle(po.PlaceOracle(text, 31))
    want = summed(P, ks.record_starts, [in_memory(mf, ol, ks, s, 1, 20) for s in (s1, s2)], 2)
    ks.close()
    for gz, ingest in ((True, "device"), (False, "host")):
        ext = ".fq.gz" if gz else ".fq"
        fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
        write_fastq(fq1, s1, "a", gz=gz)
        write_fastq(fq2, s2, "b", gz=gz)
        script = (
            "import json, sys\n"
            "import numpy as np\n"
            "from mitoflex_amd import mitofilter as mf\n"
            "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
            "a = mf.filter_fastq_files(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/o1.fq', sys.argv[4] + '/o2.fq', 1, 1, devices=[0, 1])\n"
            "v = mf.filter_fastq_files_verified(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 1, devices=[0, 1],"
            " min_depth=2, max_permille=20)\n"
            "flat = lambda rec: [[int(x) for f in rec.dtype.names for x in np.atleast_1d(r[f])] for r in rec]\n"
            "print(json.dumps({'a': list(a), 'kept': v.kept, 'total': v.total, 'depth': [int(x) for x in v.base_depth], 'place': flat(v.place_records),"
            " 'pileup': flat(v.pileup), 'consensus': bytes(v.consensus).decode(), 'pile': flat(v.pileup_records), 'score': flat(v.score_records),"
            " 'unplaced': [int(x) for x in v.unplaced], 'path': mf.last_ingest_stats()['path'], 'n_dev': mf.last_ingest_stats()['n_devices']}))\n")
        env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_GZDEV_CHUNK_BYTES="8192",
                   MF_GZDEV_SLAB_CHUNKS="5", MF_GZDEV_TEXT_PIECE="100000", MF_BATCH_READS="400", PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert r["path"] == (1 if ingest == "device" else 0) and r["n_dev"] == 2
        assert r["a"] == [r["kept"], r["total"]]
        for m in ("1", "2"):
            assert md5(str(tmp_path / ("g%s.fq" % m))) == md5(str(tmp_path / ("o%s.fq" % m)))
        files_equal(want, r["depth"], r["place"], r["pileup"], r["consensus"].encode(), r["pile"], r["score"], r["unplaced"])


# ------------------------------------------------------------------ 8. CLI
def score_text(names, starts, recs):
    head = "record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tpermille" + "".join("\tmm%d" % b for b in range(31)) + "\tmm31+\n"
    rows = []
    for j, d in enumerate(recs):
        c, m = int(d["compared"]), int(d["mismatches"])
        rows.append("%d\t%s\t%d\t%d\t%d\t%d\t%d\t%.3f" % (j, names[j], starts[j + 1] - starts[j], int(d["accepted"]), int(d["rejected"]), c, m,
                                                         1000.0 * float(m) / float(c) if c else 0.0) + "".join("\t%d" % int(x) for x in d["hist"]) + "\n")
    return head + "".join(rows)


def test_cli_score_report_and_the_cut(mf, ol, nuc_files, tmp_path):
    text, s1, s2 = nuc_files
    ks = mf.KmerSet.from_text(text, 31)
    starts, names, letters = [int(s) for s in ks.record_starts], ks.record_names, ks.bait_letters
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    t = lambda n: str(tmp_path / n)
    lib = {cut: mf.filter_fastq_files_verified(ks, fq1, fq2, t("l1.fq"), t("l2.fq"), 1, mf.PAIR_EITHER, min_depth=3, max_permille=cut) for cut in (1000, 30)}
    ks.close()
    assert int(lib[30].score_records["rejected"].sum()) > 0 == int(lib[1000].score_records["rejected"].sum())          # the cut cuts
    bait = t("bait.fa")
    open(bait, "w").write(text)

    def run(tag, extra):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq1, "--fq2", fq2, "-k", "31", "--out1", t(tag + "1.fq"), "--out2", t(tag + "2.fq")] + extra,
                           capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert p.stdout.decode().split() == [str(lib[1000].kept)]
        for m in ("1", "2"):
            assert md5(t(tag + m + ".fq")) == md5(t("l" + m + ".fq"))

    # the score report alone (no cut: 1000), alone at 30, and with each family at 30
    run("a", ["--score-report", t("s_alone.tsv")])
    assert open(t("s_alone.tsv")).read() == score_text(names, starts, lib[1000].score_records)
    run("b", ["--score-report", t("s_30.tsv"), "--max-mismatch", "30"])
    assert open(t("s_30.tsv")).read() == score_text(names, starts, lib[30].score_records)
    run("c", ["--score-report", t("s_place.tsv"), "--max-mismatch", "30", "--place-report", t("place_30.tsv"), "--base-depth", t("depth_30.tsv")])
    assert open(t("s_place.tsv")).read() == score_text(names, starts, lib[30].score_records)
    v = lib[30]
    want = "record\tname\tlength\tforward\treverse\tover_begin\tover_end\tcovered\tmean\tmax\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\t%d\n" % ((j, names[j], starts[j + 1] - starts[j]) + tuple(int(v.place_records[f][j]) for f in PLACE_REC[:5])
                                                      + (int(v.place_records["base_sum"][j]) / (starts[j + 1] - starts[j]) if starts[j + 1] > starts[j] else 0.0,
                                                         int(v.base_depth[starts[j]:starts[j + 1]].max()) if starts[j + 1] > starts[j] else 0))
        for j in range(len(names))) + "-\t*unplaced*\t%d\n" % int(v.unplaced[0])
    assert open(t("place_30.tsv")).read() == want
    assert open(t("depth_30.tsv")).read() == "".join("%s\t%d\t%d\n" % (names[j], p - starts[j] + 1, int(v.base_depth[p]))
                                                     for j in range(len(names)) for p in range(starts[j], starts[j + 1]))
    run("d", ["--score-report", t("s_pile.tsv"), "--max-mismatch", "30", "--pileup", t("pile_30.tsv"), "--consensus", t("cons_30.fa"),
              "--variants", t("var_30.tsv"), "--min-depth", "3"])
    assert open(t("s_pile.tsv")).read() == score_text(names, starts, lib[30].score_records)
    counts = counts_of(v.pileup)
    assert open(t("pile_30.tsv")).read() == "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((names[j], p - starts[j] + 1, chr(letters[p]), counts[p].sum()) + tuple(counts[p]))
                                                    for j in range(len(names)) for p in range(starts[j], starts[j + 1]))
    assert open(t("cons_30.fa")).read() == mf.consensus_fasta(names, starts, v.consensus)
    variants = mf.pileup_variants(starts, letters, v.pileup, v.consensus)
    assert open(t("var_30.tsv")).read() == "".join("%s\t%d\t%s\t%s\t%d\t%d\n" % (names[r["record"]], r["pos"] + 1, r["ref"].decode(), r["alt"].decode(), r["depth"], r["alt_count"])
                                                   for r in variants)
    # the cut changed something, and without the new flags the reports are those of a cut that cuts nothing
    run("e", ["--pileup", t("pile.tsv"), "--consensus", t("cons.fa"), "--variants", t("var.tsv"), "--min-depth", "3"])
    run("f", ["--pileup", t("pile_1000.tsv"), "--consensus", t("cons_1000.fa"), "--variants", t("var_1000.tsv"), "--min-depth", "3", "--max-mismatch", "1000",
              "--score-report", t("s_1000.tsv")])
    for n in ("pile", "var"):
        assert md5(t(n + ".tsv")) == md5(t(n + "_1000.tsv"))
    assert md5(t("cons.fa")) == md5(t("cons_1000.fa")) and md5(t("pile.tsv")) != md5(t("pile_30.tsv"))
    run("g", ["--place-report", t("place.tsv"), "--base-depth", t("depth.tsv")])
    run("h", ["--place-report", t("place_1000.tsv"), "--base-depth", t("depth_1000.tsv"), "--max-mismatch", "1000"])
    assert md5(t("place.tsv")) == md5(t("place_1000.tsv")) and md5(t("depth.tsv")) == md5(t("depth_1000.tsv"))
    assert md5(t("place.tsv")) != md5(t("place_30.tsv"))
    assert open(t("s_1000.tsv")).read() == open(t("s_alone.tsv")).read()


# ------------------------------------------------------------------ 9. bim
def test_bim_consensus_bait_with_a_cut(mf, tmp_path):
    """on the NUMT case the polished bait holds the bait's own letters wherever it is called; without the argument the file is today's"""
    from mitoflex_amd.bim import bim
    g, subst, clean, copies = numt_data()
    fa, fq = str(tmp_path / "bait.fa"), str(tmp_path / "k.fq")
    open(fa, "w").write(">g\n" + g + "\n")
    write_fastq(fq, clean + copies, "a")
    out = {n: str(tmp_path / (n + ".fa")) for n in ("default", "none", "cut")}
    r0 = bim.consensus_bait(fa, fq, None, out["default"], 21, 3)
    r1 = bim.consensus_bait(fa, fq, None, out["none"], 21, 3, max_permille=None)
    r2 = bim.consensus_bait(fa, fq, None, out["cut"], 21, 3, max_permille=30)
    assert md5(out["default"]) == md5(out["none"]) and np.array_equal(r0, r1)
    text = lambda p: "".join(open(p).read().split("\n")[1:])
    polluted, polished = text(out["none"]), text(out["cut"])
    assert len(polished) == len(g) and polished.upper() == g
    assert sum(a != b for a, b in zip(polluted.upper(), g)) == int(r0["variants"][0]) > 15
    assert int(r2["variants"][0]) == 0 and int(r2["called"][0]) == int(r0["called"][0]) == sum(c.isupper() for c in polished)
