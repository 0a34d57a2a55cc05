"""The pile-up of the placed reads (mf_pileup, mf_filter_fastq_files_pileup, `fastfilter bait --pileup / --consensus / --variants`,
bim.consensus_bait) against the plain-Python oracle of tests/pileup_oracle.py, which is written from the semantics in
include/mitofilter.h: base counts, consensus bytes, every record field, the unplaced counts and the pass bitmap are compared exactly.

The clamp at 0xFFFFFFFE is not reachable at test size (it takes 2^32 bases on one position): only the oracle's side of min(..) holds it.

One case is not as the issue that asked for these tests words it: it lists the `palindrome` read among those that contribute nothing,
but that read IS placed (tests/test_gpu_place.py asserts it: only its one window that is its own reverse complement casts no vote), so
by the header's text its 130 bases are piled.  The test asserts that."""
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
from tests.report_data import fasta, mf, mutate, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_bim import _genome, _pairs
from tests.test_gpu_place import place_bait, place_reads, special_reads
from tests.util_data import bits_to_bool, make_protein_bait, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
LETTERS = ("a", "c", "g", "t")
REC_FIELDS = ("bases", "matches", "mismatches", "called", "ambiguous", "variants")


def counts_of(pileup):
    return np.stack([pileup[f].astype(np.int64) for f in LETTERS], axis=1)


def rec_rows(records):
    return np.stack([records[f] for f in REC_FIELDS], axis=1).astype(np.uint64)


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


def check(mf, ks, reads, P, seqs, tallies, thr, mode, min_depth, want=None):
    """one mf_pileup call against the oracle; want: (passes, rows, unplaced, counts) of this threshold, computed once"""
    if want is None:
        passes, rows, _, _, unplaced = P.o.place(tallies, thr)
        want = (passes, rows, unplaced, P.pile(seqs, rows))
    passes, rows, unplaced, counts = want
    cons, rec = P.call(counts, min_depth)
    bits, pileup, consensus, records, unpl = mf.pileup_reads(ks, reads, thr, mode, min_depth)
    assert np.array_equal(bits_to_bool(bits, len(seqs)), passes)
    got = counts_of(pileup)
    bad = np.nonzero((got != pio.clamped(counts)).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), counts[i].tolist()) for i in bad[:10]]
    bad = np.nonzero(consensus != cons)[0]
    assert bad.size == 0, [(int(i), chr(consensus[i]), chr(cons[i]), counts[i].tolist()) for i in bad[:10]]
    assert np.array_equal(rec_rows(records), rec), (rec_rows(records), rec)
    assert unpl.tolist() == unplaced
    # the host helper on the device's results gives the oracle's variants
    v = mf.pileup_variants(ks.record_starts, ks.bait_letters, pileup, consensus)
    assert [(int(r["record"]), int(r["pos"]), r["ref"].decode(), r["alt"].decode(), int(r["depth"]), int(r["alt_count"])) for r in v] == P.variants(counts, cons)
    assert len(v) == int(rec[:, 5].sum())
    return want


# ------------------------------------------------------------------ 1. in memory
@pytest.mark.parametrize("k", [21, 31, 32, 41])
def test_pileup_matches_oracle(mf, ol, k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    P = pio.PileupOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    assert bytes(ks.bait_letters).decode() == P.bait
    g = parts["g"]
    for uniform in (False, True):
        names, seqs = place_reads(text, parts, k, 1200, seed=900 + k, uniform=uniform)
        if not uniform:          # reads of a sample that differs from the bait at 1 % of its positions: variants and mismatches
            seqs = seqs + drawn(mutate(g, 0.01, 77), 200, seed=78)
        tallies = o.tally(seqs)
        reads = upload(mf, ol, seqs)
        for thr in (1, 3):
            want = None
            for min_depth in (1, 3):
                for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                    want = check(mf, ks, reads, P, seqs, tallies, thr, mode, min_depth, want)
            if not uniform:
                rec = P.call(want[3], 3)[1]
                assert int(rec[:, 5].sum()) > 0 and int(rec[:, 2].sum()) > 0          # variants, mismatches
        reads.close()
    ks.close()


@pytest.mark.parametrize("k", [21, 32])
def test_special_reads_one_by_one(mf, ol, k):
    """every read that was built for a case of the base walk, piled alone, so that what it puts where can be stated without the oracle"""
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    P = pio.PileupOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    R = {n: j for j, n in enumerate(ks.record_names)}
    st = [int(s) for s in ks.record_starts]
    span = lambda name: slice(st[R[name]], st[R[name] + 1])
    g, left, right = parts["g"], parts["left"], parts["right"]
    names, special = special_reads(parts, k)
    got = {}
    for name, seq in zip(names, special):
        reads = upload(mf, ol, [seq])
        want = check(mf, ks, reads, P, [seq], o.tally([seq]), 1, mf.MODE_SCREENED, 1)
        _, pileup, _, records, unpl = mf.pileup_reads(ks, reads, 1, mf.MODE_SCREENED, 1)
        _, _, base_depth, _, _ = mf.place_reads(ks, reads, 1)
        reads.close()
        got[name] = (counts_of(pileup), records, unpl.tolist(), base_depth.astype(np.int64), want[1][0])

    def only_in(name, rec, lo, hi, letters):
        c = got[name][0]
        assert int(c.sum()) == hi - lo, name
        assert np.array_equal(c[st[R[rec]] + lo:st[R[rec]] + hi], one_hot(letters)), name
        assert got[name][2] == [0, 0]

    # clipped at the ends of the record, nothing on the neighbour
    only_in("over_begin", "mito", 0, 100, g[:100])
    assert got["over_begin"][0][:st[R["mito"]]].sum() == 0                          # the anonymous record in front of `mito`
    only_in("over_end", "mito", 3000 - 90, 3000, g[-90:])                           # reverse strand: complemented back to the bait's letters
    assert got["over_end"][0][span("repeat")].sum() == 0
    only_in("over_both", "left", 0, 600, left)
    assert got["over_both"][0][span("rand")].sum() == 0 and got["over_both"][0][span("right")].sum() == 0
    # placed on `left`; the 70 bases that overhang lie on global positions of `right` and must not be counted there
    only_in("junction", "left", 520, 600, left[-80:])
    c = got["junction"][0]
    assert c[st[R["left"]]].tolist() == [0, 0, 0, 0] and c[st[R["left"] + 1] - 1].tolist() == one_hot(left[-1])[0].tolist()
    assert c[st[R["right"]]].tolist() == [0, 0, 0, 0] and c[st[R["right"] + 1] - 1].tolist() == [0, 0, 0, 0]
    assert c[span("right")].sum() == 0
    # the N counts nowhere: base depth exceeds the count sum by one there, and only there
    c, depth = got["with_n"][0], got["with_n"][3]
    assert c[st[R["mito"]] + 580].tolist() == [0, 0, 0, 0] and depth[st[R["mito"]] + 580] == 1
    assert np.array_equal(np.nonzero(depth - c.sum(axis=1))[0], [st[R["mito"]] + 580])
    assert int(c.sum()) == 149
    # no indel handling: behind the insertion the shifted bases pile up as mismatches
    seq = special[names.index("insertion")]
    assert got["insertion"][4].tolist()[:4] == [R["mito"], 0, 1400, 1556]
    mism = sum(a != b for a, b in zip(seq, g[1400:1556]))
    assert mism > 20 and all(a == b for a, b in zip(seq[:90], g[1400:1490]))
    rec = got["insertion"][1][R["mito"]]
    assert (int(rec["bases"]), int(rec["matches"]), int(rec["mismatches"])) == (156, 156 - mism, mism)
    # not placed: nothing anywhere
    for name in ("tie", "no_anchor", "no_anchor_rc"):
        assert got[name][0].sum() == 0 and got[name][2] == [1, 0], name
    # placed (its window that is its own reverse complement casts no vote, but the read's bases are piled)
    only_in("palindrome", "pal", 200, 330, parts["pal"][200:330])
    # about 1 500 bases on the reverse strand: many 64-base chunks, complemented; the whole read counts on its winning diagonal
    for name in ("scattered_first", "scattered_last"):
        seq, row = special[names.index(name)], got[name][4]
        assert len(seq) > 1400 and row[0] == R["mito"] and row[1] == (name == "scattered_last")
        inside = [i for i, ch in enumerate(seq) if ch != "N" and 0 <= (row[2] + i if row[1] == 0 else row[2] + len(seq) - 1 - i) < 3000]
        assert int(got[name][0].sum()) == len(inside) > 64 * 4
        assert got[name][0][:st[R["mito"]]].sum() == 0 and got[name][0][st[R["mito"] + 1]:].sum() == 0
        assert int(got[name][1][R["mito"]]["matches"]) >= k + 1
    ks.close()


def test_engineered_tie(mf, ol):
    """two reads that differ in one letter and nothing else on the spot: an exact tie at min_depth 2"""
    text, parts = place_bait()
    o = po.PlaceOracle(text, 31)
    P = pio.PileupOracle(o)
    ks = mf.KmerSet.from_text(text, 31)
    left = parts["left"]
    a = left[100:250]
    b = a[:60] + ("C" if a[60] != "C" else "G") + a[61:]
    seqs = [a, revcomp(b)]
    reads = upload(mf, ol, seqs)
    tallies = o.tally(seqs)
    at = int(ks.record_starts[ks.record_names.index("left")]) + 160
    for min_depth, byte, ambiguous in ((1, "N", 1), (2, "N", 1), (3, left[160].lower(), 0)):
        check(mf, ks, reads, P, seqs, tallies, 1, mf.MODE_SCREENED, min_depth)
        _, pileup, consensus, records, _ = mf.pileup_reads(ks, reads, 1, mf.MODE_SCREENED, min_depth)
        c = counts_of(pileup)[at]
        assert sorted(c.tolist()) == [0, 0, 1, 1] and c["ACGT".index(a[60])] == 1 and c["ACGT".index(b[60])] == 1
        assert chr(consensus[at]) == byte
        assert int(records["ambiguous"].sum()) == ambiguous and int(records["variants"].sum()) == 0
        assert int(records["called"].sum()) == (149 if min_depth < 3 else 0)
        assert bytes(consensus[at - 60:at + 90]).decode() == (left[100:160] + byte + left[161:250] if min_depth < 3 else left[100:250].lower())
    reads.close(); ks.close()


def test_protein_set_is_refused(mf, ol):
    text = make_protein_bait()[0]
    ks = mf.KmerSet.protein_from_text(text, 9, 5)
    reads = upload(mf, ol, ["ACGT" * 40] * 4)
    with pytest.raises(mf.MitoFilterError, match="error -1"):
        mf.pileup_reads(ks, reads, 1)
    with pytest.raises(mf.MitoFilterError, match="error -1"):
        mf.filter_fastq_files_pileup(ks, "a.fq", None, "o.fq", None)
    with pytest.raises(mf.MitoFilterError, match="error -1"):
        ks.bait_letters
    reads.close(); ks.close()
    nuc = mf.KmerSet.from_text(place_bait()[0], 31)
    reads = upload(mf, ol, ["ACGT" * 40] * 4)
    with pytest.raises(mf.MitoFilterError, match="min_depth"):
        mf.pileup_reads(nuc, reads, 1, min_depth=0)
    reads.close(); nuc.close()


# ------------------------------------------------------------------ 2. consistency with placement
def test_pileup_agrees_with_placement(mf, ol):
    """on reads without N the count sum is the base depth everywhere, and a pile-up call leaves placement's own results as they are"""
    text, parts = place_bait()
    ks = mf.KmerSet.from_text(text, 31)
    _, seqs = place_reads(text, parts, 31, 1200, seed=321, uniform=True)
    _, ragged = place_reads(text, parts, 31, 600, seed=322, uniform=False)
    for s in ([x for x in seqs if x and not x.strip("ACGT")], [x for x in ragged if x and not x.strip("ACGT")]):
        assert len(s) > 300
        reads = upload(mf, ol, s)
        for thr in (1, 3):
            bits, pileup, _, records, unpl = mf.pileup_reads(ks, reads, thr)
            pbits, _, base_depth, precs, punpl = mf.place_reads(ks, reads, thr)
            assert np.array_equal(counts_of(pileup).sum(axis=1), base_depth.astype(np.int64))
            assert np.array_equal(bits, pbits) and unpl.tolist() == punpl.tolist()
            assert np.array_equal(records["bases"], precs["base_sum"])
        reads.close()
    ks.close()


# ------------------------------------------------------------------ 3. stacked reads
def test_stacked_reads(mf, ol):
    """thousands of copies of one read and of its reverse complement on one start (amplicon data): every wave adds to the same counters,
    and the counts must still be exact"""
    text, parts = place_bait()
    o = po.PlaceOracle(text, 31)
    P = pio.PileupOracle(o)
    ks = mf.KmerSet.from_text(text, 31)
    g = parts["g"]
    uniq = [g[300:450], revcomp(g[300:450]), g[1400:1520]]
    tally = o.tally(uniq)
    seqs = uniq[:2] * 1500 + uniq[2:] * 500
    tallies = tally[:2] * 1500 + tally[2:] * 500
    reads = upload(mf, ol, seqs)
    want = check(mf, ks, reads, P, seqs, tallies, 1, mf.MODE_SCREENED, 3)
    at = int(ks.record_starts[ks.record_names.index("mito")])
    assert np.array_equal(want[3][at + 300:at + 450], 3000 * one_hot(g[300:450]))
    reads.close(); ks.close()


# ------------------------------------------------------------------ 4. round trip, independent of the oracle
def round_trip_data():
    g = _genome(3000, 11)
    s = mutate(g, 0.01, 12)
    return g, s, drawn(s, 480, seed=13)          # about 20 x


def test_round_trip_recovers_the_sample(mf, ol):
    """error-free reads of a sample that differs from the bait at 1 % of its positions: every called letter is the sample's, and every
    variant is a position where the sample differs (run on the oracle alone on the CPU first: it satisfies the same properties)"""
    g, s, seqs = round_trip_data()
    text = ">g\n" + g + "\n"
    ks = mf.KmerSet.from_text(text, 21)
    reads = upload(mf, ol, seqs)
    _, pileup, consensus, records, unpl = mf.pileup_reads(ks, reads, 1, mf.MODE_SCREENED, 3)
    reads.close()
    cons = bytes(consensus).decode()
    called = [p for p, ch in enumerate(cons) if ch in "ACGT"]
    assert all(cons[p] == s[p] for p in called)
    v = mf.pileup_variants(ks.record_starts, ks.bait_letters, pileup, consensus)
    assert int(records["variants"][0]) == len(v) > 0
    assert all(s[int(r["pos"])] != g[int(r["pos"])] and r["alt"].decode() == s[int(r["pos"])] and r["ref"].decode() == g[int(r["pos"])] for r in v)
    assert all(int(r["alt_count"]) == int(r["depth"]) for r in v)          # error-free reads: no base disagrees
    # how much is called is the oracle's exact count, not a fraction
    o = po.PlaceOracle(text, 21)
    P = pio.PileupOracle(o)
    rows = o.place(o.tally(seqs), 1)[1]
    ocons, orec = P.call(P.pile(seqs, rows), 3)
    assert int(records["called"][0]) == len(called) == int(orec[0, 3]) > 2900
    assert np.array_equal(consensus, ocons) and np.array_equal(rec_rows(records), orec)
    ks.close()


# ------------------------------------------------------------------ 5. file level
@pytest.fixture(scope="module")
def nuc_files():
    text, parts = place_bait()
    _, s1 = place_reads(text, parts, 31, 900, seed=51, uniform=False)
    _, s2 = place_reads(text, parts, 31, 900, seed=52, uniform=False)
    s1, s2 = [s or "A" for s in s1], [s or "A" for s in s2]
    return text, s1, s2[:len(s1)]


def in_memory(mf, ol, ks, seqs, thr):
    reads = upload(mf, ol, seqs)
    _, pileup, _, records, unplaced = mf.pileup_reads(ks, reads, thr)
    reads.close()
    return counts_of(pileup), rec_rows(records), unplaced


def summed(P, parts, min_depth):
    """what the file-level call gives for the mates piled in memory: counts and the sums add, the calls come from the summed counts"""
    counts = sum(p[0] for p in parts)
    cons, rec = P.call(counts, min_depth)
    assert np.array_equal(rec[:, :3], sum(p[1] for p in parts)[:, :3])          # bases, matches, mismatches add over the mates
    return counts, cons, rec, sum(p[2] for p in parts)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_pileup_equals_the_mates_in_memory(mf, ol, nuc_files, tmp_path, monkeypatch, ingest):
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
    for thr, min_depth in ((1, 1), (3, 2)):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, out[0], out[1], thr, mf.PAIR_BOTH)
        kept, total, pileup, consensus, records, unplaced = mf.filter_fastq_files_pileup(ks, fq1, fq2, out[2], out[3], thr, mf.PAIR_BOTH,
                                                                                         min_depth=min_depth)
        assert mf.last_ingest_stats()["path"] == (1 if gz else 0)
        assert (kept, total) == (kept0, total0)
        assert md5(out[2]) == md5(out[0]) and md5(out[3]) == md5(out[1])
        wcounts, wcons, wrec, wunpl = summed(P, [in_memory(mf, ol, ks, s, thr) for s in (s1, s2)], min_depth)
        assert np.array_equal(counts_of(pileup), wcounts)
        assert np.array_equal(consensus, wcons)
        assert np.array_equal(rec_rows(records), wrec)
        assert unplaced.tolist() == wunpl.tolist()
    ks.close()


def test_files_pileup_two_devices(mf, ol, nuc_files, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), on both ingest paths, in a child process"""
    text, s1, s2 = nuc_files
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    ks = mf.KmerSet.from_text(text, 31)
    P = pio.PileupOracle(po.PlaceOracle(text, 31))
    wcounts, wcons, wrec, wunpl = summed(P, [in_memory(mf, ol, ks, s, 1) for s in (s1, s2)], 2)
    ks.close()
    for gz, ingest in ((True, "device"), (False, "host")):
        ext = ".fq.gz" if gz else ".fq"
        fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
        write_fastq(fq1, s1, "a", gz=gz)
        write_fastq(fq2, s2, "b", gz=gz)
        script = (
            "import json, sys\n"
            "from mitoflex_amd import mitofilter as mf\n"
            "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
            "a = mf.filter_fastq_files(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/o1.fq', sys.argv[4] + '/o2.fq', 1, 1, devices=[0, 1])\n"
            "b = mf.filter_fastq_files_pileup(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 1, devices=[0, 1], min_depth=2)\n"
            "print(json.dumps({'a': list(a), 'kept': b[0], 'total': b[1], 'pileup': [[int(v) for v in r] for r in b[2]],"
            " 'consensus': bytes(b[3]).decode(), 'records': [[int(v) for v in r] for r in b[4]], 'unplaced': [int(x) for x in b[5]],"
            " 'path': mf.last_ingest_stats()['path'], 'n_dev': mf.last_ingest_stats()['n_devices']}))\n")
        env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_GZDEV_CHUNK_BYTES="8192",
                   MF_GZDEV_SLAB_CHUNKS="5", MF_GZDEV_TEXT_PIECE="100000", MF_BATCH_READS="400", PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert r["path"] == (1 if ingest == "device" else 0) and r["n_dev"] == 2
        assert r["a"] == [r["kept"], r["total"]]
        for m in ("1", "2"):
            assert md5(str(tmp_path / ("g%s.fq" % m))) == md5(str(tmp_path / ("o%s.fq" % m)))
        assert np.array_equal(np.array(r["pileup"], np.int64), wcounts)
        assert r["consensus"] == bytes(wcons).decode()
        assert np.array_equal(np.array(r["records"], np.uint64), wrec)
        assert r["unplaced"] == wunpl.tolist()


# ------------------------------------------------------------------ 6. CLI
def test_cli_pileup_consensus_and_variants(mf, ol, nuc_files, tmp_path):
    text, s1, s2 = nuc_files
    o = po.PlaceOracle(text, 31)
    P = pio.PileupOracle(o)
    counts = sum(P.pile(s, o.place(o.tally(s), 1)[1]) for s in (s1, s2))
    cons, _ = P.call(counts, 3)
    ks = mf.KmerSet.from_text(text, 31)
    starts, names = [int(s) for s in ks.record_starts], ks.record_names
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    kept, _ = mf.filter_fastq_files(ks, fq1, fq2, str(tmp_path / "l1.fq"), str(tmp_path / "l2.fq"), 1, mf.PAIR_EITHER)
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    base = [CLI, "bait", "--bait", bait, "--fq1", fq1, "--fq2", fq2, "-k", "31"]
    pil, con, var = str(tmp_path / "pile.tsv"), str(tmp_path / "cons.fa"), str(tmp_path / "var.tsv")
    p1 = subprocess.run(base + ["--out1", str(tmp_path / "d1.fq"), "--out2", str(tmp_path / "d2.fq"), "--pileup", pil, "--consensus", con,
                                "--variants", var, "--min-depth", "3"], capture_output=True, timeout=300)
    assert p1.returncode == 0, p1.stderr.decode()[-2000:]
    assert p1.stdout.decode().split() == [str(kept)]
    for m in ("1", "2"):
        assert md5(str(tmp_path / ("d%s.fq" % m))) == md5(str(tmp_path / ("l%s.fq" % m)))
    want_pile = "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((names[j], p - starts[j] + 1, P.bait[p], counts[p].sum()) + tuple(counts[p]))
                        for j in range(len(names)) for p in range(starts[j], starts[j + 1]))
    assert open(pil).read() == want_pile
    want_cons = "".join(">%s\n%s" % (names[j], "".join(bytes(cons[a:min(a + 60, starts[j + 1])]).decode() + "\n" for a in range(starts[j], starts[j + 1], 60)))
                        for j in range(len(names)))
    assert open(con).read() == want_cons == mf.consensus_fasta(names, starts, cons)
    variants = P.variants(counts, cons)
    assert len(variants) > 0
    assert open(var).read() == "".join("%s\t%d\t%s\t%s\t%d\t%d\n" % (names[j], pos + 1, ref, alt, d, n) for j, pos, ref, alt, d, n in variants)
    # the consensus can be baited with again: the same records at the same positions
    again = mf.KmerSet.from_fasta(con, 31)
    assert np.array_equal(again.record_starts, ks.record_starts)
    again.close(); ks.close()
    # any flag alone; --min-depth defaults to 1
    cons1, _ = P.call(counts, 1)
    p2 = subprocess.run(base + ["--out1", str(tmp_path / "e1.fq"), "--out2", str(tmp_path / "e2.fq"), "--consensus", str(tmp_path / "c2.fa")],
                        capture_output=True, timeout=300)
    assert p2.returncode == 0 and open(str(tmp_path / "c2.fa")).read() == mf.consensus_fasta(names, starts, cons1)
    p3 = subprocess.run(base + ["--out1", str(tmp_path / "f1.fq"), "--out2", str(tmp_path / "f2.fq"), "--pileup", str(tmp_path / "p3.tsv")],
                        capture_output=True, timeout=300)
    assert p3.returncode == 0 and open(str(tmp_path / "p3.tsv")).read() == want_pile


# ------------------------------------------------------------------ 7. bim
def test_bim_consensus_bait(mf, tmp_path):
    """simulated pairs with 1 % errors at ~55 x over a bait that differs from their genome at 1 % of its positions: the consensus bait is
    the genome again wherever it is called"""
    from mitoflex_amd.bim import bim
    g = _genome()
    old = mutate(g, 0.01, 5)
    text = ">g\n" + "\n".join(old[i:i + 60] for i in range(0, len(old), 60)) + "\n>other\n" + _genome(900, 5) + "\n"
    fa, out = str(tmp_path / "bait.fa"), str(tmp_path / "next.fa")
    open(fa, "w").write(text)
    m1, m2, _ = _pairs(g, 3000, 1)
    fq1, fq2 = str(tmp_path / "k.1.fq"), str(tmp_path / "k.2.fq")
    write_fastq(fq1, m1, "a")
    write_fastq(fq2, m2, "b")
    records = bim.consensus_bait(fa, fq1, fq2, out, 31, 3)
    ks = mf.KmerSet.from_fasta(fa, 31)
    _, _, _, consensus, recs, _ = mf.filter_fastq_files_pileup(ks, fq1, fq2, str(tmp_path / "t1.fq"), str(tmp_path / "t2.fq"), min_depth=3)
    assert open(out).read() == mf.consensus_fasta(ks.record_names, ks.record_starts, consensus)
    assert np.array_equal(rec_rows(records), rec_rows(recs))
    cons = bytes(consensus[:len(g)]).decode()
    called = [p for p, ch in enumerate(cons) if ch in "ACGT"]
    assert len(called) == int(records["called"][0]) > 0.99 * len(g)
    assert sum(cons[p] == g[p] for p in called) == len(called)          # (1 % errors against ~55 x: the majority is the genome's letter)
    differ = sum(old[p] != g[p] for p in called)
    assert int(records["variants"][0]) == differ > 100
    assert int(records["called"][1]) == 0 and int(records["bases"][1]) == 0
    nxt = mf.KmerSet.from_fasta(out, 31)
    assert np.array_equal(nxt.record_starts, ks.record_starts) and nxt.record_names == ks.record_names
    nxt.close(); ks.close()
