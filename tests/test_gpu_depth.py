"""K-mer depth along the bait records (mf_kmerset_record_starts, mf_depth, mf_filter_fastq_files_depth, `fastfilter bait --depth-report /
--depth-profile`), for nucleotide and protein sets, against a plain-Python oracle written from the semantics in include/mitofilter.h: the
depth of the valid window at position p is the number of windows, over all reads that pass, whose key is the key of that window (canonical
for nucleotide sets, so both strands count; a key several bait windows hold gives its full count to each; a read holding a key twice counts
twice); the profile clamps it at 0xFFFFFFFE and holds DEPTH_NONE where no valid window starts; a record sums its valid windows, those of
depth >= 1, and the sum and maximum of their depths.  At file level every mate that passes its own threshold counts."""
import json
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from oracle import kmer_bait_ref as kb
from oracle import prot_bait_ref as pr
from tests.clade_data import Clade, gene_dna, sample_reads
from tests.report_data import fasta, keys_nuc, keys_prot, mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.util_data import bait_records, bits_to_bool, make_bait, make_reads, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NONE, CLAMP = 0xFFFFFFFF, 0xFFFFFFFE


# ------------------------------------------------------------------ oracle
class Oracle:
    """the expected depth of one set: positions, the valid windows and their keys"""

    def __init__(self, text, k, code=None):
        self.k, self.code = k, code
        recs = pr.protein_records(text) if code else kb.read_fasta_records(text)
        self.starts = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
        self.windows = []                     # (position, key, record) of every valid window
        for j, rec in enumerate(recs):
            s = rec if code else kb._norm(rec)
            for i in range(len(s) - k + 1):
                w = s[i:i + k]
                v = pr.pep_code(w) if code else (None if "N" in w else kb.canonical_code(w))
                if v is not None:
                    self.windows.append((int(self.starts[j]) + i, v, j))
        self.bait = {v for _, v, _ in self.windows}

    def keys(self, seqs):
        return [keys_prot(s, self.k, self.code) if self.code else keys_nuc(s, self.k) for s in seqs]

    def passes(self, keys, thr):
        return np.array([sum(v in self.bait for v in ks) >= thr for ks in keys], bool)

    def counts(self, keys, passes):
        c = Counter()
        for ks, p in zip(keys, passes):
            if p:
                c.update(v for v in ks if v in self.bait)
        return c

    def depth(self, cnt):
        """-> (unclamped depth per position, NONE where no valid window starts; records u64[R, 4])"""
        prof = np.full(int(self.starts[-1]), NONE, np.int64)
        rec = np.zeros((len(self.starts) - 1, 4), np.uint64)
        for p, v, j in self.windows:
            d = cnt[v]
            prof[p] = d
            rec[j, 0] += 1
            rec[j, 1] += d > 0
            rec[j, 2] += d
            rec[j, 3] = max(int(rec[j, 3]), d)
        return prof, rec


def clamp(prof):
    return np.where(prof == NONE, NONE, np.minimum(prof, CLAMP)).astype(np.uint32)


def as_rows(records):
    return np.stack([records[f] for f in ("windows", "covered", "depth_sum", "depth_max")], axis=1).astype(np.uint64)


def records_of(prof, starts):
    """per-record summary of an unclamped profile"""
    rec = np.zeros((len(starts) - 1, 4), np.uint64)
    for j in range(len(starts) - 1):
        d = prof[int(starts[j]):int(starts[j + 1])]
        d = d[d != NONE].astype(np.int64)
        if d.size:
            rec[j] = (d.size, int((d > 0).sum()), int(d.sum()), int(d.max()))
    return rec


# ------------------------------------------------------------------ data
def depth_bait():
    """records with invalid bases (IUPAC, N), shorter than k, empty, a stretch repeated within a record, k-mers shared between records
    (one of them reverse-complemented), an anonymous leading record, lower case"""
    r = bait_records(make_bait())
    g = r[0][:3000]
    rng = random.Random(7)
    x, y = "".join(rng.choices("ACGT", k=220)), "".join(rng.choices("ACGT", k=90))
    recs = [("mito desc", g), ("repeat", x + y + x + "acgtn" + y), ("empty", ""), ("tiny", "ACGTTGCA"),
            ("shared", revcomp(g[700:1300]) + g[2000:2400]), ("rec2", r[1][:1800]), ("rand", "".join(rng.choices("ACGT", k=1200)))]
    return "".join(rng.choices("ACGT", k=80)) + "\n" + fasta(recs), x


def depth_reads(text, x, n, seed, uniform):
    seqs = make_reads(text, n, seed=seed, uniform=uniform, mito_frac=0.5)
    seqs = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(seqs)]
    return seqs + [x + x[:60], revcomp(x + x[:80]), x[:100] + "N" + x[101:150]]          # keys held twice in one read; a ragged one with N


def check(mf, ks, reads, o, keys, thr, mode=None):
    passes = o.passes(keys, thr)
    bits, prof, recs = mf.record_depth(ks, reads, thr, mf.MODE_SCREENED if mode is None else mode)
    assert np.array_equal(bits_to_bool(bits, len(keys)), passes)
    fbits, _, _ = mf.filter_reads(ks, reads, thr, mf.MODE_SCREENED if mode is None else mode)
    assert np.array_equal(bits, fbits)
    oprof, orec = o.depth(o.counts(keys, passes))
    bad = np.nonzero(prof != clamp(oprof))[0]
    assert bad.size == 0, [(int(i), int(prof[i]), int(oprof[i])) for i in bad[:10]]
    assert np.array_equal(as_rows(recs), orec), (as_rows(recs), orec)
    return prof, recs


# ------------------------------------------------------------------ 1. nucleotide sets
@pytest.mark.parametrize("k", [21, 31, 41])
def test_nucleotide_matches_oracle(mf, ol, k):
    text, x = depth_bait()
    o = Oracle(text, k)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    for uniform in (True, False):
        seqs = depth_reads(text, x, 1500, seed=900 + k, uniform=uniform)
        keys = o.keys(seqs)
        reads = upload(mf, ol, seqs)
        for thr in (1, 2):
            results = [check(mf, ks, reads, o, keys, thr, mode) for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE)]
            assert np.array_equal(results[0][0], results[1][0])
            prof, recs = results[0]
            assert recs["windows"][3] == 0 and recs["windows"][4] == 0          # the empty record and the one shorter than k
            assert int(recs["depth_max"].max()) > 0
        reads.close()
    ks.close()


def test_repeats_and_strands(mf, ol):
    """a key a read holds twice counts twice; a key two bait windows hold counts in both; both strands count"""
    text, x = depth_bait()
    k = 31
    o = Oracle(text, k)
    ks = mf.KmerSet.from_text(text, k)
    seqs = [x, revcomp(x)]
    reads = upload(mf, ol, seqs)
    _, prof, recs = mf.record_depth(ks, reads, 1)
    rs = ks.record_starts
    p = int(rs[2])             # record 2, "repeat": x + y + x (record 0 is the anonymous leading one)
    assert prof[p] == 2 and prof[p + 310] == 2           # each key of x: once in either read, its full count in both bait windows
    assert prof[p + 220 - k + 1] == 0                    # spans x and y
    assert recs["depth_max"][2] == 2
    check(mf, ks, reads, o, o.keys(seqs), 1)
    reads.close(); ks.close()


@pytest.fixture()
def front(mf):
    def set_(mode, f2=0, f3=-1, canon=-1):
        mf.set_option("front", mode)
        mf.set_option("front2_log2b", f2)
        mf.set_option("front3_log2b", f3)
        mf.set_option("canon", canon)
    yield set_
    set_(-1, 0, -1, -1)


@pytest.mark.parametrize("form", [(1, 6, -1), (2, 6, 12), (3, 0, -1), (4, 6, 8), (2, 0, -1, 1), (4, 0, -1, 1)])
def test_large_bait_screen_forms(mf, ol, front, form):
    front(*form)
    text, x = depth_bait()
    k = 31
    o = Oracle(text, k)
    ks = mf.KmerSet.from_text(text, k)
    seqs = depth_reads(text, x, 1200, seed=77, uniform=False)
    keys = o.keys(seqs)
    reads = upload(mf, ol, seqs)
    for thr in (1, 2):
        check(mf, ks, reads, o, keys, thr)
    reads.close(); ks.close()


def test_depth_index_by_slot_gives_the_same(mf, ol):
    """the scattered form (a counter per table slot, kept to measure against) computes the same profile"""
    text, x = depth_bait()
    seqs = depth_reads(text, x, 800, seed=78, uniform=True)
    reads = upload(mf, ol, seqs)
    ks = mf.KmerSet.from_text(text, 31)
    want = mf.record_depth(ks, reads, 1)
    mf.set_option("depth_index", 1)
    try:
        ks2 = mf.KmerSet.from_text(text, 31)
        got = mf.record_depth(ks2, reads, 1)
    finally:
        mf.set_option("depth_index", 0)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    reads.close(); ks.close(); ks2.close()


# ------------------------------------------------------------------ 2. protein sets
@pytest.fixture(scope="module")
def clade():
    return Clade(n_species=6)


def protein_reads(clade, n, seed):
    dna = gene_dna(clade.unseen(0.04, seed=seed), 5, seed=seed + 1)
    seqs, _ = sample_reads(dna, n, seed=seed + 2)
    rng = random.Random(seed)
    out = []
    for i, s in enumerate(seqs):
        if i % 4 == 1:
            s = s[:rng.randint(20, len(s))]                   # ragged, some shorter than 3kp
        if i % 7 == 2:
            q = rng.randrange(len(s))
            s = s[:q] + "N" + s[q + 1:]
        out.append(s)
    return out + ["".join(rng.choices("ACGT", k=150)) for _ in range(n // 10)]


def test_protein_matches_oracle(mf, ol, clade):
    kp, code = 9, 5
    o = Oracle(clade.text, kp, code)
    ks = mf.KmerSet.protein_from_text(clade.text, kp, code)
    assert np.array_equal(ks.record_starts, o.starts)
    seqs = protein_reads(clade, 700, seed=41)
    keys = o.keys(seqs)
    reads = upload(mf, ol, seqs)
    for thr in (1, 2):
        _, recs = check(mf, ks, reads, o, keys, thr)
        assert int(recs["covered"].sum()) > 0
    reads.close(); ks.close()


def test_protein_record_calls_still_refused(mf, clade):
    ks = mf.KmerSet.protein_from_text(clade.text, 9, 5)
    assert len(ks.record_starts) == len(ks.group_names) + 1
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        ks.record_names
    ks.close()


# ------------------------------------------------------------------ 3. file level
@pytest.fixture(scope="module")
def nuc_files():
    text, x = depth_bait()
    s1 = depth_reads(text, x, 1800, seed=51, uniform=False)
    s2 = depth_reads(text, x, 1800, seed=52, uniform=False)
    return text, s1, s2


def in_memory(mf, ol, ks, seqs, thr):
    """the unclamped in-memory profile of one mate's reads (the test data stays far below the clamp)"""
    reads = upload(mf, ol, seqs)
    _, prof, _ = mf.record_depth(ks, reads, thr)
    reads.close()
    return prof.astype(np.int64)


def summed(profs):
    out = profs[0].copy()
    for p in profs[1:]:
        out = np.where(out == NONE, NONE, out + p)
    return out


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
@pytest.mark.parametrize("pe,pair", [(False, 0), (True, 0), (True, 1)])
def test_files_depth(mf, ol, nuc_files, tmp_path, monkeypatch, ingest, pe, pair):
    text, s1, s2 = nuc_files
    gz = ingest == "device-gz"
    monkeypatch.setenv("MF_INGEST", "device" if gz else "host")
    monkeypatch.setenv("MF_BATCH_READS", "300")
    monkeypatch.setenv("MF_GZDEV_CHUNK_BYTES", "8192")
    monkeypatch.setenv("MF_GZDEV_SLAB_CHUNKS", "5")
    monkeypatch.setenv("MF_GZDEV_TEXT_PIECE", "100000")
    ext = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + ext)), (str(tmp_path / ("a_2" + ext)) if pe else None)
    write_fastq(fq1, s1, "a", gz=gz)
    if pe:
        write_fastq(fq2, s2, "b", gz=gz)
    ks = mf.KmerSet.from_text(text, 31)
    o = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    for thr in (1, 2):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, o[0], o[1] if pe else None, thr, pair)
        kept, total, prof, recs = mf.filter_fastq_files_depth(ks, fq1, fq2, o[2], o[3] if pe else None, thr, pair)
        assert mf.last_ingest_stats()["path"] == (1 if gz else 0)
        assert (kept, total) == (kept0, total0)
        assert open(o[2], "rb").read() == open(o[0], "rb").read()
        if pe:
            assert open(o[3], "rb").read() == open(o[1], "rb").read()
        want = summed([in_memory(mf, ol, ks, s, thr) for s in ([s1, s2] if pe else [s1])])
        assert np.array_equal(prof.astype(np.int64), want)
        assert np.array_equal(as_rows(recs), records_of(want, ks.record_starts))
    orc = Oracle(text, 31)
    keys = orc.keys(s1 + (s2 if pe else []))
    oprof, orec = orc.depth(orc.counts(keys, orc.passes(keys, 2)))
    assert np.array_equal(prof, clamp(oprof)) and np.array_equal(as_rows(recs), orec)
    ks.close()


def test_files_depth_protein(mf, ol, clade, tmp_path, monkeypatch):
    monkeypatch.setenv("MF_INGEST", "device")
    monkeypatch.setenv("MF_GZDEV_CHUNK_BYTES", "8192")
    monkeypatch.setenv("MF_GZDEV_TEXT_PIECE", "60000")
    s1, s2 = protein_reads(clade, 500, seed=61), protein_reads(clade, 500, seed=62)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    ks = mf.KmerSet.protein_from_text(clade.text, 9, 5)
    kept0, _ = mf.filter_fastq_files(ks, fq1, fq2, str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq"), 1, mf.PAIR_BOTH)
    kept, _, prof, recs = mf.filter_fastq_files_depth(ks, fq1, fq2, str(tmp_path / "d1.fq"), str(tmp_path / "d2.fq"), 1, mf.PAIR_BOTH)
    assert kept == kept0
    for m in ("1", "2"):
        assert open(str(tmp_path / ("d%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
    want = summed([in_memory(mf, ol, ks, s, 1) for s in (s1, s2)])
    assert np.array_equal(prof.astype(np.int64), want)
    assert np.array_equal(as_rows(recs), records_of(want, ks.record_starts))
    ks.close()


def test_files_depth_two_devices(mf, ol, nuc_files, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), on both ingest paths, in a child process"""
    text, s1, s2 = nuc_files
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    ks = mf.KmerSet.from_text(text, 31)
    want = summed([in_memory(mf, ol, ks, s, 1) for s in (s1, s2)])
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
            "a = mf.filter_fastq_files(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/o1.fq', sys.argv[4] + '/o2.fq', 1, 0, devices=[0, 1])\n"
            "b = mf.filter_fastq_files_depth(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 0, devices=[0, 1])\n"
            "print(json.dumps({'a': list(a), 'kept': b[0], 'total': b[1], 'profile': [int(x) for x in b[2]],"
            " 'path': mf.last_ingest_stats()['path'], 'n_dev': mf.last_ingest_stats()['n_devices']}))\n")
        env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_GZDEV_CHUNK_BYTES="8192",
                   MF_GZDEV_SLAB_CHUNKS="5", MF_GZDEV_TEXT_PIECE="100000", MF_BATCH_READS="400", PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert r["path"] == (1 if ingest == "device" else 0) and r["n_dev"] == 2
        assert r["a"] == [r["kept"], r["total"]]
        for m in ("1", "2"):
            assert open(str(tmp_path / ("g%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
        assert np.array_equal(np.array(r["profile"], np.int64), want)


# ------------------------------------------------------------------ 4. CLI
def tsvs(names, starts, prof):
    rec = records_of(prof, starts)
    report = "record\tname\tlength\twindows\tcovered\tmean\tmax\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\t%.3f\t%d\n" % (j, n, int(starts[j + 1] - starts[j]), rec[j, 0], rec[j, 1],
                                             (int(rec[j, 2]) / int(rec[j, 0])) if rec[j, 0] else 0.0, rec[j, 3])
        for j, n in enumerate(names))
    profile = "".join("%s\t%d\t%d\n" % (n, p - int(starts[j]) + 1, prof[p])
                      for j, n in enumerate(names) for p in range(int(starts[j]), int(starts[j + 1])) if prof[p] != NONE)
    return report, profile


@pytest.mark.parametrize("protein", [False, True])
def test_cli_depth_report_and_profile(mf, ol, nuc_files, clade, tmp_path, protein):
    if protein:
        text, s1, s2 = clade.text, protein_reads(clade, 400, seed=71), protein_reads(clade, 400, seed=72)
        ks = mf.KmerSet.protein_from_text(text, 9, 5)
        flags = ["--protein", "--code", "5", "-k", "9"]
    else:
        text, s1, s2 = nuc_files
        ks = mf.KmerSet.from_text(text, 31)
        flags = ["-k", "31"]
    want = summed([in_memory(mf, ol, ks, s, 1) for s in (s1, s2)])
    starts, names = ks.record_starts, ks.group_names
    ks.close()
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    base = [CLI, "bait", "--bait", bait, "--fq1", fq1, "--fq2", fq2] + flags
    p0 = subprocess.run(base + ["--out1", str(tmp_path / "o1.fq"), "--out2", str(tmp_path / "o2.fq")], capture_output=True, timeout=300)
    assert p0.returncode == 0, p0.stderr.decode()[-2000:]
    rep, prof = str(tmp_path / "depth.tsv"), str(tmp_path / "profile.tsv")
    p1 = subprocess.run(base + ["--out1", str(tmp_path / "d1.fq"), "--out2", str(tmp_path / "d2.fq"), "--depth-report", rep, "--depth-profile", prof],
                        capture_output=True, timeout=300)
    assert p1.returncode == 0, p1.stderr.decode()[-2000:]
    assert p1.stdout == p0.stdout
    for m in ("1", "2"):
        assert open(str(tmp_path / ("d%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
    wrep, wprof = tsvs(names, starts, want)
    assert open(rep).read() == wrep
    assert open(prof).read() == wprof
    # either flag alone
    p2 = subprocess.run(base + ["--out1", str(tmp_path / "e1.fq"), "--out2", str(tmp_path / "e2.fq"), "--depth-profile", str(tmp_path / "p2.tsv")],
                        capture_output=True, timeout=300)
    assert p2.returncode == 0 and open(str(tmp_path / "p2.tsv")).read() == wprof


def test_low_complexity_reads(mf, ol):
    """microsatellite and poly-A reads pile onto a few keys (the wave adds repeated keys once, by count)"""
    text, x = depth_bait()
    text += fasta([("msat", "GC" * 5 + "TA" * 70 + "C" + "A" * 90 + "CAG" * 40 + "G")])
    o = Oracle(text, 31)
    ks = mf.KmerSet.from_text(text, 31)
    rng = random.Random(83)
    seqs = depth_reads(text, x, 400, seed=84, uniform=False)
    for i in range(300):
        m = rng.choice(["A", "TA", "AT", "CAG", "T", "TG"])
        s = (m * 200)[rng.randrange(3):][:rng.choice([150, 150, 64, 65, 97, 200])]
        seqs.append(revcomp(s) if i % 2 else s)
    reads = upload(mf, ol, seqs)
    for thr in (1, 2):
        _, recs = check(mf, ks, reads, o, o.keys(seqs), thr)
    assert int(recs["depth_max"][-1]) > 1000
    reads.close(); ks.close()
