"""Record assignment of baited reads (mf_assign, mf_filter_fastq_files_by_record, `fastfilter bait --report`) against a plain-Python
oracle written straight from the spec (include/mitofilter.h): a key is unique to record j when j is the only record with a valid window
holding it; a passing read goes to the record with the strictly largest count of its windows whose key is unique to it, ambiguous when
there is none or a tie, unassigned when it does not pass."""
import json
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from oracle.kmer_bait_ref import _norm, canonical_code, read_fasta_records
from tests.report_data import eight_record_bait, fasta, mf, mutate, ol  # noqa: F401  (mf, ol: fixtures)
from tests.util_data import bait_records, bits_to_bool, make_bait, make_protein_bait, make_reads, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
AMB, NONE = 0xFFFFFFFE, 0xFFFFFFFF


# ------------------------------------------------------------------ oracle
def oracle_owners(fasta_text, k):
    """canonical key -> the record it is unique to, or -1 (shared)"""
    own = {}
    for j, rec in enumerate(read_fasta_records(fasta_text)):
        s = _norm(rec)
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if "N" in w:
                continue
            c = canonical_code(w)
            o = own.get(c)
            own[c] = j if o is None or o == j else -1
    return own


def oracle_tally(seq, k, own):
    """(hits, u: Counter record -> windows unique to it)"""
    s = _norm(seq)
    hits, u = 0, Counter()
    for p in range(len(s) - k + 1):
        w = s[p:p + k]
        if "N" in w:
            continue
        o = own.get(canonical_code(w))
        if o is None:
            continue
        hits += 1
        if o >= 0:
            u[o] += 1
    return hits, u


_tally_cache = {}


def oracle_assign(seqs, k, own, thr, n_rec):
    """-> (passes bool[n], assign u32[n], counts u64[n_rec + 2])"""
    key = (k, id(own), hash(tuple(seqs)))
    if key not in _tally_cache:
        _tally_cache[key] = [oracle_tally(s, k, own) for s in seqs]
    passes = np.zeros(len(seqs), bool)
    assign = np.full(len(seqs), NONE, np.uint32)
    for i, (hits, u) in enumerate(_tally_cache[key]):
        if hits < thr:
            continue
        passes[i] = True
        if not u:
            assign[i] = AMB
            continue
        m = max(u.values())
        win = [j for j, v in u.items() if v == m]
        assign[i] = win[0] if len(win) == 1 else AMB
    return passes, assign, counts_of(assign, n_rec)


def counts_of(assign, n_rec):
    c = np.zeros(n_rec + 2, np.uint64)
    for a in assign:
        c[n_rec + 1 if a == NONE else n_rec if a == AMB else a] += 1
    return c


@pytest.fixture(scope="module")
def bait8():
    return eight_record_bait()


_owner_cache = {}


def owners(text, k):
    key = (text, k)
    if key not in _owner_cache:
        _owner_cache[key] = oracle_owners(text, k)
    return _owner_cache[key]


def check_assign(mf, ol, ks, text, seqs, k, thr, mode, reads=None):
    """reads: the uploaded set of seqs, left open; without one the set is uploaded here and closed"""
    own_upload = reads is None
    if own_upload:
        R = ol.OracleReads.from_seqs(seqs)
        reads = mf.Reads.from_packed(R.words, R.offsets, R.npos)
    n_rec = len(read_fasta_records(text))
    passes, oassign, ocounts = oracle_assign(seqs, k, owners(text, k), thr, n_rec)
    fbits, _, _ = mf.filter_reads(ks, reads, thr, mode)
    bits, assign, counts = mf.assign_reads(ks, reads, thr, mode)
    if own_upload:
        reads.close()
    assert np.array_equal(bits, fbits)
    assert np.array_equal(bits_to_bool(bits, len(seqs)), passes)
    bad = np.nonzero(assign != oassign)[0]
    assert bad.size == 0, [(int(i), int(assign[i]), int(oassign[i])) for i in bad[:10]]
    assert np.array_equal(counts, ocounts), (counts, ocounts)
    assert int(counts.sum()) == len(seqs)
    return bits, assign, counts


# ------------------------------------------------------------------ 1. names
def test_record_names_and_count(mf):
    import ctypes as C
    text = ("ACGTACGTTTGACCAGTACGATCGATCGGA\n>alpha desc words\r\nACGTTGCAACGTTAGCAGCATTACGGACTAGGCA\r\n>empty\n>short\tdescribed\nACG\n"
            ">alpha\nTTTTGGGGCCCCAAAATTTTGGGGCCCCAAAA\n>gamma\r\nACGT\n>\n\nACGTAC\n")
    ks = mf.KmerSet.from_text(text, 21)
    assert ks.record_names == ["", "alpha", "empty", "short", "alpha", "gamma", ""]
    n = C.c_uint64()
    assert mf.load().mf_kmerset_record_count(ks._h, C.byref(n)) == 0 and n.value == 7
    need = C.c_size_t()
    assert mf.load().mf_kmerset_record_name(ks._h, 1, C.create_string_buffer(3), 3, C.byref(need)) == -1 and need.value == 6
    assert mf.load().mf_kmerset_record_name(ks._h, 7, C.create_string_buffer(16), 16, None) == -1
    ks.close()


# ------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize("k", [15, 21, 27, 31, 32, 33, 41, 63])
def test_assign_matches_oracle(mf, ol, bait8, k):
    ks = mf.KmerSet.from_text(bait8, k)
    assert len(ks.record_names) == 8
    for uniform in (True, False):
        seqs = make_reads(bait8, 1500, seed=700 + k, uniform=uniform, mito_frac=0.5)
        seqs = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(seqs)]
        for thr in (1, 3):
            for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                check_assign(mf, ol, ks, bait8, seqs, k, thr, mode)
    ks.close()


# ------------------------------------------------------------------ 3. screen forms
@pytest.mark.parametrize("form", [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (0, 1, 0), (2, 1, 0), (4, 1, 0), (0, 0, 1), (3, 1, 1)])
def test_screen_forms_give_the_same_assignment(mf, ol, bait8, form):
    front, canon, s8 = form
    k = 25 if s8 else 31
    seqs = make_reads(bait8, 1200, seed=41, mito_frac=0.5)
    ref = mf.KmerSet.from_text(bait8, k)
    R = ol.OracleReads.from_seqs(seqs)
    reads = mf.Reads.from_packed(R.words, R.offsets, R.npos)
    _, want, wcounts = mf.assign_reads(ref, reads, 1)
    try:
        mf.set_option("front", front)
        mf.set_option("canon", canon)
        mf.set_option("s8_finish", s8)
        ks = mf.KmerSet.from_text(bait8, k)
    finally:
        mf.set_option("front", -1)
        mf.set_option("canon", -1)
        mf.set_option("s8_finish", -1)
    _, got, gcounts = mf.assign_reads(ks, reads, 1)
    assert np.array_equal(got, want) and np.array_equal(gcounts, wcounts)
    check_assign(mf, ol, ks, bait8, seqs, k, 1, mf.MODE_SCREENED)
    ks.close(); ref.close(); reads.close()


# ------------------------------------------------------------------ 4. long and crowded reads
def crowded_bait_and_reads():
    rng = random.Random(77)
    recs = [("r%d" % j, "".join(rng.choices("ACGT", k=60 + (12 if j in (77, 5) else 0)))) for j in range(120)]
    longs = [("long%d" % j, "".join(rng.choices("ACGT", k=13000))) for j in range(2)]
    recs += longs + [("long0_copy", mutate(longs[0][1], 0.02, 9))]
    text = fasta(recs)
    body = [s for _, s in recs[:120]]
    reads = ["".join(b for j, b in enumerate(body) if j != 5),         # unique k-mers of 119 records; record 77 wins (beyond the 64 of a map)
             "".join(b for j, b in enumerate(body) if j != 77),        # ... record 5 wins
             "".join(body),                                            # records 5 and 77 tie: ambiguous
             revcomp("".join(b for j, b in enumerate(body[::-1]) if j != 119 - 5))]      # record 77 again, other strand
    return text, reads, [s for _, s in longs]


@pytest.mark.parametrize("L", [4096, 4097, 10000, 0])
def test_long_and_crowded_reads(mf, ol, L):
    text, crowded, longs = crowded_bait_and_reads()
    rng = random.Random(L)
    seqs = list(crowded)
    for i in range(40):
        n = L if L else rng.randint(100, 12000)
        src = longs[i % 2]
        p = rng.randrange(0, len(src) - n + 1)
        s = mutate(src[p:p + n], 0.01, i)
        seqs.append(revcomp(s) if i % 2 else s)
    if L:
        seqs = [s[:L].ljust(L, "A") if len(s) != L else s for s in seqs]
    ks = mf.KmerSet.from_text(text, 31)
    _, assign, _ = check_assign(mf, ol, ks, text, seqs, 31, 1, mf.MODE_SCREENED)
    if not L:
        assert list(assign[:4]) == [77, 5, AMB, 77]
    ks.close()


# ------------------------------------------------------------------ 5. one record
def test_single_record_bait(mf, ol):
    text = ">only\n" + bait_records(make_bait())[0] + "\n"
    ks = mf.KmerSet.from_text(text, 31)
    seqs = make_reads(text, 3000, seed=5)
    bits, assign, counts = check_assign(mf, ol, ks, text, seqs, 31, 1, mf.MODE_SCREENED)
    n_pass = int(bits_to_bool(bits, len(seqs)).sum())
    assert n_pass > 0 and list(counts) == [n_pass, 0, len(seqs) - n_pass]
    assert set(np.unique(assign)) <= {0, NONE}
    ks.close()


# ------------------------------------------------------------------ 6. state across calls
def test_state_across_calls(mf, ol, bait8):
    seqs = make_reads(bait8, 2000, seed=66, mito_frac=0.4)
    R = ol.OracleReads.from_seqs(seqs)
    reads = mf.Reads.from_packed(R.words, R.offsets, R.npos)
    n_rec = 8
    want = {k: oracle_assign(seqs, k, owners(bait8, k), 1, n_rec) for k in (63, 31)}
    ks = {k: mf.KmerSet.from_text(bait8, k) for k in (63, 31)}
    for _ in range(3):
        for k in (63, 31):
            bits, assign, counts = mf.assign_reads(ks[k], reads, 1)
            assert np.array_equal(assign, want[k][1]) and np.array_equal(counts, want[k][2])
            assert int(counts[:n_rec + 1].sum()) == int(bits_to_bool(bits, len(seqs)).sum())
            if k == 63:
                fbits, _, _ = mf.filter_reads(ks[31], reads, 1)
                assert np.array_equal(bits_to_bool(fbits, len(seqs)), want[31][0])
    reads.close()
    for v in ks.values():
        v.close()


# ------------------------------------------------------------------ 7. file level
def file_counts(seqs1, seqs2, k, text, thr, both):
    n_rec = len(read_fasta_records(text))
    p1, a1, _ = oracle_assign(seqs1, k, owners(text, k), thr, n_rec)
    if seqs2 is None:
        return int(p1.sum()), counts_of(a1[p1], n_rec)
    n = min(len(seqs1), len(seqs2))
    p2, a2, _ = oracle_assign(seqs2[:n], k, owners(text, k), thr, n_rec)
    keep = (p1[:n] & p2) if both else (p1[:n] | p2)
    return int(keep.sum()), counts_of(np.concatenate([a1[:n][keep], a2[keep]]), n_rec)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("pe,pair", [(False, 0), (True, 0), (True, 1)])
def test_files_by_record(mf, bait8, tmp_path, monkeypatch, path, gz, pe, pair):
    monkeypatch.setenv("MF_INGEST", path)
    s1 = make_reads(bait8, 2500, seed=91, mito_frac=0.3)
    s2 = make_reads(bait8, 2500, seed=92, mito_frac=0.3) if pe else None
    ext = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + ext)), (str(tmp_path / ("a_2" + ext)) if pe else None)
    write_fastq(fq1, s1, "a", gz=gz)
    if pe:
        write_fastq(fq2, s2, "b", gz=gz)
    ks = mf.KmerSet.from_text(bait8, 31)
    o = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "g1.fq", "g2.fq")]
    kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, o[0], o[1] if pe else None, 1, pair)
    kept, total, counts = mf.filter_fastq_files_by_record(ks, fq1, fq2, o[2], o[3] if pe else None, 1, pair)
    assert mf.last_ingest_stats()["path"] == (1 if path == "device" else 0)
    assert (kept, total) == (kept0, total0)
    assert open(o[2], "rb").read() == open(o[0], "rb").read()
    if pe:
        assert open(o[3], "rb").read() == open(o[1], "rb").read()
    okept, ocounts = file_counts(s1, s2, 31, bait8, 1, pair == 1)
    assert kept == okept
    assert np.array_equal(counts, ocounts), (counts, ocounts)
    assert int(counts.sum()) == kept * (2 if pe else 1)
    ks.close()


def test_files_by_record_two_devices(bait8, tmp_path):
    """n_devices = 2 on the library with the test hooks (MF_FAKE_DEVICES: two logical devices on the one GPU), device ingest path;
    a child process, because the variable is read when the library is loaded"""
    s1 = make_reads(bait8, 3000, seed=93)
    s2 = make_reads(bait8, 3000, seed=94)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(bait8)
    script = (
        "import json, sys\n"
        "from mitoflex_amd import mitofilter as mf\n"
        "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
        "a = mf.filter_fastq_files(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/o1.fq', sys.argv[4] + '/o2.fq', 1, 0, n_devices=2)\n"
        "b = mf.filter_fastq_files_by_record(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 0, n_devices=2)\n"
        "print(json.dumps({'a': list(a), 'kept': b[0], 'total': b[1], 'counts': [int(x) for x in b[2]], 'path': mf.last_ingest_stats()['path'],"
        " 'n_dev': mf.last_ingest_stats()['n_devices']}))\n")
    env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST="device", MF_GZDEV_CHUNK_BYTES="8192", MF_GZDEV_SLAB_CHUNKS="5",
               MF_GZDEV_TEXT_PIECE="200000", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert r["path"] == 1 and r["n_dev"] == 2
    assert r["a"] == [r["kept"], r["total"]]
    for m in ("1", "2"):
        assert open(str(tmp_path / ("g%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
    okept, ocounts = file_counts(s1, s2, 31, bait8, 1, False)
    assert r["kept"] == okept and r["counts"] == [int(x) for x in ocounts]


# ------------------------------------------------------------------ 8. CLI
def test_cli_report(mf, bait8, tmp_path):
    cli = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
    s1 = make_reads(bait8, 2000, seed=95)
    s2 = make_reads(bait8, 2000, seed=96)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(bait8)
    base = [cli, "bait", "--bait", bait, "-k", "31", "--fq1", fq1, "--fq2", fq2, "--pair", "both"]
    p0 = subprocess.run(base + ["--out1", str(tmp_path / "o1.fq"), "--out2", str(tmp_path / "o2.fq")], capture_output=True, timeout=300)
    assert p0.returncode == 0, p0.stderr.decode()[-2000:]
    rep = str(tmp_path / "report.tsv")
    p1 = subprocess.run(base + ["--out1", str(tmp_path / "g1.fq"), "--out2", str(tmp_path / "g2.fq"), "--report", rep], capture_output=True, timeout=300)
    assert p1.returncode == 0, p1.stderr.decode()[-2000:]
    assert p1.stdout == p0.stdout
    for m in ("1", "2"):
        assert open(str(tmp_path / ("g%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
    okept, oc = file_counts(s1, s2, 31, bait8, 1, True)
    assert int(p1.stdout.decode()) == okept
    names = ["mito", "mito_1pc", "mito_10pc", "mito_1pc_dup", "tiny", "rec2", "rec2_10pc", "rand"]
    want = "record\tname\treads\n" + "".join("%d\t%s\t%d\n" % (j, n, oc[j]) for j, n in enumerate(names))
    want += "-\t*ambiguous*\t%d\n-\t*unassigned*\t%d\n" % (oc[8], oc[9])
    assert open(rep).read() == want
    p2 = subprocess.run(base + ["--out1", str(tmp_path / "h1.fq"), "--out2", str(tmp_path / "h2.fq"), "--report"], capture_output=True, timeout=60)
    assert p2.returncode == 1
    p3 = subprocess.run(base + ["--out1", str(tmp_path / "h1.fq"), "--out2", str(tmp_path / "h2.fq"), "--protein", "--report", rep], capture_output=True, timeout=60)
    assert p3.returncode == 1 and b"--protein" in p3.stderr


# ------------------------------------------------------------------ 9. protein sets
def test_protein_sets_refused(mf, tmp_path):
    ptext = make_protein_bait()[0]
    ks = mf.KmerSet.protein_from_text(ptext, 9, 5)
    reads = mf.Reads.from_packed(np.zeros(16, np.uint32), np.array([0, 100], np.uint64), np.zeros(0, np.uint64))
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.assign_reads(ks, reads, 1)
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30], "a")
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.filter_fastq_files_by_record(ks, fq, None, str(tmp_path / "o.fq"), None)
    reads.close(); ks.close()
