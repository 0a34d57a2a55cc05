"""The keep rule (include/mitofilter.h, "which mates are written"): mf_verify_keep, mf_filter_fastq_files_verified_keep, `fastfilter
bait --write`, bim.kmer_bait_map(keep=..).  The expected bits come from tests/verify_oracle.VerifyOracle.verify (plain Python over
strings): placed = rows[:, 0] < AMBIGUOUS; accepted mode = passes & ~(placed & ~accepted); placed mode = passes & placed & accepted.
There is no tolerance anywhere."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import place_oracle as po
from tests import verify_oracle as vo
from tests.report_data import mf, mutate, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_place import place_bait, place_reads, special_reads
from tests.test_gpu_verify import drawn, md5, nuc_files, numt_data, substituted  # noqa: F401  (nuc_files: fixture)
from tests.util_data import bits_to_bool, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
REPORTS = ("base_depth", "place_records", "pileup", "consensus", "pileup_records", "score_records", "unplaced")
MODES = (0, 1, 2)          # KEEP_PASSING, KEEP_ACCEPTED, KEEP_PLACED


def oracle_bits(want, keep):
    """the keep bits of every read from what VerifyOracle.verify gave"""
    placed = want["rows"][:, 0] < po.AMBIGUOUS
    if keep == 1:
        return want["passes"] & ~(placed & ~want["accepted"])
    if keep == 2:
        return want["passes"] & placed & want["accepted"]
    return want["passes"].copy()


def words_of(bits):
    """bool[n] -> the u32 words of the bitmap, tail bits 0"""
    b = np.zeros((len(bits) + 31) // 32 * 32, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint32)


def verify_keep(mf, ks, reads, thr, mode, min_depth, max_permille, keep):
    """verify_reads with a keep mode; KEEP_PASSING, which the wrapper serves with mf_verify, goes to mf_verify_keep itself here"""
    if keep != mf.KEEP_PASSING:
        return mf.verify_reads(ks, reads, thr, mode, min_depth, max_permille, keep=keep)
    per_read, read_results = mf._read_outputs(reads, mf.PLACE, mf.SCORE)
    ptrs, results = mf._report_outputs(ks, mf._VERIFY_FIELDS)
    n = reads.info.n_reads
    keep_bits = np.full(max((n + 31) // 32, 1), 0xDEADBEEF, np.uint32)
    mf._chk(mf.load().mf_verify_keep(ks._h, reads._h, thr, mode, min_depth, max_permille, keep, per_read[0], keep_bits.ctypes.data,
                                     *per_read[1:], *ptrs, None))
    bits, place, score = read_results()
    return mf.VerifiedKeep(bits=bits, keep_bits=keep_bits[:(n + 31) // 32], place=place, score=score, **results())


def same_but_keep_bits(v, base):
    """every output of a call with a keep mode is, bit for bit, the call's without"""
    for f in ("bits", "place", "score") + REPORTS:
        a, b = getattr(v, f), getattr(base, f)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f


def check_keep_bits(v, want, keep, n):
    words = words_of(oracle_bits(want, keep))
    assert v.keep_bits.dtype == np.uint32 and len(v.keep_bits) == (n + 31) // 32
    bad = np.nonzero(bits_to_bool(v.keep_bits, n) != oracle_bits(want, keep))[0]
    assert bad.size == 0, (keep, [(int(i), want["rows"][i].tolist(), want["scores"][i].tolist()) for i in bad[:10]])
    assert np.array_equal(v.keep_bits, words)          # (the tail bits of the last word are 0)
    if n % 32:
        assert int(v.keep_bits[-1]) >> (n % 32) == 0


# ------------------------------------------------------------------ 1. resident parity
@pytest.mark.parametrize("k", [21, 31, 41])
def test_keep_bits_match_oracle(mf, ol, k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    V = vo.VerifyOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    for uniform in (False, True):
        _, seqs = place_reads(text, parts, k, 1200, seed=1300 + k, uniform=uniform)
        seqs = seqs + drawn(mutate(parts["g"], 0.01, 77), 200, seed=79, lo=150 if uniform else 100)
        n = len(seqs)
        assert n % 32
        tallies = o.tally(seqs)
        reads = upload(mf, ol, seqs)
        cleared = {}
        for thr in (1, 3):
            for max_permille in (1000, 20, 0):
                want = V.verify(seqs, tallies, thr, max_permille)
                base = mf.verify_reads(ks, reads, thr, mf.MODE_SCREENED, 2, max_permille)
                assert type(base) is mf.Verified and base.keep_bits is None and np.array_equal(bits_to_bool(base.bits, n), want["passes"])
                for keep in MODES:
                    v = verify_keep(mf, ks, reads, thr, mf.MODE_SCREENED, 2, max_permille, keep)
                    same_but_keep_bits(v, base)
                    check_keep_bits(v, want, keep, n)
                    if keep == mf.KEEP_PASSING:
                        assert np.array_equal(v.keep_bits, v.bits)
                    cleared[(thr, max_permille, keep)] = int(want["passes"].sum()) - int(oracle_bits(want, keep).sum())
        # the data tell the modes apart: nothing is rejected at 1000, the cut clears more the tighter it is, and `placed` clears more
        assert cleared[(1, 1000, 1)] == 0 < cleared[(1, 20, 1)] < cleared[(1, 0, 1)]
        assert 0 < cleared[(1, 1000, 2)] and all(cleared[(1, c, 1)] < cleared[(1, c, 2)] for c in (1000, 20, 0))
        # the pileup=False instantiation writes the same bits
        w = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 2, 20, pileup=False, keep=mf.KEEP_PLACED)
        check_keep_bits(w, V.verify(seqs, tallies, 1, 20), 2, n)
        assert w.pileup is None
        reads.close()
    ks.close()


def test_keep_outside_the_modes_is_refused(mf, ol):
    text, _ = place_bait()
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, ["ACGT" * 20])
    for keep in (-1, 3):
        with pytest.raises(ValueError):
            mf.verify_reads(ks, reads, keep=keep)
        rc = mf.load().mf_verify_keep(ks._h, reads._h, 1, mf.MODE_SCREENED, 1, 1000, keep, *([None] * 12))
        assert rc != 0 and "keep" in mf.load().mf_last_error().decode()
    reads.close(); ks.close()


# ------------------------------------------------------------------ 2. word edges
def test_word_edges(mf, ol):
    """every read passes and is placed; exactly the listed ones are reads of the diverged copy, which a cut of 30 rejects
    (test_numt_reads_are_cut_and_the_consensus_is_the_bait_s): bits 0 and 31 of a word, a whole word, the last read, one read, 33"""
    g, _, clean, copies = numt_data()
    text = ">g\n" + g + "\n"
    V = vo.VerifyOracle(po.PlaceOracle(text, 21))
    ks = mf.KmerSet.from_text(text, 21)
    cases = (
        (70, {0, 31, 32, 63, 64, 69}, [0x7FFFFFFE, 0x7FFFFFFE, 0x0000001E]),
        (96, set(range(32, 64)), [0xFFFFFFFF, 0x00000000, 0xFFFFFFFF]),
        (1, {0}, [0x00000000]),
        (33, {0, 32}, [0xFFFFFFFE, 0x00000000]),
        (33, {31}, [0x7FFFFFFF, 0x00000001]),
    )
    for n, rejected, words in cases:
        seqs = [copies[i] if i in rejected else clean[i] for i in range(n)]
        want = V.verify(seqs, V.o.tally(seqs), 1, 30)
        assert want["passes"].all() and (want["rows"][:, 0] == 0).all() and np.nonzero(~want["accepted"])[0].tolist() == sorted(rejected)
        reads = upload(mf, ol, seqs)
        for keep in (mf.KEEP_ACCEPTED, mf.KEEP_PLACED):
            v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 1, 30, keep=keep)
            assert v.keep_bits.tolist() == words, (n, keep, [hex(int(x)) for x in v.keep_bits])
            assert words_of(oracle_bits(want, keep)).tolist() == words
            assert v.bits.tolist() == words_of(np.ones(n, bool)).tolist()
            assert int(v.score_records["rejected"][0]) == len(rejected)
        reads.close()
    ks.close()


# ------------------------------------------------------------------ 3. several reads a wave
SIX = ("forward", "reverse", "rejected", "ambiguous", "no_anchor", "not_passing")


def six_reads():
    """(bait text, k, the six reads, their expected bits under KEEP_ACCEPTED and KEEP_PLACED at a cut of 30)"""
    text, parts = place_bait()
    g = parts["g"]
    names, special = special_reads(parts, 31)
    rng = random.Random(3)
    seqs = [g[300:450], revcomp(g[1600:1750]), substituted(g[300:450], range(5, 55, 5)), special[names.index("tie")],
            special[names.index("no_anchor")], "".join(rng.choices("ACGT", k=150))]
    return text, 31, seqs, {1: [1, 1, 0, 1, 1, 0], 2: [1, 1, 0, 0, 0, 0]}


def test_several_reads_a_wave(mf, ol):
    """place_kernel launches at most 32 waves a CU, so below 8 192 reads a wave sees one read: 4 096 copies of each of six reads in
    blocks give every wave several reads, of one kind and, where the blocks meet, of two"""
    text, k, six, bits = six_reads()
    V = vo.VerifyOracle(po.PlaceOracle(text, k))
    want = V.verify(six, V.o.tally(six), 1, 30)
    assert want["passes"].tolist() == [True] * 5 + [False]
    assert (want["rows"][:, 0] < po.AMBIGUOUS).tolist() == [True, True, True, False, False, False]
    assert want["rows"][:3, 1].tolist() == [0, 1, 0] and want["accepted"].tolist() == [True, True, False, False, False, False]
    for keep in (1, 2):
        assert oracle_bits(want, keep).tolist() == [bool(b) for b in bits[keep]]
    copies = 4096
    seqs = [s for s in six for _ in range(copies)]
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    for keep in (mf.KEEP_ACCEPTED, mf.KEEP_PLACED):
        v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 1, 30, pileup=False, keep=keep)
        assert np.array_equal(v.keep_bits, words_of(np.repeat(np.array(bits[keep], bool), copies))), keep
        assert np.array_equal(v.bits, words_of(np.repeat(want["passes"], copies)))
        assert int(v.score_records["rejected"].sum()) == copies and int(v.unplaced[0]) == 2 * copies
    reads.close(); ks.close()


# ------------------------------------------------------------------ 4. files, both ingest paths
def fastq_records(path):
    """the records of a FASTQ file written by write_fastq, as the library writes them (a bare '+' line)"""
    lines = open(path, "rb").read().split(b"\n")
    return [lines[i] + b"\n" + lines[i + 1] + b"\n+\n" + lines[i + 3] + b"\n" for i in range(0, len(lines) - 1, 4)]


@pytest.fixture(scope="module")
def file_oracle(nuc_files):
    """the oracle's verdict on both mates of nuc_files at thr 1, cut 20, once for every test below"""
    text, s1, s2 = nuc_files
    V = vo.VerifyOracle(po.PlaceOracle(text, 31))
    want = [V.verify(s, V.o.tally(s), 1, 20) for s in (s1, s2)]
    bits = {keep: [oracle_bits(w, keep) for w in want] for keep in MODES}
    return want, bits


def pair_rule(bits, both):
    return (bits[0] & bits[1]) if both else (bits[0] | bits[1])


def test_the_oracle_s_figures_for_the_files(nuc_files, file_oracle):
    """what the file tests stand on, from the oracle alone: the three modes differ under both pair rules, and under `either` some pair
    is written through one mate only"""
    _, s1, s2 = nuc_files
    want, bits = file_oracle
    assert len(s1) == len(s2) == 962
    assert [[int(b.sum()) for b in bits[keep]] for keep in MODES] == [[360, 387], [294, 312], [217, 230]]
    assert [int((w["passes"] & (w["rows"][:, 0] < po.AMBIGUOUS) & ~w["accepted"]).sum()) for w in want] == [66, 75]
    assert [int((w["passes"] & (w["rows"][:, 0] >= po.AMBIGUOUS)).sum()) for w in want] == [77, 82]
    assert [int(pair_rule(bits[keep], False).sum()) for keep in MODES] == [542, 499, 399]
    assert [int(pair_rule(bits[keep], True).sum()) for keep in MODES] == [205, 107, 48]
    for keep in MODES:
        assert int((bits[keep][0] ^ bits[keep][1]).sum()) > 0          # a pair written through one mate only


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_hold_what_the_keep_rule_selects(mf, ol, nuc_files, file_oracle, tmp_path, monkeypatch, ingest):
    text, s1, s2 = nuc_files
    want, bits = file_oracle
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
    plain = [str(tmp_path / "p_1.fq"), str(tmp_path / "p_2.fq")]
    write_fastq(plain[0], s1, "a")
    write_fastq(plain[1], s2, "b")
    recs = [fastq_records(p) for p in plain]
    ks = mf.KmerSet.from_text(text, 31)
    out = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    path = 1 if gz else 0
    for pair_mode, both in ((mf.PAIR_EITHER, False), (mf.PAIR_BOTH, True)):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, out[0], out[1], 1, pair_mode)
        base = mf.filter_fastq_files_verified(ks, fq1, fq2, out[2], out[3], 1, pair_mode, max_permille=20)
        assert (base.kept, base.total) == (kept0, total0) == (int(pair_rule(bits[0], both).sum()), 962)
        for keep in MODES:
            if keep == mf.KEEP_PASSING:          # (the wrapper serves it with the older call: the new one itself)
                ptrs, results = mf._report_outputs(ks, mf._VERIFY_FIELDS)
                kept, total = mf._files_call("mf_filter_fastq_files_verified_keep", ks, fq1, fq2, out[2], out[3], 1, pair_mode, None, 1, 1, 20, keep, *ptrs)
                v = mf.Verified(kept=kept, total=total, **results())
            else:
                v = mf.filter_fastq_files_verified(ks, fq1, fq2, out[2], out[3], 1, pair_mode, max_permille=20, keep=keep)
            assert mf.last_ingest_stats()["path"] == path
            sel = pair_rule(bits[keep], both)
            assert (v.kept, v.total) == (int(sel.sum()), 962), (pair_mode, keep)
            for m in (0, 1):
                assert open(out[2 + m], "rb").read() == b"".join(r for r, s in zip(recs[m], sel) if s), (pair_mode, keep, m)
            if keep == mf.KEEP_PASSING:
                assert md5(out[2]) == md5(out[0]) and md5(out[3]) == md5(out[1])
            for f in REPORTS:          # what the reports count does not depend on the keep mode
                assert np.array_equal(getattr(v, f), getattr(base, f)), (pair_mode, keep, f)
    # single end, mate 1 alone, and the header's two identities
    kept0, total0 = mf.filter_fastq_files(ks, fq1, None, out[0], None, 1)
    assert (kept0, total0) == (360, 962)
    for keep in MODES[1:]:
        v = mf.filter_fastq_files_verified(ks, fq1, None, out[2], None, 1, max_permille=20, keep=keep)
        assert mf.last_ingest_stats()["path"] == path
        assert (v.kept, v.total) == (int(bits[keep][0].sum()), 962)
        assert open(out[2], "rb").read() == b"".join(r for r, s in zip(recs[0], bits[keep][0]) if s), keep
        passing = v.total - int(v.unplaced[1])
        if keep == mf.KEEP_ACCEPTED:
            assert v.kept == passing - int(v.score_records["rejected"].sum()) == 294
        else:
            assert v.kept == int(v.score_records["accepted"].sum()) == 217
    ks.close()


# ------------------------------------------------------------------ 5. two logical devices
def test_files_keep_two_devices(mf, nuc_files, file_oracle, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), on both ingest paths, in a child process:
    KEEP_ACCEPTED / PAIR_EITHER writes what one device writes"""
    text, s1, s2 = nuc_files
    _, bits = file_oracle
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    sel = pair_rule(bits[1], False)
    for gz, ingest in ((True, "device"), (False, "host")):
        ext = ".fq.gz" if gz else ".fq"
        fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
        write_fastq(fq1, s1, "a", gz=gz)
        write_fastq(fq2, s2, "b", gz=gz)
        script = (
            "import json, sys\n"
            "from mitoflex_amd import mitofilter as mf\n"
            "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
            "out = {}\n"
            "for tag, devices in (('one', [0]), ('two', [0, 1])):\n"
            "    v = mf.filter_fastq_files_verified(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/' + tag + '1.fq', sys.argv[4] + '/' + tag + '2.fq', 1,"
            " mf.PAIR_EITHER, devices=devices, max_permille=20, pileup=False, keep=mf.KEEP_ACCEPTED)\n"
            "    st = mf.last_ingest_stats()\n"
            "    out[tag] = {'kept': v.kept, 'total': v.total, 'rejected': int(v.score_records['rejected'].sum()), 'path': st['path'], 'n_dev': st['n_devices']}\n"
            "print(json.dumps(out))\n")
        env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_GZDEV_CHUNK_BYTES="8192",
                   MF_GZDEV_SLAB_CHUNKS="5", MF_GZDEV_TEXT_PIECE="100000", MF_BATCH_READS="400", PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert r["one"]["n_dev"] == 1 and r["two"]["n_dev"] == 2 and r["one"]["path"] == r["two"]["path"] == (1 if ingest == "device" else 0)
        assert r["one"]["kept"] == r["two"]["kept"] == int(sel.sum()) and r["one"]["total"] == r["two"]["total"] == 962
        assert r["one"]["rejected"] == r["two"]["rejected"] == 66 + 75
        for m in ("1", "2"):
            assert md5(str(tmp_path / ("two%s.fq" % m))) == md5(str(tmp_path / ("one%s.fq" % m)))


# ------------------------------------------------------------------ 6. CLI
def test_cli_write(mf, nuc_files, tmp_path):
    text, s1, s2 = nuc_files
    ks = mf.KmerSet.from_text(text, 31)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    t = lambda n: str(tmp_path / n)
    lib = {"passing": mf.filter_fastq_files(ks, fq1, fq2, t("passing1.fq"), t("passing2.fq"), 1, mf.PAIR_EITHER)[0],
           "accepted": mf.filter_fastq_files_verified(ks, fq1, fq2, t("accepted1.fq"), t("accepted2.fq"), 1, mf.PAIR_EITHER, max_permille=20,
                                                      keep=mf.KEEP_ACCEPTED).kept,
           "placed": mf.filter_fastq_files_verified(ks, fq1, fq2, t("placed1.fq"), t("placed2.fq"), 1, mf.PAIR_EITHER, keep=mf.KEEP_PLACED).kept}
    ks.close()
    assert lib["passing"] > lib["accepted"] > lib["placed"] > 0
    bait = t("bait.fa")
    open(bait, "w").write(text)
    base = [CLI, "bait", "--bait", bait, "--fq1", fq1, "--fq2", fq2, "-k", "31"]

    def run(tag, extra, same_as):
        p = subprocess.run(base + ["--out1", t(tag + "1.fq"), "--out2", t(tag + "2.fq")] + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert p.stdout.decode().split() == [str(lib[same_as])], (tag, p.stdout)
        for m in ("1", "2"):
            assert md5(t(tag + m + ".fq")) == md5(t(same_as + m + ".fq")), (tag, m)

    run("a", ["--write", "accepted", "--max-mismatch", "20"], "accepted")
    run("b", ["--write", "placed"], "placed")
    run("c", ["--write", "passing"], "passing")
    run("d", [], "passing")
    run("e", ["--write", "accepted", "--max-mismatch", "20", "--score-report", t("s.tsv"), "--place-report", t("p.tsv")], "accepted")
    run("f", ["--max-mismatch", "20", "--score-report", t("s0.tsv"), "--place-report", t("p0.tsv")], "passing")
    assert md5(t("s.tsv")) == md5(t("s0.tsv")) and md5(t("p.tsv")) == md5(t("p0.tsv"))          # the reports do not depend on it
    for extra in (["--write", "accepted", "--report", t("r.tsv")], ["--write", "placed", "--group-report", t("r.tsv")],
                  ["--write", "accepted", "--depth-report", t("r.tsv")], ["--write", "placed", "--depth-profile", t("r.tsv")],
                  ["--write", "accepted", "--protein"], ["--write", "rejected"], ["--write"]):
        p = subprocess.run(base + ["--out1", t("x1.fq"), "--out2", t("x2.fq")] + extra, capture_output=True, timeout=60)
        assert p.returncode != 0 and p.stdout == b"" and b"error" in p.stderr, extra


# ------------------------------------------------------------------ 7. bim
def test_bim_kmer_bait_map_keeps_the_diverged_copy_out(mf, tmp_path):
    """on the NUMT case (every read passes and is placed; a cut of 30 rejects exactly the copy's reads) the bait step writes the clean
    reads alone; without the arguments its files are today's"""
    from mitoflex_amd.bim import bim
    g, _, clean, copies = numt_data()
    fa, fq = str(tmp_path / "bait.fa"), str(tmp_path / "k.fq")
    open(fa, "w").write(">g\n" + g + "\n")
    seqs = [s for pair in zip(clean, copies) for s in pair] + clean[len(copies):]          # interleaved
    is_copy = [i < 2 * len(copies) and i % 2 == 1 for i in range(len(seqs))]
    write_fastq(fq, seqs, "a")
    recs = fastq_records(fq)
    _, all1, _ = bim.kmer_bait_map(1, fa, str(tmp_path), "all", fq, None, kmer=21)
    _, def1, _ = bim.kmer_bait_map(1, fa, str(tmp_path), "def", fq, None, kmer=21, max_permille=None, keep=None)
    _, cut1, _ = bim.kmer_bait_map(1, fa, str(tmp_path), "cut", fq, None, kmer=21, max_permille=30, keep=mf.KEEP_ACCEPTED)
    assert open(all1, "rb").read() == b"".join(recs) and md5(def1) == md5(all1)
    assert open(cut1, "rb").read() == b"".join(r for r, c in zip(recs, is_copy) if not c)
