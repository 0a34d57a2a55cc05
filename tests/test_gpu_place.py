"""Placement of the baited reads on the bait (mf_place, mf_filter_fastq_files_placed, `fastfilter bait --place-report / --base-depth`,
bim's device insert-size estimate) against the plain-Python oracle of tests/place_oracle.py, which is written from the semantics in
include/mitofilter.h: per-read placements, base depth, record summaries, the unplaced counts and the pass bitmap are all compared
exactly."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import place_oracle as po
from tests.report_data import fasta, mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_bim import _genome, _pairs
from tests.util_data import bait_records, bits_to_bool, make_bait, make_protein_bait, make_reads, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
FIELDS = ("record", "strand", "start", "end", "votes", "windows")
REC_FIELDS = ("forward", "reverse", "over_begin", "over_end", "covered", "base_sum")


# ------------------------------------------------------------------ data
def place_bait():
    """the shape of the depth tests' bait -- an anonymous leading record, invalid bases, records shorter than k, an empty record, a
    stretch repeated within a record, k-mers shared between records (one of them reverse-complemented) -- plus two records that lie next
    to each other (`left`, `right`) and a record holding a 32-base window that is its own reverse complement (`pal`)"""
    r = bait_records(make_bait())
    g = r[0][:3000]
    rng = random.Random(7)
    rnd = lambda n: "".join(rng.choices("ACGT", k=n))
    x, y = rnd(220), rnd(90)
    h = rnd(16)
    parts = {"g": g, "x": x, "left": rnd(600), "right": rnd(600), "pal": rnd(250) + h + revcomp(h) + rnd(250)}
    recs = [("mito desc", g), ("repeat", x + y + x + "acgtn" + y), ("empty", ""), ("tiny", "ACGTTGCA"),
            ("shared", revcomp(g[700:1300]) + g[2000:2400]), ("rec2", r[1][:1800]), ("rand", rnd(1200)),
            ("left", parts["left"]), ("right", parts["right"]), ("pal", parts["pal"])]
    return rnd(80) + "\n" + fasta(recs), parts


def scattered_read(g, k, seed, long_at):
    """70 segments of k bases from scattered places of g (outside what the `shared` record repeats), one of them k + 1 long, each on a
    diagonal of its own, with an N between two segments so that no window spans them: 70 candidates, exactly one with 2 votes"""
    rng = random.Random(seed)
    spots = [p for lo, hi in ((0, 640), (1360, 1940), (2460, 2940)) for p in range(lo, hi, 16)]
    rng.shuffle(spots)
    segs, diagonals, at = [], set(), 0
    for p in spots:
        if p - at in diagonals or len(segs) == 70:
            continue
        diagonals.add(p - at)
        segs.append(g[p:p + k + (len(segs) == long_at)])
        at += len(segs[-1]) + 1
    assert len(segs) == 70
    return "N".join(segs)


def special_reads(parts, k):
    g, x = parts["g"], parts["x"]
    rng = random.Random(31)
    rnd = lambda n: "".join(rng.choices("ACGT", k=n))
    seqs = {
        "over_begin": rnd(60) + g[:100],
        "over_end": revcomp(g[-90:] + rnd(60)),
        "over_both": rnd(30) + parts["left"] + rnd(30),
        "junction": parts["left"][-80:] + parts["right"][:70],
        "with_n": g[500:580] + "N" + g[581:650],
        "insertion": g[1400:1490] + "ACGTAC" + g[1490:1550],
        "tie": g[200:260] + "N" + g[1500:1560],
        "no_anchor": x[:150],
        "no_anchor_rc": revcomp(x[40:200]),
        "scattered_first": scattered_read(g, k, 1, 0),
        "scattered_last": revcomp(scattered_read(g, k, 2, 69)),
        "palindrome": parts["pal"][200:330],
    }
    return list(seqs), list(seqs.values())


def place_reads(text, parts, k, n, seed, uniform, read_len=150):
    seqs = make_reads(text, n, seed=seed, read_len=read_len, uniform=uniform, mito_frac=0.5)
    if uniform:
        return [], seqs
    names, special = special_reads(parts, k)
    return names, special + seqs


def rows_of(place):
    return np.stack([place[f].astype(np.int64) for f in FIELDS], axis=1)


def rec_rows(records):
    return np.stack([records[f] for f in REC_FIELDS], axis=1).astype(np.uint64)


def check(mf, ks, reads, o, tallies, thr, mode):
    passes, rows, depth, rec, unplaced = o.place(tallies, thr)
    bits, place, base_depth, records, unpl = mf.place_reads(ks, reads, thr, mode)
    assert np.array_equal(bits_to_bool(bits, len(tallies)), passes)
    fbits, _, _ = mf.filter_reads(ks, reads, thr, mode)
    assert np.array_equal(bits, fbits)
    got = rows_of(place)
    bad = np.nonzero((got != rows).any(axis=1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), rows[i].tolist()) for i in bad[:10]]
    bad = np.nonzero(base_depth.astype(np.int64) != np.minimum(depth, po.CLAMP))[0]
    assert bad.size == 0, [(int(i), int(base_depth[i]), int(depth[i])) for i in bad[:10]]
    assert np.array_equal(rec_rows(records), rec), (rec_rows(records), rec)
    assert unpl.tolist() == unplaced
    assert int(records["forward"].sum() + records["reverse"].sum()) + sum(unplaced) == len(tallies)
    return rows


# ------------------------------------------------------------------ 1. in memory
@pytest.mark.parametrize("k", [21, 31, 32, 41])
def test_place_matches_oracle(mf, ol, k):
    text, parts = place_bait()
    o = po.PlaceOracle(text, k)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    if k == 32:          # the set holds a window that is its own reverse complement, and it is no anchor
        pal = parts["pal"][250:282]
        assert pal == revcomp(pal) and pal in o.bait and pal not in o.anchors
    for uniform in (False, True):
        names, seqs = place_reads(text, parts, k, 1200, seed=500 + k, uniform=uniform)
        tallies = o.tally(seqs)
        reads = upload(mf, ol, seqs)
        for thr in (1, 3):
            results = [check(mf, ks, reads, o, tallies, thr, mode) for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE)]
            assert np.array_equal(results[0], results[1])
        reads.close()
        if uniform:
            continue
        # the reads that were built for a case are that case (at the last threshold, 3)
        rows = dict(zip(names, results[0]))
        votes = {n: tallies[i][1] for i, n in enumerate(names)}
        R = {n: j for j, n in enumerate(ks.record_names)}
        assert rows["over_begin"].tolist()[:4] == [R["mito"], 0, -60, 100]
        assert rows["over_end"].tolist()[:4] == [R["mito"], 1, 3000 - 90, 3000 + 60]
        assert rows["over_both"].tolist()[:4] == [R["left"], 0, -30, 630]
        assert rows["junction"].tolist()[:4] == [R["left"], 0, 520, 670] and len(votes["junction"]) == 2
        assert rows["with_n"].tolist()[:4] == [R["mito"], 0, 500, 650]
        assert rows["insertion"].tolist()[:4] == [R["mito"], 0, 1400, 1556] and len(votes["insertion"]) == 2
        assert rows["tie"][0] == po.AMBIGUOUS and rows["tie"][5] == 2 * (60 - k + 1)
        assert sorted(votes["tie"].values()) == [60 - k + 1] * 2
        for n in ("no_anchor", "no_anchor_rc"):
            assert rows[n].tolist() == [po.AMBIGUOUS, 0, 0, 0, 0, 0]
        for n in ("scattered_first", "scattered_last"):
            assert len(votes[n]) > 64 and sorted(votes[n].values())[-2:] == [1, 2]
            assert rows[n][0] == R["mito"] and rows[n][4] == 2 and rows[n][5] == len(votes[n]) + 1
        assert rows["scattered_last"][1] == 1
        assert rows["palindrome"][0] == R["pal"]
        if k == 32:          # every window of the read but the one that is its own reverse complement is an anchor window
            assert rows["palindrome"][5] == 130 - k + 1 - 1 and rows["palindrome"][4] == rows["palindrome"][5]
    ks.close()


def test_protein_set_is_refused(mf, ol):
    text = make_protein_bait()[0]
    ks = mf.KmerSet.protein_from_text(text, 9, 5)
    reads = upload(mf, ol, ["ACGT" * 40] * 4)
    with pytest.raises(mf.MitoFilterError, match="error -1"):
        mf.place_reads(ks, reads, 1)
    with pytest.raises(mf.MitoFilterError, match="error -1"):
        mf.filter_fastq_files_placed(ks, "a.fq", None, "o.fq", None)
    reads.close(); ks.close()


def test_stacked_reads(mf, ol):
    """many reads on one start (amplicon data): the same two difference counters and the same record counters take every add"""
    text, parts = place_bait()
    o = po.PlaceOracle(text, 31)
    ks = mf.KmerSet.from_text(text, 31)
    g = parts["g"]
    seqs = [g[300:450], revcomp(g[300:450])] * 1500 + [g[1400:1520]] * 500
    reads = upload(mf, ol, seqs)
    check(mf, ks, reads, o, o.tally(seqs), 1, mf.MODE_SCREENED)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 2. file level
@pytest.fixture(scope="module")
def nuc_files():
    text, parts = place_bait()
    _, s1 = place_reads(text, parts, 31, 900, seed=41, uniform=False)
    _, s2 = place_reads(text, parts, 31, 900, seed=42, uniform=False)
    s1, s2 = [s or "A" for s in s1], [s or "A" for s in s2]
    return text, s1, s2[:len(s1)]


def in_memory(mf, ol, ks, seqs, thr):
    reads = upload(mf, ol, seqs)
    _, _, depth, records, unplaced = mf.place_reads(ks, reads, thr)
    reads.close()
    return depth.astype(np.int64), rec_rows(records), unplaced


def summed(parts, starts):
    depth = sum(p[0] for p in parts)
    rec = sum(p[1] for p in parts)
    for j in range(len(starts) - 1):
        rec[j, 4] = int((depth[int(starts[j]):int(starts[j + 1])] > 0).sum())          # (covered does not add)
    return depth, rec, sum(p[2] for p in parts)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_placed_equals_the_mates_in_memory(mf, ol, nuc_files, tmp_path, monkeypatch, ingest):
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
    out = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    for thr in (1, 3):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, out[0], out[1], thr, mf.PAIR_BOTH)
        kept, total, depth, records, unplaced = mf.filter_fastq_files_placed(ks, fq1, fq2, out[2], out[3], thr, mf.PAIR_BOTH)
        assert mf.last_ingest_stats()["path"] == (1 if gz else 0)
        assert (kept, total) == (kept0, total0)
        assert md5(out[2]) == md5(out[0]) and md5(out[3]) == md5(out[1])
        wdepth, wrec, wunpl = summed([in_memory(mf, ol, ks, s, thr) for s in (s1, s2)], ks.record_starts)
        assert np.array_equal(depth.astype(np.int64), wdepth)
        assert np.array_equal(rec_rows(records), wrec)
        assert unplaced.tolist() == wunpl.tolist()
    ks.close()


def test_files_placed_two_devices(mf, ol, nuc_files, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), on both ingest paths, in a child process"""
    text, s1, s2 = nuc_files
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    ks = mf.KmerSet.from_text(text, 31)
    wdepth, wrec, wunpl = summed([in_memory(mf, ol, ks, s, 1) for s in (s1, s2)], ks.record_starts)
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
            "b = mf.filter_fastq_files_placed(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 1, devices=[0, 1])\n"
            "print(json.dumps({'a': list(a), 'kept': b[0], 'total': b[1], 'depth': [int(x) for x in b[2]],"
            " 'records': [[int(v) for v in r] for r in b[3]], 'unplaced': [int(x) for x in b[4]],"
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
        assert np.array_equal(np.array(r["depth"], np.int64), wdepth)
        assert np.array_equal(np.array(r["records"], np.uint64), wrec)
        assert r["unplaced"] == wunpl.tolist()


# ------------------------------------------------------------------ 3. CLI
def test_cli_place_report_and_base_depth(mf, ol, nuc_files, tmp_path):
    text, s1, s2 = nuc_files
    ks = mf.KmerSet.from_text(text, 31)
    starts, names = ks.record_starts, ks.record_names
    dev0 = [0]
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    kept, _, depth, records, unplaced = mf.filter_fastq_files_placed(ks, fq1, fq2, str(tmp_path / "l1.fq"), str(tmp_path / "l2.fq"), 1, mf.PAIR_EITHER,
                                                                      devices=dev0)
    ks.close()
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    base = [CLI, "bait", "--bait", bait, "--fq1", fq1, "--fq2", fq2, "-k", "31"]
    rep, dep = str(tmp_path / "place.tsv"), str(tmp_path / "base.tsv")
    p1 = subprocess.run(base + ["--out1", str(tmp_path / "d1.fq"), "--out2", str(tmp_path / "d2.fq"), "--place-report", rep, "--base-depth", dep],
                        capture_output=True, timeout=300)
    assert p1.returncode == 0, p1.stderr.decode()[-2000:]
    assert p1.stdout.decode().split() == [str(kept)]
    for m in ("1", "2"):
        assert md5(str(tmp_path / ("d%s.fq" % m))) == md5(str(tmp_path / ("l%s.fq" % m)))
    lines = [ln.split("\t") for ln in open(rep).read().splitlines()]
    assert lines[0] == ["record", "name", "length", "forward", "reverse", "over_begin", "over_end", "covered", "mean", "max"]
    assert lines[-1] == ["-", "*unplaced*", str(int(unplaced[0]))]
    assert len(lines) == len(names) + 2
    for j, ln in enumerate(lines[1:-1]):
        d = depth[int(starts[j]):int(starts[j + 1])]
        length = int(starts[j + 1] - starts[j])
        assert ln[:3] == [str(j), names[j], str(length)]
        assert [int(v) for v in ln[3:8]] == [int(records[f][j]) for f in REC_FIELDS[:5]]
        assert ln[8] == "%.3f" % (int(records["base_sum"][j]) / length if length else 0.0)
        assert int(ln[9]) == (int(d.max()) if d.size else 0)
    want = "".join("%s\t%d\t%d\n" % (names[j], p - int(starts[j]) + 1, depth[p])
                   for j in range(len(names)) for p in range(int(starts[j]), int(starts[j + 1])))
    assert open(dep).read() == want
    # either flag alone
    p2 = subprocess.run(base + ["--out1", str(tmp_path / "e1.fq"), "--out2", str(tmp_path / "e2.fq"), "--base-depth", str(tmp_path / "b2.tsv")],
                        capture_output=True, timeout=300)
    assert p2.returncode == 0 and open(str(tmp_path / "b2.tsv")).read() == want
    p3 = subprocess.run(base + ["--out1", str(tmp_path / "f1.fq"), "--out2", str(tmp_path / "f2.fq"), "--place-report", str(tmp_path / "r3.tsv")],
                        capture_output=True, timeout=300)
    assert p3.returncode == 0 and open(str(tmp_path / "r3.tsv")).read() == open(rep).read()


# ------------------------------------------------------------------ 4. bim
def test_bim_device_insert_sizes(mf, tmp_path):
    """simulated pairs without indels: the device estimate is within 1.5 bases of the truth (the bar DESIGN.md 9 #1 records for the host
    estimate), the per-pair sizes are those of the oracle's placements, and kmer_bait_map(anchors="device") writes IS lines cal_insert reads"""
    from mitoflex_amd.bim import bim
    g = _genome()
    text = ">g\n" + "\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + "\n>other\n" + _genome(900, 5) + "\n"
    fa = str(tmp_path / "bait.fa")
    open(fa, "w").write(text)
    m1, m2, frags = _pairs(g, 3000, 1)
    fq1, fq2 = str(tmp_path / "k.1.fq"), str(tmp_path / "k.2.fq")
    write_fastq(fq1, m1, "a")
    write_fastq(fq2, m2, "b")
    sizes = bim.pair_insert_sizes_device(fa, fq1, fq2, 31)
    o = po.PlaceOracle(text, 31)
    want = po.inserts(o.place(o.tally(m1), 1)[1], o.place(o.tally(m2), 1)[1])
    assert np.array_equal(sizes, want)
    hist = bim.estimate_insert_sizes_device(fa, fq1, fq2, 31)
    assert sum(hist.values()) == int((want > 0).sum()) > 0.97 * len(m1)
    truth = sum(s for _, s in frags) / len(frags)
    est = sum(a * b for a, b in hist.items()) / sum(hist.values())
    print("device insert-size estimate %.3f, truth %.3f, pairs %d" % (est, truth, sum(hist.values())))
    assert abs(est - truth) < 1.5
    assert bim.estimate_insert_sizes_device(fa, fq1, fq2, 31, max_pairs=100) == {
        int(s): int(c) for s, c in zip(*np.unique(want[:100][want[:100] > 0], return_counts=True))}
    # the whole step: bait with the filter, then IS lines from the device placements of the kept pairs
    stats, k1, k2 = bim.kmer_bait_map(1, fa, str(tmp_path), "gen0", fq1, fq2, anchors="device")
    assert any(ln.startswith("IS\t") for ln in open(stats))
    kept_hist = bim.estimate_insert_sizes_device(fa, k1, k2, 31)
    assert bim.cal_insert(stats, str(tmp_path), "gen0") == pytest.approx(sum(a * b for a, b in kept_hist.items()) / sum(kept_hist.values()))
    assert abs(bim.cal_insert(stats, str(tmp_path), "gen0") - truth) < 1.5
