"""The extended records (mf_align_extended, mf_filter_fastq_files_extended) against the plain-Python oracle of tests/extend_oracle.py,
which is written from the rule in include/mitofilter.h: the extension pile, the extended records, their offsets and their summaries are
compared exactly, and every output the gapped call gives is held to that call bit for bit.  There is no tolerance anywhere.
tests/test_extend_data.py holds the inputs to their conditions without a device."""
import filecmp
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import align_data as ad
from tests import extend_data as xd
from tests import extend_oracle as xo
from tests import extend_text
from tests import place_oracle as po
from tests.report_data import mf, ol, upload  # noqa: F401  (fixtures)
from tests.test_gpu_keep import HOOKS_LIB
from tests.util_data import write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")

OLD = ("bits", "keep_bits", "place", "align", "base_depth", "place_records", "pileup", "consensus", "pileup_records", "indels", "align_records", "unplaced",
       "ins_pile", "gapped", "gapped_starts", "gapped_records")
NEW = ("ext_pile", "extended", "extended_starts", "extend_records")
EXT_REC = ("length", "begin_bases", "end_bases", "begin_piled", "end_piled")
ES = (1, 16, 64, 4096)
GZDEV = {"MF_GZDEV_CHUNK_BYTES": "8192", "MF_GZDEV_SLAB_CHUNKS": "5", "MF_GZDEV_TEXT_PIECE": "100000"}
COPIES = 256


@functools.lru_cache(maxsize=None)
def placement(k):
    """the placement oracle of the `ends` bait for k: computed once, shared, left unchanged"""
    return po.PlaceOracle(xd.ends_bait()[0], k)


@functools.lru_cache(maxsize=None)
def ends_want(k, band, uniform=None, seed=79):
    """the oracle's run on an `ends` read set, its insertion pile and its extension pile at the largest E (a smaller E is its first columns)"""
    o = placement(k)
    X = xo.ExtendOracle(o)
    seqs, _ = xd.ends_reads(seed=seed, uniform=uniform)
    want = X.A.run(seqs, o.tally(seqs), 1, xd.CUT, band)
    return X, seqs, want, X.G.pile(seqs, want, band), X.pile(seqs, want, band, max(ES))


def ext_table(ext_pile):
    return np.stack([ext_pile[f].astype(np.int64) for f in "acgt"], axis=3)


def check_extended(a, X, want, ins, ext, min_depth, E):
    """the four new outputs of one call against the oracle's sums; ext: int[R, 2, E, 4]"""
    got = ext_table(a.ext_pile)
    assert got.shape == ext.shape == (len(X.o.recs), 2, E, 4) and np.array_equal(got, xo.clamped(ext)), np.argwhere(got != ext)[:8].tolist()
    extended, xstarts, xrecs = X.call(want, ins, ext, min_depth)
    assert a.extended_starts.tolist() == xstarts
    assert bytes(a.extended) == extended
    assert [[int(a.extend_records[f][j]) for f in EXT_REC] for j in range(len(xrecs))] == xrecs
    assert np.array_equal(np.diff(a.extended_starts.astype(np.int64)), a.extend_records["length"].astype(np.int64))
    if "rows" in want:          # the invariant: at most as many bases as accepted reads reach the column
        assert (got.sum(axis=3) <= xo.overhang_bounds(X.o, want, E)).all()


# ------------------------------------------------------------------ 1. the older outputs are unchanged
@pytest.mark.parametrize("max_permille", [30, 1000])
def test_old_outputs_are_unchanged(mf, ol, max_permille):
    text = xd.ends_bait()[0]
    seqs, _ = xd.ends_reads()
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for band in (8, 0):
        g = mf.align_reads(ks, reads, band, 2, max_permille, mf.KEEP_ACCEPTED, gapped=True)
        z = mf.align_reads(ks, reads, band, 2, max_permille, mf.KEEP_ACCEPTED, extend=0, gapped=True)
        assert all(getattr(g, f) is None for f in NEW) and all(getattr(z, f) is None for f in NEW)
        for E in (1, 64, 4096):
            x = mf.align_reads(ks, reads, band, 2, max_permille, mf.KEEP_ACCEPTED, extend=E, gapped=True)
            for f in OLD:
                assert np.array_equal(getattr(g, f), getattr(x, f)) and np.array_equal(getattr(g, f), getattr(z, f)), (f, band, E)
            assert all(getattr(x, f) is not None for f in NEW)
            # without the gapped and the pile-up outputs the extension is the same: asking for it implies both
            w = mf.align_reads(ks, reads, band, 2, max_permille, mf.KEEP_ACCEPTED, pileup=False, extend=E)
            assert w.pileup is None and w.gapped is None and w.ins_pile is None
            for f in NEW:
                assert np.array_equal(getattr(w, f), getattr(x, f)), (f, band, E)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 2. parity with the oracle
@pytest.mark.parametrize("k,band", [(21, 0), (21, 4), (31, 0), (31, 8), (31, 30), (41, 8), (41, 31)])
@pytest.mark.parametrize("uniform", [None, 64, 100], ids=["ragged", "len64", "len100"])
def test_extended_matches_oracle(mf, ol, k, band, uniform):
    text = xd.ends_bait()[0]
    X, seqs, want, ins, ext = ends_want(k, band, uniform)
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    assert reads.info.uniform_len == (uniform or 0)
    for E in ES:
        for min_depth in (1, 3):
            a = mf.align_reads(ks, reads, band, min_depth, xd.CUT, mf.KEEP_ACCEPTED, extend=E, gapped=True)
            assert np.array_equal(a.base_depth.astype(np.int64), np.minimum(want["depth"], po.CLAMP))
            assert a.place_records["over_begin"].astype(np.int64).tolist() == want["place_rec"][:, 2].astype(np.int64).tolist()
            assert bytes(a.gapped) == X.G.call(want, ins, min_depth)[0]
            check_extended(a, X, want, ins, ext[:, :, :E], min_depth, E)
    if uniform is None:
        assert int(ext.sum()) > 1500 and int(a.extend_records["begin_bases"].sum()) > 60 and int(a.extend_records["end_bases"].sum()) > 60
    reads.close(); ks.close()


# ------------------------------------------------------------------ 3. reconstruction
@pytest.mark.parametrize("shape", xd.SHAPES, ids=lambda s: "k%d_band%d_E%d" % s[:3])
def test_the_extension_reconstructs_the_flanks(mf, ol, shape):
    k, band, E, min_depth, read_len, step = shape
    genome, bait, seqs = xd.reconstruction(read_len, step)
    text = ">g\n" + bait + "\n"
    o = po.PlaceOracle(text, k)
    want = xo.ExtendOracle(o).run(seqs, o.tally(seqs), 1, 1000, band, min_depth, E)
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    a = mf.align_reads(ks, reads, band, min_depth, 1000, extend=E, gapped=True)
    assert bytes(a.extended) == want["extended"] and np.array_equal(ext_table(a.ext_pile), want["ext_pile"])
    r = a.extend_records[0]
    nb, ne = int(r["begin_bases"]), int(r["end_bases"])
    assert [int(r[f]) for f in EXT_REC] == want["extend_records"][0] and min(nb, ne) >= (16 if E == 16 else 32)
    assert bytes(a.extended).decode().upper() == genome[xd.BAIT_LO - nb:xd.BAIT_HI + ne]
    # the wrapper's restatement of the rule over the downloaded arrays
    x2 = mf.extended_consensus(a.gapped, a.gapped_starts, a.ext_pile, min_depth)
    assert np.array_equal(x2[0], a.extended) and np.array_equal(x2[1], a.extended_starts) and np.array_equal(x2[2], a.extend_records)
    reads.close(); ks.close()


def test_bim_consensus_bait_grows_twice(mf, tmp_path):
    from mitoflex_amd.bim import bim
    genome, bait, seqs = xd.reconstruction(100, 4)
    fq = str(tmp_path / "k.fq")
    write_fastq(fq, seqs, "a")
    fa = [str(tmp_path / ("g%d.fa" % i)) for i in range(3)]
    open(fa[0], "w").write(">g\n" + bait + "\n")
    body = lambda p: "".join(open(p).read().split("\n")[1:]).upper()
    at, n = [genome.find(bait)], [len(bait)]
    for gen in (1, 2):
        rec = bim.consensus_bait(fa[gen - 1], fq, None, fa[gen], 31, 3, band=4, extend=64)
        assert rec.dtype == mf.PILEUP_RECORD and open(fa[gen]).read().startswith(">g\n")          # the summaries stay what they are
        s = body(fa[gen])
        at.append(genome.find(s)); n.append(len(s))
        assert at[gen] >= 0                                           # still a substring of the genome
        assert at[gen] < at[gen - 1] and at[gen] + n[gen] > at[gen - 1] + n[gen - 1]          # strictly longer at both ends
    plain = str(tmp_path / "plain.fa")
    bim.consensus_bait(fa[0], fq, None, plain, 31, 3, band=4)
    assert len(body(plain)) == len(bait)
    with pytest.raises(ValueError, match="extend needs a band"):
        bim.consensus_bait(fa[0], fq, None, str(tmp_path / "no.fa"), 31, 3, extend=64)


# ------------------------------------------------------------------ 4. several reads a wave
def test_tiled_reads_match_oracle(mf, ol):
    text = xd.ends_bait()[0]
    X, distinct, want, ins, ext = ends_want(31, 8)
    seqs, _ = ad.tiled_reads(distinct, COPIES, seed=5)
    assert int(want["passes"].sum()) * COPIES > 4 * 8192          # above 8 192 passing reads a wave takes more than one
    tiled = {f: want[f] * COPIES for f in ("depth", "counts", "indels")}
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for E, min_depth in ((64, 1), (64, 3 * COPIES), (4096, 3 * COPIES)):
        a = mf.align_reads(ks, reads, 8, min_depth, xd.CUT, mf.KEEP_ACCEPTED, extend=E, gapped=True)
        assert np.array_equal(a.base_depth.astype(np.int64), tiled["depth"])
        assert np.array_equal(np.stack([a.pileup[f].astype(np.int64) for f in "acgt"], axis=1), tiled["counts"])
        assert np.array_equal(np.stack([a.ins_pile[f].astype(np.int64) for f in "acgt"], axis=2), ins * COPIES)
        check_extended(a, X, tiled, ins * COPIES, ext[:, :, :E] * COPIES, min_depth, E)
        assert a.extend_records["begin_piled"].astype(np.int64).tolist() == (ext[:, 0, :E].sum(axis=(1, 2)) * COPIES).tolist()
    reads.close(); ks.close()


# ------------------------------------------------------------------ 5. file level
def mates():
    return [ends_want(31, 8, None, seed) for seed in (79, 83)]


def summed(two):
    (X, _, w1, i1, e1), (_, _, w2, i2, e2) = two
    return X, {f: w1[f] + w2[f] for f in ("depth", "counts", "indels")}, i1 + i2, e1 + e2


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_extended_add_over_mates(mf, ol, tmp_path, monkeypatch, ingest):
    gz = ingest == "device-gz"
    monkeypatch.setenv("MF_INGEST", "device" if gz else "host")
    monkeypatch.setenv("MF_BATCH_READS", "300")
    for name, value in GZDEV.items():
        monkeypatch.setenv(name, value)
    two = mates()
    m1, m2 = two[0][1] * 4, two[1][1] * 4                          # four copies a mate: several batches of 300
    assert len(m1) == len(m2) > 600
    suffix = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + suffix)), str(tmp_path / ("a_2" + suffix))
    write_fastq(fq1, m1, "a", gz=gz)
    write_fastq(fq2, m2, "b", gz=gz)
    X, both, ins, ext = summed(two)
    both, ins, ext = {f: v * 4 for f, v in both.items()}, ins * 4, ext * 4
    ks = mf.KmerSet.from_text(xd.ends_bait()[0], 31)
    out = [str(tmp_path / n) for n in ("x_1.fq", "x_2.fq", "g_1.fq", "g_2.fq")]
    for pair_mode in (mf.PAIR_EITHER, mf.PAIR_BOTH):
        x = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[0], out[1], band=8, pair_mode=pair_mode, min_depth=3, max_permille=xd.CUT, keep=mf.KEEP_ACCEPTED,
                                          extend=64, gapped=True)
        assert mf.last_ingest_stats()["path"] == (1 if gz else 0)
        g = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[2], out[3], band=8, pair_mode=pair_mode, min_depth=3, max_permille=xd.CUT, keep=mf.KEEP_ACCEPTED,
                                          gapped=True)
        assert filecmp.cmp(out[0], out[2], shallow=False) and filecmp.cmp(out[1], out[3], shallow=False) and (x.kept, x.total) == (g.kept, g.total)
        for f in OLD[4:]:
            assert np.array_equal(getattr(x, f), getattr(g, f)), f
        assert all(getattr(g, f) is None for f in NEW)
        check_extended(x, X, both, ins, ext[:, :, :64], 3, 64)
    # single end: mate 1 alone
    x = mf.filter_fastq_files_aligned(ks, fq1, None, out[0], None, band=8, min_depth=3, max_permille=xd.CUT, extend=16)
    one = {f: two[0][2][f] * 4 for f in ("depth", "counts", "indels")}
    check_extended(x, X, one, two[0][3] * 4, two[0][4][:, :, :16] * 4, 3, 16)
    assert x.gapped is None
    ks.close()


CHILD = (
    "import json, sys\n"
    "from mitoflex_amd import mitofilter as mf\n"
    "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
    "out = {}\n"
    "for tag, devices in (('one', [0]), ('two', [0, 1])):\n"
    "    names = [sys.argv[4] + '/' + tag + m + '.fq' for m in '12']\n"
    "    v = mf.filter_fastq_files_aligned(ks, sys.argv[2], sys.argv[3], names[0], names[1], band=8, devices=devices, min_depth=3, max_permille=30,\n"
    "                                      keep=mf.KEEP_ACCEPTED, extend=64)\n"
    "    st = mf.last_ingest_stats()\n"
    "    out[tag] = {'n_dev': st['n_devices'], 'kept': v.kept, 'ext': [v.ext_pile[f].astype(int).tolist() for f in 'acgt'], 'extended': bytes(v.extended).decode(),\n"
    "                'starts': v.extended_starts.tolist(), 'records': [[int(x) for x in r] for r in v.extend_records.tolist()]}\n"
    "print(json.dumps(out))\n")


def test_files_extended_two_devices(mf, tmp_path):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES) in a child process: what two devices report is
    what one does, and what the oracle gives"""
    two = mates()
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(xd.ends_bait()[0])
    fq1, fq2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    write_fastq(fq1, two[0][1] * 4, "a")
    write_fastq(fq2, two[1][1] * 4, "b")
    env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST="host", MF_BATCH_READS="300", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", CHILD, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert r["one"]["n_dev"] == 1 and r["two"]["n_dev"] == 2
    X, both, ins, ext = summed(two)
    ext = ext[:, :, :64] * 4
    extended, xstarts, xrecs = X.call({f: v * 4 for f, v in both.items()}, ins * 4, ext, 3)
    for tag in ("one", "two"):
        got = r[tag]
        assert np.array_equal(np.stack([np.array(t) for t in got["ext"]], axis=3), ext), tag
        assert (got["extended"].encode(), got["starts"], got["records"]) == (extended, xstarts, xrecs), tag
    assert r["one"]["kept"] == r["two"]["kept"]


# ------------------------------------------------------------------ 6. CLI
def test_cli_extension_reports_match_the_oracle(mf, ol, tmp_path):
    two = mates()
    t = lambda n: str(tmp_path / n)
    write_fastq(t("a_1.fq.gz"), two[0][1], "p", gz=True)
    write_fastq(t("a_2.fq.gz"), two[1][1], "p", gz=True)
    open(t("bait.fa"), "w").write(xd.ends_bait()[0])
    names = ["e0", "e1", "e2"]
    base = [CLI, "bait", "--bait", t("bait.fa"), "--fq1", t("a_1.fq.gz"), "--fq2", t("a_2.fq.gz"), "-k", "31", "--max-mismatch", "30"]
    X, both, ins, ext = summed(two)
    p = subprocess.run(base + ["--out1", t("b_1.fq"), "--out2", t("b_2.fq"), "--band", "8", "--extend", "64", "--extended-consensus", t("x.fa"),
                               "--extension-report", t("x.tsv"), "--consensus", t("cons.fa"), "--min-depth", "3"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    extended, xstarts, _ = X.call(both, ins, ext[:, :, :64], 3)
    assert open(t("x.fa")).read() == extend_text.extended_fasta(names, xstarts, extended)
    assert open(t("x.tsv")).read() == extend_text.extension_text(names, ext[:, :, :64]) and len(open(t("x.tsv")).read().splitlines()) > 100
    # without the three flags the line writes what it wrote
    q = subprocess.run(base + ["--out1", t("c_1.fq"), "--out2", t("c_2.fq"), "--band", "8", "--consensus", t("cons2.fa"), "--min-depth", "3"], capture_output=True, timeout=300)
    assert q.returncode == 0 and q.stdout == p.stdout and filecmp.cmp(t("cons.fa"), t("cons2.fa"), shallow=False) and filecmp.cmp(t("b_1.fq"), t("c_1.fq"), shallow=False)
    # --band 0 --extend 16: the path is the placement's diagonal
    o = placement(31)
    X0 = xo.ExtendOracle(o)
    w0 = [X0.A.run(m, o.tally(m), 1, 30, 0) for m in (two[0][1], two[1][1])]
    e0 = sum(X0.pile(m, w, 0, 16) for m, w in zip((two[0][1], two[1][1]), w0))
    b0 = {f: w0[0][f] + w0[1][f] for f in ("depth", "counts", "indels")}
    r = subprocess.run(base + ["--out1", t("d_1.fq"), "--out2", t("d_2.fq"), "--band", "0", "--extend", "16", "--extended-consensus", t("x0.fa"),
                               "--extension-report", t("x0.tsv")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    x0, s0, _ = X0.call(b0, np.zeros((900, 0, 4), np.int64), e0, 1)
    assert open(t("x0.fa")).read() == extend_text.extended_fasta(names, s0, x0) and open(t("x0.tsv")).read() == extend_text.extension_text(names, e0)
    # the flag errors
    for extra in (["--extend", "16", "--extended-consensus", t("no.fa")], ["--band", "8", "--extended-consensus", t("no.fa")],
                  ["--band", "8", "--extension-report", t("no.tsv")], ["--band", "8", "--extend", "5000", "--extended-consensus", t("no.fa")]):
        e = subprocess.run(base + ["--out1", t("e_1.fq"), "--out2", t("e_2.fq")] + extra, capture_output=True, timeout=60)
        assert e.returncode == 1 and e.stderr.startswith(b"error: ") and not os.path.exists(t("no.fa")) and not os.path.exists(t("no.tsv")), extra


# ------------------------------------------------------------------ 7. refusals
def test_protein_sets_and_bad_extends_are_refused(mf, ol):
    from tests.util_data import make_protein_bait
    seqs, _ = xd.ends_reads()
    reads = upload(mf, ol, seqs[:50])
    prot = mf.KmerSet.protein_from_text(make_protein_bait()[0], 9)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.align_reads(prot, reads, 4, extend=16)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.filter_fastq_files_aligned(prot, "no_such.fq", None, "o.fq", None, band=4, extend=16)
    prot.close()
    ks = mf.KmerSet.from_text(xd.ends_bait()[0], 21)
    with pytest.raises(mf.MitoFilterError, match="band"):
        mf.align_reads(ks, reads, 21, extend=16)
    lib = mf.load()
    x = np.zeros(4, np.uint64)
    rc = lib.mf_align_extended(ks._h, reads._h, 1, mf.MODE_SCREENED, 1, 1000, 0, 4, 0, *([None] * 15), None, None, x.ctypes.data, None, None, None)
    assert rc == -1 and b"extend is 0" in lib.mf_last_error() and not x.any()
    reads.close(); ks.close()
