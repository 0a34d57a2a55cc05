"""The gapped consensus (mf_align_gapped, mf_filter_fastq_files_gapped) against the plain-Python oracle of tests/gapped_oracle.py, which
is written from the rule in include/mitofilter.h: the insertion pile, the gapped consensus, its record offsets and its record summaries
are compared exactly; every output the older aligning call gives is held to that call bit for bit.  There is no tolerance anywhere."""
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import align_data as ad
from tests import gapped_data as gd
from tests import gapped_oracle as go
from tests import gapped_text
from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests.report_data import mf, ol, upload  # noqa: F401  (fixtures)
from tests.util_data import write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")

OLD = ("bits", "keep_bits", "place", "align", "base_depth", "place_records", "pileup", "consensus", "pileup_records", "indels", "align_records", "unplaced")
NEW = ("ins_pile", "gapped", "gapped_starts", "gapped_records")
GAP_REC = ("length", "deleted", "insertions", "inserted_bases")


@functools.lru_cache(maxsize=None)
def inputs():
    text, parts = ad.align_bait()
    seqs, groups = ad.ragged_reads(parts)
    return text, parts, seqs, groups


@functools.lru_cache(maxsize=None)
def placement(k):
    """the placement oracle of the bait for k: computed once, shared, left unchanged"""
    return po.PlaceOracle(inputs()[0], k)


@functools.lru_cache(maxsize=None)
def ragged_want(k, band, max_permille):
    """the oracle's run on the ragged reads and their insertion pile (the call is made per min_depth from these)"""
    o = placement(k)
    G = go.GappedOracle(o)
    seqs = inputs()[2]
    want = G.A.run(seqs, o.tally(seqs), 1, max_permille, band)
    return G, want, G.pile(seqs, want, band)


def pile_table(ins_pile):
    return np.stack([ins_pile[f].astype(np.int64) for f in "acgt"], axis=2)


def check_gapped(a, G, want, pile, min_depth, band):
    """the four new outputs of one call against the oracle's sums"""
    got = pile_table(a.ins_pile)
    assert got.shape == pile.shape and np.array_equal(got, go.clamped(pile)), np.argwhere(got != pile)[:8].tolist()
    # for every position: the sum over the offsets and the four letters is at most ins_bases
    assert (got.sum(axis=(1, 2)) <= a.indels["ins_bases"].astype(np.int64)).all()
    gapped, gstarts, grecs = G.call(want, pile, min_depth)
    assert a.gapped_starts.tolist() == gstarts
    assert bytes(a.gapped) == gapped
    assert [[int(a.gapped_records[f][j]) for f in GAP_REC] for j in range(len(grecs))] == grecs
    lens = np.diff(np.asarray(G.o.starts, np.int64))
    r = a.gapped_records
    assert np.array_equal(r["length"].astype(np.int64), lens - r["deleted"].astype(np.int64) + r["inserted_bases"].astype(np.int64))
    assert np.array_equal(np.diff(a.gapped_starts.astype(np.int64)), r["length"].astype(np.int64))


# ------------------------------------------------------------------ 1. the older outputs are unchanged
@pytest.mark.parametrize("max_permille", [30, 1000])
def test_old_outputs_are_unchanged(mf, ol, max_permille):
    text, _, seqs, _ = inputs()
    assert len(seqs) == 2007
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for keep in (mf.KEEP_PASSING, mf.KEEP_ACCEPTED):
        a = mf.align_reads(ks, reads, 8, 2, max_permille, keep)
        g = mf.align_reads(ks, reads, 8, 2, max_permille, keep, gapped=True)
        for f in OLD:
            assert np.array_equal(getattr(a, f), getattr(g, f)), (f, keep)
        assert all(getattr(a, f) is None for f in NEW) and all(getattr(g, f) is not None for f in NEW)
        # mf_align_gapped with the four outputs NULL is mf_align
        lib = mf.load()
        n, P, R = len(seqs), int(ks.record_starts[-1]), len(ks.record_starts) - 1
        bits, keep_bits = np.zeros((n + 31) // 32, np.uint32), np.zeros((n + 31) // 32, np.uint32)
        place, align = np.zeros(n, mf.PLACE), np.zeros(n, mf.ALIGN)
        depth, precs, pile, cons = np.zeros(P, np.uint32), np.zeros(R, mf.PLACE_RECORD), np.zeros(P, mf.PILEUP), np.zeros(P, np.uint8)
        prec2, indels, arecs, unplaced = np.zeros(R, mf.PILEUP_RECORD), np.zeros(P, mf.INDEL), np.zeros(R, mf.ALIGN_RECORD), np.zeros(2, np.uint64)
        ptr = lambda x: x.ctypes.data
        rc = lib.mf_align_gapped(ks._h, reads._h, 1, mf.MODE_SCREENED, 2, max_permille, int(keep), 8, ptr(bits), ptr(keep_bits), ptr(place), ptr(align), ptr(depth),
                                 ptr(precs), ptr(pile), ptr(cons), ptr(prec2), ptr(indels), ptr(arecs), None, None, None, None, ptr(unplaced), None)
        assert rc == 0, lib.mf_last_error()
        for f, x in zip(OLD, (bits, keep_bits, place, align, depth, precs, pile, cons, prec2, indels, arecs, unplaced)):
            assert np.array_equal(getattr(a, f), x), (f, keep)
        # without the pile-up outputs the gapped consensus is the same: asking for it implies the counters
        w = mf.align_reads(ks, reads, 8, 2, max_permille, keep, pileup=False, gapped=True)
        assert w.pileup is None and w.consensus is None and w.pileup_records is None
        for f in NEW + ("align", "indels", "base_depth"):
            assert np.array_equal(getattr(w, f), getattr(g, f)), f
    reads.close(); ks.close()


# ------------------------------------------------------------------ 2. parity with the oracle
@pytest.mark.parametrize("k,band", [(21, 1), (21, 4), (21, 20), (31, 1), (31, 8), (31, 30), (41, 8), (41, 31)])
def test_gapped_matches_oracle(mf, ol, k, band):
    text, _, seqs, groups = inputs()
    max_permille = {1: 1000, 4: 40, 8: 60}.get(band, 20)
    G, want, pile = ragged_want(k, band, max_permille)
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    for min_depth in (1, 3):
        a = mf.align_reads(ks, reads, band, min_depth, max_permille, mf.KEEP_ACCEPTED, gapped=True)
        assert a.ins_pile.shape == (int(ks.record_starts[-1]), 2 * band)
        assert np.array_equal(np.stack([a.indels[f].astype(np.int64) for f in ("del", "ins", "ins_bases")], axis=1), want["indels"])
        assert np.array_equal(a.base_depth.astype(np.int64), np.minimum(want["depth"], po.CLAMP))
        check_gapped(a, G, want, pile, min_depth, band)
    if band >= 4:
        assert int(pile.sum()) > 300 and int(a.gapped_records["deleted"].sum()) > 0          # the stack's three deleted positions at the least
    reads.close(); ks.close()


@pytest.mark.parametrize("L", [64, 65, 150])
def test_uniform_lengths_match_oracle(mf, ol, L):
    text, parts, _, _ = inputs()
    for k, band in ((21, 4), (31, 8)):
        seqs = ad.uniform_reads(parts, L, 240, seed=100 + L)
        o = placement(k)
        G = go.GappedOracle(o)
        want = G.A.run(seqs, o.tally(seqs), 1, 50, band)
        pile = G.pile(seqs, want, band)
        ks = mf.KmerSet.from_text(text, k)
        reads = upload(mf, ol, seqs)
        assert reads.info.uniform_len == L
        for min_depth in (1, 3):
            check_gapped(mf.align_reads(ks, reads, band, min_depth, 50, mf.KEEP_ACCEPTED, gapped=True), G, want, pile, min_depth, band)
        reads.close(); ks.close()


# ------------------------------------------------------------------ 3. band 0
def test_band_0_is_the_consensus(mf, ol):
    text, _, seqs, _ = inputs()
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for min_depth in (1, 3):
        a = mf.align_reads(ks, reads, 0, min_depth, 30, gapped=True)
        assert np.array_equal(a.gapped, a.consensus) and np.array_equal(a.gapped_starts, ks.record_starts)
        assert a.ins_pile.shape == (int(ks.record_starts[-1]), 0)
        assert a.gapped_records["length"].tolist() == np.diff(ks.record_starts.astype(np.int64)).tolist()
        assert not any(a.gapped_records[f].any() for f in GAP_REC[1:])
        b = mf.align_reads(ks, reads, 0, min_depth, 30)
        for f in OLD:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    reads.close(); ks.close()


# ------------------------------------------------------------------ 4. reconstruction
@pytest.mark.parametrize("k,band", [(31, 8), (21, 4), (31, 1)])
def test_the_gapped_consensus_reconstructs_the_sample(mf, ol, k, band):
    bait, sample, seqs = gd.reconstruction(band)
    o = po.PlaceOracle(">g\n" + bait + "\n", k)
    want = go.GappedOracle(o).run(seqs, o.tally(seqs), 1, 1000, band, 3)
    # the oracle first
    assert want["accepted"].all() and len(seqs) == 451
    text = want["gapped"].decode()
    assert text.upper() == sample
    D = []                                                          # the depth behind every emitted byte
    for p in range(len(bait)):
        D += [int(want["depth"][p])] * (len(go.call([0, 1], want["depth"][p:p + 1], want["indels"][p:p + 1, 0], b"x", want["ins_pile"][p:p + 1], 3)[0]))
    assert len(D) == len(text)
    lower = np.array([c.islower() for c in text])
    assert lower.any() and (np.array(D)[lower] < 3).all()          # lower case only where the depth is below min_depth
    ks = mf.KmerSet.from_text(">g\n" + bait + "\n", k)
    reads = upload(mf, ol, seqs)
    a = mf.align_reads(ks, reads, band, 3, 1000, gapped=True)
    assert bytes(a.gapped) == want["gapped"] and bytes(a.gapped).decode().upper() == sample
    assert a.gapped_starts.tolist() == [0, len(sample)]
    assert [int(a.gapped_records[f][0]) for f in GAP_REC] == want["gapped_records"][0]
    assert (int(a.gapped_records["deleted"][0]), int(a.gapped_records["inserted_bases"][0])) == (min(3, band), min(5, band))
    assert np.array_equal(pile_table(a.ins_pile), want["ins_pile"])
    # the wrapper's restatement of the rule over the downloaded arrays
    g2 = mf.gapped_consensus(ks.record_starts, a.base_depth, a.indels, a.ins_pile, a.consensus, 3)
    assert np.array_equal(g2[0], a.gapped) and np.array_equal(g2[1], a.gapped_starts) and np.array_equal(g2[2], a.gapped_records)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 5. stacks and ties
def test_stacks_and_ties(mf, ol):
    """identical reads: every insertion adds to the same four addresses"""
    bait = gd.stack_bait()
    text = ">s\n" + bait + "\n"
    o = po.PlaceOracle(text, 31)
    G = go.GappedOracle(o)
    ks = mf.KmerSet.from_text(text, 31)
    cases = ((gd.stack_reads(bait, 250, 0, other="TGCT", n_other=250), bait[:250] + "TNCT" + bait[250:], [604, 0, 1, 4]),
             (gd.stack_reads(bait, 250, 250), bait, [600, 0, 0, 0]),
             (gd.stack_reads(bait, 251, 250), bait[:250] + "TCCT" + bait[250:], [604, 0, 1, 4]))
    for seqs, called, rec in cases:
        want = G.run(seqs, o.tally(seqs), 1, 1000, 8, 1)
        assert want["accepted"].all() and want["gapped"].decode().upper() == called and want["gapped_records"] == [rec]
        reads = upload(mf, ol, seqs)
        a = mf.align_reads(ks, reads, 8, 1, 1000, gapped=True)
        check_gapped(a, G, want, want["ins_pile"], 1, 8)
        assert bytes(a.gapped).decode().upper() == called
        reads.close()
    ks.close()


# ------------------------------------------------------------------ 6. several reads a wave
def test_tiled_reads_match_oracle(mf, ol):
    text, parts, _, _ = inputs()
    distinct, _ = ad.distinct_reads(parts)
    seqs, index = ad.tiled_reads(distinct, ad.TILE_COPIES, seed=5)
    o = placement(31)
    G = go.GappedOracle(o)
    want = G.A.run(distinct, o.tally(distinct), 1, ad.TILE_CUT, 8)
    assert int(want["passes"].sum()) * ad.TILE_COPIES > 4 * 8192          # above 8 192 passing reads a wave takes more than one
    pile = G.pile(distinct, want, 8) * ad.TILE_COPIES
    tiled = {f: want[f] * ad.TILE_COPIES for f in ("depth", "counts", "indels")}
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for min_depth in (1, 3 * ad.TILE_COPIES):
        a = mf.align_reads(ks, reads, 8, min_depth, ad.TILE_CUT, mf.KEEP_ACCEPTED, gapped=True)
        assert np.array_equal(a.base_depth.astype(np.int64), tiled["depth"])
        assert np.array_equal(np.stack([a.indels[f].astype(np.int64) for f in ("del", "ins", "ins_bases")], axis=1), tiled["indels"])
        assert np.array_equal(np.stack([a.pileup[f].astype(np.int64) for f in "acgt"], axis=1), tiled["counts"])
        check_gapped(a, G, tiled, pile, min_depth, 8)
    assert int(pile.sum()) > 50 * ad.TILE_COPIES
    reads.close(); ks.close()


# ------------------------------------------------------------------ 7. file level
@pytest.mark.parametrize("gz", [True, False], ids=["gz", "plain"])
def test_files_gapped_add_over_mates(mf, ol, tmp_path, gz):
    text, parts, _, _ = inputs()
    m1, m2, _ = ad.align_mates(parts)
    ext = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
    write_fastq(fq1, m1, "a", gz=gz)
    write_fastq(fq2, m2, "b", gz=gz)
    ks = mf.KmerSet.from_text(text, 31)
    x, y = [], []
    for m, into in ((m1, x), (m2, y)):
        reads = upload(mf, ol, m)
        into.append(mf.align_reads(ks, reads, ad.FILE_BAND, 2, ad.FILE_CUT, mf.KEEP_ACCEPTED, gapped=True))
        reads.close()
    x, y = x[0], y[0]
    out = [str(tmp_path / n) for n in ("g_1.fq", "g_2.fq", "a_1o.fq", "a_2o.fq")]
    f = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[0], out[1], band=ad.FILE_BAND, min_depth=2, max_permille=ad.FILE_CUT, keep=mf.KEEP_ACCEPTED, gapped=True)
    v = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[2], out[3], band=ad.FILE_BAND, min_depth=2, max_permille=ad.FILE_CUT, keep=mf.KEEP_ACCEPTED)
    assert filecmp.cmp(out[0], out[2], shallow=False) and filecmp.cmp(out[1], out[3], shallow=False) and (f.kept, f.total) == (v.kept, v.total)
    for name in ("base_depth", "place_records", "pileup", "consensus", "pileup_records", "indels", "align_records", "unplaced"):
        assert np.array_equal(getattr(f, name), getattr(v, name)), name
    assert all(getattr(v, name) is None for name in NEW)
    assert np.array_equal(pile_table(f.ins_pile), pile_table(x.ins_pile) + pile_table(y.ins_pile)) and int(pile_table(f.ins_pile).sum()) > 100
    # the call on the sums (nothing here is clamped): the wrapper's restatement of the rule, which tests/test_gapped_oracle.py holds to the oracle
    g, gstarts, grecs = mf.gapped_consensus(ks.record_starts, f.base_depth, f.indels, f.ins_pile, f.consensus, 2)
    assert np.array_equal(f.gapped, g) and np.array_equal(f.gapped_starts, gstarts) and np.array_equal(f.gapped_records, grecs)
    assert int(f.gapped_records["deleted"].sum()) > 0 and not np.array_equal(f.gapped, f.consensus)
    ks.close()


# ------------------------------------------------------------------ 8. CLI
def test_cli_gapped_reports_match_the_oracle(mf, ol, tmp_path):
    text, parts, seqs, groups = inputs()
    lo, hi = groups["indel"]
    st = groups["stack"][0]                                         # 60 + 60 identical reads with a 3-base deletion: the gapped consensus calls it
    m1 = seqs[lo:lo + 250] + seqs[:150] + seqs[st:st + 60]
    m2 = seqs[lo + 250:hi] + seqs[150:300] + seqs[st + 60:st + 120]
    t = lambda n: str(tmp_path / n)
    write_fastq(t("a_1.fq.gz"), m1, "p", gz=True)
    write_fastq(t("a_2.fq.gz"), m2, "p", gz=True)
    open(t("bait.fa"), "w").write(text)
    o = placement(31)
    G = go.GappedOracle(o)
    want = [G.A.run(m, o.tally(m), 1, 30, 8) for m in (m1, m2)]
    pile = G.pile(m1, want[0], 8) + G.pile(m2, want[1], 8)
    both = {f: want[0][f] + want[1][f] for f in ("depth", "counts", "indels")}
    gapped, gstarts, _ = G.call(both, pile, 2)
    names, starts = ["g", "rep", "short"], [int(s) for s in o.starts]
    base = [CLI, "bait", "--bait", t("bait.fa"), "--fq1", t("a_1.fq.gz"), "--fq2", t("a_2.fq.gz"), "-k", "31", "--max-mismatch", "30"]
    p = subprocess.run(base + ["--out1", t("b_1.fq"), "--out2", t("b_2.fq"), "--band", "8", "--gapped-consensus", t("gapped.fa"), "--insertions", t("ins.tsv"),
                               "--consensus", t("cons.fa"), "--min-depth", "2"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(t("gapped.fa")).read() == gapped_text.gapped_fasta(names, gstarts, gapped)
    assert open(t("ins.tsv")).read() == gapped_text.insertions_text(names, starts, both["depth"], pile)
    assert open(t("cons.fa")).read() == mf.consensus_fasta(names, starts, pio.PileupOracle(o).call(both["counts"], 2)[0])
    assert open(t("gapped.fa")).read() != open(t("cons.fa")).read() and len(open(t("ins.tsv")).read().splitlines()) > 20
    # without the new flags the line writes what it wrote
    q = subprocess.run(base + ["--out1", t("c_1.fq"), "--out2", t("c_2.fq"), "--band", "8", "--consensus", t("cons2.fa"), "--min-depth", "2"], capture_output=True, timeout=300)
    assert q.returncode == 0 and q.stdout == p.stdout and filecmp.cmp(t("cons.fa"), t("cons2.fa"), shallow=False) and filecmp.cmp(t("b_1.fq"), t("c_1.fq"), shallow=False)
    # --gapped-consensus without --band
    r = subprocess.run(base + ["--out1", t("d_1.fq"), "--out2", t("d_2.fq"), "--gapped-consensus", t("no.fa")], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--band" in r.stderr and not os.path.exists(t("no.fa"))


# ------------------------------------------------------------------ 9. bim
def test_bim_consensus_bait_gapped(mf, tmp_path):
    from mitoflex_amd.bim import bim
    bait, sample, seqs = gd.reconstruction(8)
    fa, fq = str(tmp_path / "bait.fa"), str(tmp_path / "k.fq")
    open(fa, "w").write(">g\n" + bait + "\n")
    write_fastq(fq, seqs, "a")
    out = {n: str(tmp_path / (n + ".fa")) for n in ("band", "plain", "gapped")}
    r1 = bim.consensus_bait(fa, fq, None, out["band"], 31, 3, band=8)
    r0 = bim.consensus_bait(fa, fq, None, out["plain"], 31, 3, band=8, gapped=False)
    r2 = bim.consensus_bait(fa, fq, None, out["gapped"], 31, 3, band=8, gapped=True)
    assert open(out["band"]).read() == open(out["plain"]).read() and np.array_equal(r0, r1) and np.array_equal(r1, r2)
    body = lambda p: "".join(open(p).read().split("\n")[1:])
    assert open(out["gapped"]).read().startswith(">g\n")
    assert len(body(out["band"])) == len(bait) and body(out["gapped"]).upper() == sample
    with pytest.raises(ValueError, match="gapped needs a band"):
        bim.consensus_bait(fa, fq, None, str(tmp_path / "no.fa"), 31, 3, gapped=True)
    # the polished bait can be baited with again: the reads lie on it without an indel
    ks = mf.KmerSet.from_fasta(out["gapped"], 31)
    assert int(ks.record_starts[-1]) == len(sample)
    v = mf.filter_fastq_files_aligned(ks, fq, None, str(tmp_path / "o.fq"), None, band=8, min_depth=3)
    assert int(v.align_records["accepted"][0]) == len(seqs) and int(v.align_records["gapped"][0]) == 0 and int(v.align_records["mismatches"][0]) == 0
    ks.close()


# ------------------------------------------------------------------ 10. refusals
def test_band_at_k_and_protein_sets_are_refused(mf, ol):
    from tests.util_data import make_protein_bait
    text, _, seqs, _ = inputs()
    reads = upload(mf, ol, seqs[:50])
    ks = mf.KmerSet.from_text(text, 21)
    for band in (21, 31):
        with pytest.raises(mf.MitoFilterError, match="band"):
            mf.align_reads(ks, reads, band, gapped=True)
        with pytest.raises(mf.MitoFilterError, match="band"):
            mf.filter_fastq_files_aligned(ks, "no_such.fq", None, "o.fq", None, band=band, gapped=True)
    assert mf.align_reads(ks, reads, 20, gapped=True).gapped is not None
    ks.close()
    prot = mf.KmerSet.protein_from_text(make_protein_bait()[0], 9)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.align_reads(prot, reads, 4, gapped=True)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.filter_fastq_files_aligned(prot, "no_such.fq", None, "o.fq", None, band=4, gapped=True)
    prot.close(); reads.close()
