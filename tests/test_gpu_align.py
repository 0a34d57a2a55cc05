"""Banded alignment of the placed reads (mf_align, mf_filter_fastq_files_aligned) against the plain-Python oracle of
tests/align_oracle.py, which is written from the rule in include/mitofilter.h: per-read alignments, the cut, the keep bits, and every
placement, pile-up and indel output of the accepted reads are compared exactly; band 0 is held to mf_verify_keep of the same library bit
for bit.  There is no tolerance anywhere."""
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import align_text
from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests import verify_oracle as vo
from tests.report_data import mf, ol, upload  # noqa: F401  (fixtures)
from tests.util_data import bits_to_bool, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")

PLACE_FIELDS = ("record", "strand", "start", "end", "votes", "windows")
ALIGN_FIELDS = ("compared", "mismatches", "insertions", "deletions", "ref_begin", "ref_end")
PLACE_REC = ("forward", "reverse", "over_begin", "over_end", "covered", "base_sum")
PILE_REC = ("bases", "matches", "mismatches", "called", "ambiguous", "variants")
ALIGN_REC = ("accepted", "rejected", "compared", "mismatches", "insertions", "deletions", "gapped")
SHARED = ("bits", "keep_bits", "place", "base_depth", "place_records", "pileup", "consensus", "pileup_records", "unplaced")


def table(a, fields):
    return np.stack([a[f].astype(np.int64) for f in fields], axis=1)


def align_rows(records):
    return np.concatenate([table(records, ALIGN_REC), records["hist"].astype(np.int64)], axis=1).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def inputs():
    text, parts = ad.align_bait()
    seqs, groups = ad.ragged_reads(parts)
    return text, parts, seqs, groups


@functools.lru_cache(maxsize=None)
def placement(k):
    """the placement oracle of the bait for k and the tallies of the ragged reads: computed once, shared, left unchanged"""
    text, _, seqs, _ = inputs()
    o = po.PlaceOracle(text, k)
    return o, o.tally(seqs)


def first_bad(got, want):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    return [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def identities(a, want=None):
    """the identities of the header's banded-alignment section"""
    r, p = a.align_records, a.place_records
    assert np.array_equal(r["accepted"], p["forward"] + p["reverse"])
    assert np.array_equal(r["hist"].sum(axis=1), r["accepted"] + r["rejected"])
    if want is not None:
        assert np.array_equal(p["base_sum"].astype(np.int64), want["footprints"])
    if a.pileup_records is not None:
        assert np.array_equal(a.pileup_records["mismatches"], r["mismatches"])


def check(mf, ks, reads, o, seqs, want, band, max_permille, keep, min_depth=2, threshold=1, mode=0):
    """one mf_align call against what the oracle gave for (threshold, band, max_permille); mode 0 is MODE_SCREENED"""
    a = mf.align_reads(ks, reads, band, min_depth, max_permille, keep, threshold=threshold, mode=mode)
    return check_result(mf, a, o, seqs, want, keep, min_depth)


def check_result(mf, a, o, seqs, want, keep, min_depth):
    """what an aligning call gave -- mf_align, or the outputs mf_align_gapped and mf_align_extended share with it -- against what the oracle
    gave for its band and cut; the pile-up outputs where the call was asked for them"""
    n = len(seqs)
    assert np.array_equal(bits_to_bool(a.bits, n), want["passes"])
    got = table(a.place, PLACE_FIELDS)
    assert np.array_equal(got, want["rows"]), first_bad(got, want["rows"])
    got = table(a.align, ALIGN_FIELDS)
    assert np.array_equal(got, want["aligns"]), first_bad(got, want["aligns"])
    assert np.array_equal(a.base_depth.astype(np.int64), np.minimum(want["depth"], po.CLAMP)), first_bad(a.base_depth.astype(np.int64), want["depth"])
    assert np.array_equal(table(a.place_records, PLACE_REC).astype(np.uint64), want["place_rec"]), (table(a.place_records, PLACE_REC), want["place_rec"])
    assert np.array_equal(align_rows(a.align_records), want["align_rec"]), (align_rows(a.align_records), want["align_rec"])
    got = table(a.indels, ("del", "ins", "ins_bases"))
    assert np.array_equal(got, want["indels"]), first_bad(got, want["indels"])
    if a.pileup is not None or a.consensus is not None or a.pileup_records is not None:          # (pileup=False gives none of the three)
        got = table(a.pileup, ("a", "c", "g", "t"))
        assert np.array_equal(got, pio.clamped(want["counts"])), first_bad(got, want["counts"])
        cons, rec = pio.PileupOracle(o).call(want["counts"], min_depth)
        assert np.array_equal(a.consensus, cons)
        assert np.array_equal(table(a.pileup_records, PILE_REC).astype(np.uint64), rec)
    assert a.unplaced.tolist() == want["unplaced"]
    placed = want["rows"][:, 0] < po.AMBIGUOUS
    cleared = placed & ~want["accepted"] if keep == mf.KEEP_ACCEPTED else (want["passes"] & ~(placed & want["accepted"]) if keep == mf.KEEP_PLACED else np.zeros(n, bool))
    assert np.array_equal(bits_to_bool(a.keep_bits, n), want["passes"] & ~cleared)
    identities(a, want)
    # sum(del) over a record <= deletions: a deleted position outside the record counts in the read, not in the table
    for j in range(len(o.recs)):
        lo, hi = int(o.starts[j]), int(o.starts[j + 1])
        assert int(a.indels["del"][lo:hi].sum()) <= int(a.align_records["deletions"][j])
    return a


# ------------------------------------------------------------------ 1. band 0 is mf_verify_keep, bit for bit
@pytest.mark.parametrize("keep", [0, 1, 2])
def test_band_0_is_verify_keep(mf, ol, keep):
    text, _, seqs, _ = inputs()
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    for max_permille in (0, 30, 1000):
        v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 2, max_permille, keep=keep)
        a = mf.align_reads(ks, reads, 0, 2, max_permille, keep)
        for f in SHARED:
            want = v.bits if f == "keep_bits" and keep == mf.KEEP_PASSING else getattr(v, f)
            assert np.array_equal(getattr(a, f), want), (f, max_permille)
        assert np.array_equal(a.align["compared"], v.score["compared"]) and np.array_equal(a.align["mismatches"], v.score["mismatches"])
        assert not a.align["insertions"].any() and not a.align["deletions"].any() and not table(a.indels, ("del", "ins", "ins_bases")).any()
        placed = a.place["record"] < mf.PLACE_AMBIGUOUS
        assert np.array_equal(a.align["ref_begin"][placed], a.place["start"][placed]) and np.array_equal(a.align["ref_end"][placed], a.place["end"][placed])
        assert not a.align["ref_begin"][~placed].any() and not a.align["ref_end"][~placed].any()
        for f in ("accepted", "rejected", "compared", "mismatches", "hist"):
            assert np.array_equal(a.align_records[f], v.score_records[f]), (f, max_permille)
        assert not table(a.align_records, ("insertions", "deletions", "gapped")).any()
        # without a pile-up the other outputs are the same
        w = mf.align_reads(ks, reads, 0, 2, max_permille, keep, pileup=False)
        assert w.pileup is None and w.consensus is None and w.pileup_records is None
        assert np.array_equal(w.align, a.align) and np.array_equal(w.align_records, a.align_records) and np.array_equal(w.base_depth, a.base_depth)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 2. parity with the oracle
# band 1, 4, 8 and the widest band k allows: 31 (63 lanes) for k = 41, k - 1 below that
@pytest.mark.parametrize("k,band", [(k, b) for k in (21, 31, 41) for b in (1, 4, 8, min(31, k - 1))])
def test_align_matches_oracle(mf, ol, k, band):
    text, _, seqs, groups = inputs()
    o, tallies = placement(k)
    A = ao.AlignOracle(o)
    ks = mf.KmerSet.from_text(text, k)
    assert np.array_equal(ks.record_starts, o.starts)
    reads = upload(mf, ol, seqs)
    max_permille, keep = {1: (1000, mf.KEEP_PASSING), 4: (40, mf.KEEP_ACCEPTED), 8: (60, mf.KEEP_PLACED)}.get(band, (20, mf.KEEP_ACCEPTED))
    want = A.run(seqs, tallies, 1, max_permille, band)
    lo, hi = groups["indel"]
    assert (want["rows"][lo:hi, 0] < po.AMBIGUOUS).mean() >= 0.9          # the oracle places the simulated indel reads
    a = check(mf, ks, reads, o, seqs, want, band, max_permille, keep)
    if band >= 4:
        assert int(a.align_records["gapped"].sum()) > 300 and int(a.indels["del"].sum()) > 0 and int(a.indels["ins"].sum()) > 0
        assert int(a.align_records["rejected"].sum()) > 0
        lo, hi = groups["stack"]
        assert (want["aligns"][lo:hi, 3] == 3).all() and int(a.indels["del"].max()) >= 500
        if band >= 8:
            lo = groups["long"][0]
            assert want["aligns"][lo].tolist()[2:4] == [0, 5] and int(a.align["deletions"][lo]) == 5
    reads.close(); ks.close()


@pytest.mark.parametrize("L", ["k", "k+1", 63, 64, 65, 150, 151])
def test_uniform_lengths_match_oracle(mf, ol, L):
    text, parts, _, _ = inputs()
    for k, band in ((21, 4), (31, 8)):
        n = {"k": k, "k+1": k + 1}.get(L, L)
        seqs = ad.uniform_reads(parts, n, 240, seed=100 + n)
        o = placement(k)[0]
        ks = mf.KmerSet.from_text(text, k)
        reads = upload(mf, ol, seqs)
        assert reads.info.uniform_len == n
        want = ao.AlignOracle(o).run(seqs, o.tally(seqs), 1, 50, band)
        assert want["accepted"].sum() > 50
        check(mf, ks, reads, o, seqs, want, band, 50, mf.KEEP_ACCEPTED)
        reads.close(); ks.close()


# ------------------------------------------------------------------ 3. what it is for
def test_indel_reads_pass_a_tight_cut_that_the_ungapped_score_fails(mf, ol):
    text, parts, _, _ = inputs()
    seqs, gs = ad.indel_reads(parts, 600, seed=31, lo=150)
    o = po.PlaceOracle(text, 31)
    tallies = o.tally(seqs)
    rows = o.place(tallies, 1)[1]
    placed = rows[:, 0] < po.AMBIGUOUS
    assert placed.mean() >= 0.9
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    a = mf.align_reads(ks, reads, 8, 1, 60, mf.KEEP_ACCEPTED)
    assert np.array_equal(a.place["record"] < mf.PLACE_AMBIGUOUS, placed)
    edits = table(a.align, ("mismatches", "insertions", "deletions")).sum(axis=1)
    assert (edits[placed] <= np.array(gs)[placed]).all()
    keep = bits_to_bool(a.keep_bits, len(seqs))
    assert keep[placed].all() and int(a.align_records["rejected"].sum()) == 0
    # the ungapped score at the same cut drops the reads the verification oracle rejects -- most of these
    v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, 1, 60, keep=mf.KEEP_ACCEPTED)
    want = vo.VerifyOracle(o).verify(seqs, tallies, 1, 60)
    rejected = placed & ~want["accepted"]
    assert rejected.sum() > 300
    assert np.array_equal(bits_to_bool(v.keep_bits, len(seqs)), want["passes"] & ~rejected)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 5. file level
def test_files_aligned_add_over_mates(mf, ol, tmp_path):
    text, parts, seqs, groups = inputs()
    lo, hi = groups["indel"]
    m1 = seqs[lo:lo + 300] + seqs[:200]
    m2 = seqs[lo + 200:hi][:300] + seqs[300:500]
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, m1, "p", gz=True)
    write_fastq(fq2, m2, "p", gz=True)
    ks = mf.KmerSet.from_text(text, 31)
    per_mate = []
    for m in (m1, m2):
        reads = upload(mf, ol, m)
        per_mate.append(mf.align_reads(ks, reads, 8, 2, 50, mf.KEEP_ACCEPTED))
        reads.close()
    x, y = per_mate
    out = [str(tmp_path / n) for n in ("o_1.fq", "o_2.fq", "v_1.fq", "v_2.fq", "f_1.fq", "f_2.fq")]
    f = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[0], out[1], band=8, min_depth=2, max_permille=50, keep=mf.KEEP_ACCEPTED)
    assert np.array_equal(f.base_depth, x.base_depth + y.base_depth)
    for name, fields in (("place_records", PLACE_REC[:4]), ("align_records", ALIGN_REC + ("hist",)), ("pileup", ("a", "c", "g", "t")),
                         ("indels", ("del", "ins", "ins_bases"))):
        for fld in fields:
            assert np.array_equal(getattr(f, name)[fld], getattr(x, name)[fld] + getattr(y, name)[fld]), (name, fld)
    assert f.unplaced.tolist() == (x.unplaced + y.unplaced).tolist() and f.total == 500
    k1, k2 = bits_to_bool(x.keep_bits, 500), bits_to_bool(y.keep_bits, 500)
    assert f.kept == int((k1 | k2).sum()) and int(f.align_records["gapped"].sum()) > 100
    # with KEEP_PASSING the files are the plain filter's
    g = mf.filter_fastq_files_aligned(ks, fq1, fq2, out[2], out[3], band=8, min_depth=2, max_permille=50)
    kept, total = mf.filter_fastq_files(ks, fq1, fq2, out[4], out[5])
    assert (g.kept, g.total) == (kept, total) and kept >= f.kept
    assert filecmp.cmp(out[2], out[4], shallow=False) and filecmp.cmp(out[3], out[5], shallow=False)
    assert np.array_equal(g.align_records, f.align_records) and np.array_equal(g.indels, f.indels)
    ks.close()


def test_cli_band_reports_match_the_oracle(mf, ol, tmp_path):
    """`fastfilter bait --band 8 --indels --score-report --consensus`: the three files are the texts made from the oracle's counts added
    over the mates; with --write accepted at a tight cut the band keeps the indel-bearing reads that the same line without it drops"""
    text, parts, seqs, groups = inputs()
    lo, hi = groups["indel"]
    m1 = seqs[lo:lo + 250] + seqs[:150]
    m2 = seqs[lo + 250:hi] + seqs[150:300]
    t = lambda n: str(tmp_path / n)
    write_fastq(t("a_1.fq.gz"), m1, "p", gz=True)
    write_fastq(t("a_2.fq.gz"), m2, "p", gz=True)
    open(t("bait.fa"), "w").write(text)
    o = placement(31)[0]
    A = ao.AlignOracle(o)
    want = [A.run(m, o.tally(m), 1, 30, 8) for m in (m1, m2)]
    names, starts = ["g", "rep", "short"], [int(s) for s in o.starts]
    base = [CLI, "bait", "--bait", t("bait.fa"), "--fq1", t("a_1.fq.gz"), "--fq2", t("a_2.fq.gz"), "-k", "31", "--write", "accepted", "--max-mismatch", "30"]
    p = subprocess.run(base + ["--out1", t("b_1.fq"), "--out2", t("b_2.fq"), "--band", "8", "--indels", t("indels.tsv"), "--score-report", t("score.tsv"),
                               "--consensus", t("cons.fa"), "--min-depth", "2"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    depth = want[0]["depth"] + want[1]["depth"]
    assert open(t("score.tsv")).read() == align_text.align_report_text(names, starts, (want[0]["align_rec"] + want[1]["align_rec"]).astype(np.int64))
    assert open(t("indels.tsv")).read() == align_text.indels_text(names, starts, depth, want[0]["indels"] + want[1]["indels"])
    cons, _ = pio.PileupOracle(o).call(want[0]["counts"] + want[1]["counts"], 2)
    assert open(t("cons.fa")).read() == mf.consensus_fasta(names, starts, cons)
    keep = [w["passes"] & ~((w["rows"][:, 0] < po.AMBIGUOUS) & ~w["accepted"]) for w in want]
    assert p.stdout.decode().split() == [str(int((keep[0] | keep[1]).sum()))]
    # the same line without --band: the ungapped score rejects most of the indel reads, and their pairs are not written
    q = subprocess.run(base + ["--out1", t("u_1.fq"), "--out2", t("u_2.fq"), "--score-report", t("score_u.tsv")], capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr.decode()[-2000:]
    banded, ungapped = int(p.stdout), int(q.stdout)
    assert banded - ungapped > 150
    names_of = lambda path: set(open(path).read().split("\n")[0::4])
    assert names_of(t("u_1.fq")) < names_of(t("b_1.fq"))
    assert open(t("score_u.tsv")).read().startswith("record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tpermille\tmm0")


# ------------------------------------------------------------------ 6. bim
def test_bim_consensus_bait_with_a_band(mf, tmp_path):
    """A sample with a 3-base deletion against the bait, 67 positions before the bait's end: every read that reaches behind the deletion is
    placed by its longer part before it, so without a band the bases behind it pile three positions off and the polished bait is called
    from them; with band=8 those variants are gone and the deletion shows in the indel table."""
    import random
    from mitoflex_amd.bim import bim
    rng = random.Random(99)
    g = "".join(rng.choices("ACGT", k=2400))
    sample = g[:2330] + g[2333:]
    reads = []
    for a in range(0, len(sample) - 150 + 1, 3):                   # 150-base reads every 3 bases, both strands: depth 50
        s = sample[a:a + 150]
        if not 65 <= 2330 - a <= 85:                                # (no read with the deletion near its middle: placement's tie rule)
            reads.append(s if a % 2 else revcomp(s))
    fa, fq = str(tmp_path / "bait.fa"), str(tmp_path / "k.fq")
    open(fa, "w").write(">g\n" + g + "\n")
    write_fastq(fq, reads, "a")
    out = {n: str(tmp_path / (n + ".fa")) for n in ("default", "none", "band")}
    r0 = bim.consensus_bait(fa, fq, None, out["default"], 31, 3)
    r1 = bim.consensus_bait(fa, fq, None, out["none"], 31, 3, band=None)
    r2 = bim.consensus_bait(fa, fq, None, out["band"], 31, 3, band=8)
    assert open(out["default"]).read() == open(out["none"]).read() and np.array_equal(r0, r1)
    body = lambda p: "".join(open(p).read().split("\n")[1:])
    polluted, polished = body(out["none"]), body(out["band"])
    # (the oracles on these reads: 44 variants and 557 mismatching bases without a band, none and 4 with it)
    assert int(r0["variants"][0]) == sum(a != b for a, b in zip(polluted.upper(), g)) > 30 and int(r0["mismatches"][0]) > 400
    assert all(a == b for a, b in zip(polluted.upper()[:2330], g))          # ... all of them behind the deletion
    assert len(polished) == len(g) and polished.upper() == g
    assert int(r2["variants"][0]) == 0 and int(r2["mismatches"][0]) < 10
    ks = mf.KmerSet.from_fasta(fa, 31)
    v = mf.filter_fastq_files_aligned(ks, fq, None, str(tmp_path / "o.fq"), None, band=8, min_depth=3)
    iv = mf.indel_variants(ks.record_starts, v.base_depth, v.indels, min_depth=3, min_permille=500)
    ks.close()
    # three deleted positions at [2330, 2333), or where in the repeats around them the rule's order of moves puts them
    assert len(iv) == 3 and (iv["del"] >= 15).all() and (iv["del"] * 1000 >= 500 * iv["depth"]).all()
    assert all(2330 - 6 <= int(p) < 2333 + 6 for p in iv["pos"])
    assert int(v.align_records["deletions"][0]) >= 3 * 15 and int(v.align_records["gapped"][0]) >= 15


# ------------------------------------------------------------------ arguments that need a set
def test_band_at_k_and_protein_sets_are_refused(mf, ol):
    from tests.util_data import make_protein_bait
    text, _, seqs, _ = inputs()
    reads = upload(mf, ol, seqs[:50])
    ks = mf.KmerSet.from_text(text, 21)
    for band in (21, 31):
        with pytest.raises(mf.MitoFilterError, match="band"):
            mf.align_reads(ks, reads, band)
        with pytest.raises(mf.MitoFilterError, match="band"):
            mf.filter_fastq_files_aligned(ks, "no_such.fq", None, "o.fq", None, band=band)
    assert mf.align_reads(ks, reads, 20).align is not None
    ks.close()
    prot = mf.KmerSet.protein_from_text(make_protein_bait()[0], 9)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.align_reads(prot, reads, 4)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.filter_fastq_files_aligned(prot, "no_such.fq", None, "o.fq", None, band=4)
    prot.close(); reads.close()
