"""The pile-up entry points of the C ABI without a GPU: the symbols load and are exported, the record types have the stated layout, NULL
handles and min_depth = 0 are refused with MF_E_ARG before any device is touched, `fastfilter bait --pileup / --consensus / --variants`
exits non-zero without a device and 1 when combined with another report (before the library is loaded), and the two host helpers
mitofilter.consensus_fasta and mitofilter.pileup_variants work on hand-made arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_pileup", "mf_filter_fastq_files_pileup", "mf_kmerset_bait_letters")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    assert callable(mitofilter.pileup_reads) and callable(mitofilter.filter_fastq_files_pileup)
    assert isinstance(mitofilter.KmerSet.bait_letters, property)
    assert mitofilter.PILEUP.names == ("a", "c", "g", "t") and mitofilter.PILEUP.itemsize == 16
    assert all(mitofilter.PILEUP[f] == np.uint32 for f in mitofilter.PILEUP.names)
    assert mitofilter.PILEUP_RECORD.names == ("bases", "matches", "mismatches", "called", "ambiguous", "variants")
    assert mitofilter.PILEUP_RECORD.itemsize == 48
    assert lib.mf_abi_version() == 5


def test_null_handles_and_min_depth_0_are_refused(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    pile = (C.c_uint32 * 8)(*([4] * 8))
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 12)(*([3] * 12))
    unplaced = (C.c_uint64 * 2)(6, 6)
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)
    assert lib.mf_pileup(None, None, 1, 0, 1, bits, pile, cons, recs, unplaced, None) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()
    assert lib.mf_filter_fastq_files_pileup(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, 1, pile, cons, recs, unplaced, C.byref(kept),
                                            C.byref(total)) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()
    assert lib.mf_pileup(None, None, 1, 0, 0, bits, pile, cons, recs, unplaced, None) == MF_E_ARG
    assert b"min_depth" in lib.mf_last_error()
    assert lib.mf_filter_fastq_files_pileup(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, 0, pile, cons, recs, unplaced, C.byref(kept),
                                            C.byref(total)) == MF_E_ARG
    assert b"min_depth" in lib.mf_last_error()
    need = C.c_size_t(77)
    assert lib.mf_kmerset_bait_letters(None, cons, 4, C.byref(need)) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error() and need.value == 77
    assert list(bits) == [9, 9] and list(pile) == [4] * 8 and list(cons) == [5] * 4 and list(recs) == [3] * 12
    assert list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


FLAG_SETS = (["--pileup", "p.tsv"], ["--consensus", "c.fa"], ["--variants", "v.tsv"], ["--variants", "v.tsv", "--min-depth", "3"],
             ["--pileup", "p.tsv", "--consensus", "c.fa", "--variants", "v.tsv", "--min-depth", "2"])


def _paths(tmp_path, extra):
    return [str(tmp_path / a) if a.endswith((".tsv", ".fa")) else a for a in extra]


def test_cli_pileup_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for extra in FLAG_SETS:
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq")] + _paths(tmp_path, extra), capture_output=True,
                           env=env, timeout=120)
        assert p.returncode != 0 and p.stdout == b"", p.stderr


@pytest.mark.parametrize("extra", [
    ["--pileup", "p.tsv", "--protein"],
    ["--pileup", "p.tsv", "--report", "r.tsv"],
    ["--pileup", "p.tsv", "--depth-report", "k.tsv"],
    ["--pileup", "p.tsv", "--place-report", "d.tsv"],
    ["--pileup", "p.tsv", "--group-report", "g.tsv"],
    ["--pileup", "p.tsv", "--depth-profile", "k.tsv"],
    ["--pileup", "p.tsv", "--base-depth", "b.tsv"],
    ["--consensus", "c.fa", "--protein"],
    ["--consensus", "c.fa", "--place-report", "d.tsv"],
    ["--variants", "v.tsv", "--report", "r.tsv"],
    ["--protein", "--variants", "v.tsv"],
    ["--min-depth", "3"],                                                   # nothing that uses it
    ["--pileup", "p.tsv", "--min-depth", "0"],
    ["--pileup", "p.tsv", "--min-depth", "-2"],
    ["--pileup", "p.tsv", "--min-depth", "three"],
    ["--pileup", "p.tsv", "--min-depth"],                                   # no value
    ["--pileup"],
    ["--consensus"],
    ["--variants"],
])
def test_cli_pileup_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                       + _paths(tmp_path, extra), capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") or n == "c.fa" for n in os.listdir(str(tmp_path)))


def test_cli_pileup_flags_reach_the_library(built_lib, tmp_path):
    """well-formed pile-up arguments, any flag alone, get as far as loading the library (exit 2 on a missing one)"""
    bait, fq = _inputs(tmp_path)
    for extra in FLAG_SETS:
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                           + _paths(tmp_path, extra), capture_output=True, timeout=60)
        assert p.returncode == 2 and b"no_such_library" in p.stderr


def test_cli_usage_names_the_flags(built_lib):
    p = subprocess.run([CLI, "bait"], capture_output=True, timeout=60)
    assert p.returncode == 1
    for flag in (b"--pileup", b"--consensus", b"--variants", b"--min-depth"):
        assert flag in p.stderr


# ------------------------------------------------------------------ host helpers
def test_consensus_fasta_on_hand_made_arrays():
    from mitoflex_amd import mitofilter as mf
    names = ["first", "", "empty", "exact", "last"]
    seqs = ["ACGTNacgtn" * 7 + "AC", "GG", "", "T" * 120, "acg"]          # 72 letters; 2; none; exactly two full lines; 3
    starts = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    cons = np.frombuffer("".join(seqs).encode(), np.uint8)
    text = mf.consensus_fasta(names, starts, cons)
    assert text == (">first\n" + seqs[0][:60] + "\n" + seqs[0][60:] + "\n>\nGG\n>empty\n>exact\n" + "T" * 60 + "\n" + "T" * 60 + "\n>last\nacg\n")
    # a line wrap exactly at width: no empty line behind a full one
    assert mf.consensus_fasta(["exact"], [0, 120], b"T" * 120, width=40) == ">exact\n" + ("T" * 40 + "\n") * 3
    assert mf.consensus_fasta(["x"], [0, 5], b"ACGTA", width=5) == ">x\nACGTA\n"
    assert mf.consensus_fasta(["x"], [0, 5], b"ACGTA", width=4) == ">x\nACGT\nA\n"
    assert mf.consensus_fasta([], [0], b"") == ""
    assert mf.consensus_fasta(["only"], [0, 0], np.zeros(0, np.uint8)) == ">only\n"
    with pytest.raises(ValueError):
        mf.consensus_fasta(["x"], [0, 5], b"ACGTA", width=0)
    with pytest.raises(ValueError):
        mf.consensus_fasta(["x", "y"], [0, 5], b"ACGTA")
    with pytest.raises(ValueError):
        mf.consensus_fasta(["x"], [0, 6], b"ACGTA")


def test_pileup_variants_on_hand_made_arrays():
    from mitoflex_amd import mitofilter as mf
    # records: r0 = positions 0..5, r1 empty, r2 = positions 6..8
    starts = np.array([0, 6, 6, 9], np.uint64)
    letters = np.frombuffer(b"ACGNTA" + b"GGT", np.uint8)
    rows = [(5, 0, 0, 0),          # 0  called A = ref: no variant
            (1, 4, 0, 0),          # 1  ref C, called C: no variant
            (0, 0, 1, 6),          # 2  ref G, called T: variant, depth 7, alt count 6
            (0, 3, 0, 0),          # 3  invalid bait letter, called C: no variant
            (2, 0, 2, 0),          # 4  a tie: N
            (0, 1, 0, 0),          # 5  below min_depth 2: the bait's letter in lower case
            (0, 0, 0, 0),          # 6  no base at all
            (9, 0, 0, 1),          # 7  ref G, called A: variant
            (0, 2, 0, 1)]          # 8  ref T, called C: variant at the last position of the last record
    pile = np.array(rows, dtype=mf.PILEUP)
    cons = np.frombuffer(b"ACTCNa" + b"gAC", np.uint8)
    v = mf.pileup_variants(starts, letters, pile, cons)
    assert v.dtype.names == ("record", "pos", "ref", "alt", "depth", "alt_count")
    assert [(int(r["record"]), int(r["pos"]), r["ref"], r["alt"], int(r["depth"]), int(r["alt_count"])) for r in v] == [
        (0, 2, b"G", b"T", 7, 6), (2, 1, b"G", b"A", 10, 9), (2, 2, b"T", b"C", 3, 2)]
    # bytes are taken as well as arrays; no variants gives an empty array of the same type
    assert mf.pileup_variants(starts, bytes(letters), pile, bytes(cons)).tolist() == v.tolist()
    none = mf.pileup_variants(starts, letters, pile, np.frombuffer(b"acgntaggt", np.uint8))
    assert len(none) == 0 and none.dtype == v.dtype
    assert len(mf.pileup_variants([0], b"", np.zeros(0, mf.PILEUP), b"")) == 0
    with pytest.raises(ValueError):
        mf.pileup_variants(starts, letters[:5], pile, cons)


def test_bim_consensus_bait_arguments_are_checked(tmp_path):
    from mitoflex_amd.bim import bim
    assert callable(bim.consensus_bait)
    fa = str(tmp_path / "bait.fa")
    with pytest.raises(ValueError):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), min_depth=0)
    with pytest.raises(ValueError):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), kmer=0)
    with pytest.raises(ValueError):
        bim.consensus_bait(fa, "a.fq", None, fa)
    assert not os.path.exists(str(tmp_path / "out.fa"))
