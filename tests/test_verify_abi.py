"""The verification entry points of the C ABI without a GPU: the two symbols load and are exported, the record types have the stated
layout, NULL handles, max_permille = 1001 and min_depth = 0 are refused with MF_E_ARG and a message that names the argument before any
device is touched, `fastfilter bait --score-report / --max-mismatch` exits 1 on a command line that cannot be run (before the library
is loaded) and gets as far as loading it otherwise, and bim.consensus_bait checks its max_permille."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_verify", "mf_filter_fastq_files_verified")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    assert callable(mitofilter.verify_reads) and callable(mitofilter.filter_fastq_files_verified)
    assert mitofilter.SCORE.names == ("compared", "mismatches") and mitofilter.SCORE.itemsize == 8
    assert all(mitofilter.SCORE[f] == np.uint32 for f in mitofilter.SCORE.names)
    assert mitofilter.SCORE_RECORD.names == ("accepted", "rejected", "compared", "mismatches", "hist")
    assert mitofilter.SCORE_RECORD.itemsize == 8 * 36 and mitofilter.SCORE_BINS == 32
    assert mitofilter.SCORE_RECORD["hist"].shape == (32,) and mitofilter.SCORE_RECORD["hist"].base == np.uint64
    assert all(mitofilter.SCORE_RECORD[f] == np.uint64 for f in mitofilter.SCORE_RECORD.names[:4])
    v = mitofilter.Verified(kept=3, total=4)
    assert (v.kept, v.total, v.bits, v.score, v.pileup) == (3, 4, None, None, None)
    assert set(mitofilter.Verified.__slots__) == {"bits", "kept", "total", "place", "score", "base_depth", "place_records", "pileup", "consensus",
                                                  "pileup_records", "score_records", "unplaced"}
    with pytest.raises(TypeError):
        mitofilter.Verified(nonsense=1)
    assert lib.mf_abi_version() == 5


def test_null_handles_and_bad_cuts_are_refused(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    place = (C.c_uint32 * 6)(*([8] * 6))
    score = (C.c_uint32 * 2)(7, 7)
    depth = (C.c_uint32 * 4)(2, 2, 2, 2)
    precs = (C.c_uint64 * 6)(*([1] * 6))
    pile = (C.c_uint32 * 8)(*([4] * 8))
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 6)(*([3] * 6))
    srecs = (C.c_uint64 * 36)(*([10] * 36))
    unplaced = (C.c_uint64 * 2)(6, 6)
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)

    def resident(min_depth, max_permille):
        return lib.mf_verify(None, None, 1, 0, min_depth, max_permille, bits, place, score, depth, precs, pile, cons, recs, srecs, unplaced, None)

    def files(min_depth, max_permille):
        return lib.mf_filter_fastq_files_verified(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, min_depth, max_permille, depth, precs, pile, cons,
                                                  recs, srecs, unplaced, C.byref(kept), C.byref(total))

    for call in (resident, files):
        assert call(1, 1000) == MF_E_ARG
        assert b"NULL" in lib.mf_last_error()
        assert call(1, 1001) == MF_E_ARG
        assert b"max_permille" in lib.mf_last_error()
        assert call(0, 30) == MF_E_ARG
        assert b"min_depth" in lib.mf_last_error()
    assert list(bits) == [9, 9] and list(place) == [8] * 6 and list(score) == [7, 7] and list(depth) == [2] * 4 and list(precs) == [1] * 6
    assert list(pile) == [4] * 8 and list(cons) == [5] * 4 and list(recs) == [3] * 6 and list(srecs) == [10] * 36
    assert list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)


def test_the_wrapper_checks_the_cut_before_the_library():
    from mitoflex_amd import mitofilter
    with pytest.raises(ValueError, match="max_permille"):
        mitofilter.verify_reads(None, None, max_permille=1001)
    with pytest.raises(ValueError, match="min_depth"):
        mitofilter.filter_fastq_files_verified(None, "a.fq", None, "o.fq", None, min_depth=0)


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


def _paths(tmp_path, extra):
    return [str(tmp_path / a) if a.endswith((".tsv", ".fa")) else a for a in extra]


FLAG_SETS = (["--score-report", "s.tsv"],
             ["--score-report", "s.tsv", "--max-mismatch", "30"],          # (its accepted / rejected columns are the cut's)
             ["--score-report", "s.tsv", "--place-report", "d.tsv", "--max-mismatch", "30"],
             ["--score-report", "s.tsv", "--pileup", "p.tsv", "--consensus", "c.fa", "--variants", "v.tsv", "--min-depth", "3", "--max-mismatch", "0"],
             ["--base-depth", "b.tsv", "--max-mismatch", "1000"],
             ["--consensus", "c.fa", "--max-mismatch", "30"],
             ["--score-report", "s.tsv", "--variants", "v.tsv"])


@pytest.mark.parametrize("extra", [
    ["--max-mismatch", "30"],                                                # nothing that uses it
    ["--max-mismatch", "30", "--report", "r.tsv"],
    ["--max-mismatch", "30", "--depth-report", "k.tsv"],
    ["--pileup", "p.tsv", "--max-mismatch", "1001"],
    ["--pileup", "p.tsv", "--max-mismatch", "-1"],
    ["--pileup", "p.tsv", "--max-mismatch", "thirty"],
    ["--pileup", "p.tsv", "--max-mismatch", "30x"],
    ["--pileup", "p.tsv", "--max-mismatch", ""],
    ["--place-report", "d.tsv", "--max-mismatch"],                           # no value
    ["--score-report"],
    ["--score-report", "s.tsv", "--protein"],
    ["--score-report", "s.tsv", "--report", "r.tsv"],
    ["--score-report", "s.tsv", "--group-report", "g.tsv"],
    ["--score-report", "s.tsv", "--depth-report", "k.tsv"],
    ["--score-report", "s.tsv", "--depth-profile", "k.tsv"],
    ["--score-report", "s.tsv", "--pileup", "p.tsv", "--place-report", "d.tsv"],          # the two families stay exclusive of each other
    ["--score-report", "s.tsv", "--consensus", "c.fa", "--base-depth", "b.tsv", "--max-mismatch", "30"],
])
def test_cli_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                       + _paths(tmp_path, extra), capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert b"no_such_library" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") or n == "c.fa" for n in os.listdir(str(tmp_path)))


def test_cli_flags_reach_the_library(built_lib, tmp_path):
    """well-formed arguments -- the score report alone and with either family, the cut with either family -- get as far as loading the
    library (exit 2 on a missing one)"""
    bait, fq = _inputs(tmp_path)
    for extra in FLAG_SETS:
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                           + _paths(tmp_path, extra), capture_output=True, timeout=60)
        assert p.returncode == 2 and b"no_such_library" in p.stderr, (extra, p.stderr)


def test_cli_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for extra in FLAG_SETS[:2]:
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq")] + _paths(tmp_path, extra), capture_output=True,
                           env=env, timeout=120)
        assert p.returncode != 0 and p.stdout == b"", p.stderr


def test_cli_usage_names_the_flags(built_lib):
    p = subprocess.run([CLI, "bait"], capture_output=True, timeout=60)
    assert p.returncode == 1
    for flag in (b"--score-report", b"--max-mismatch"):
        assert flag in p.stderr


def test_bim_consensus_bait_checks_max_permille(tmp_path):
    import inspect
    from mitoflex_amd.bim import bim
    assert inspect.signature(bim.consensus_bait).parameters["max_permille"].default is None
    fa = str(tmp_path / "bait.fa")
    for bad in (1001, -1):
        with pytest.raises(ValueError, match="max_permille"):
            bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), max_permille=bad)
    assert not os.path.exists(str(tmp_path / "out.fa"))
