"""The banded-alignment entry points of the C ABI without a GPU: the two symbols load and are exported, the record types have the stated
layout, NULL handles, band = 32, keep = 3, max_permille = 1001 and min_depth = 0 are refused with MF_E_ARG and a message that names the
argument before any device is touched, the wrappers check band before the library, `fastfilter bait --band / --indels` exits 1 on a
command line that cannot be run (before the library is loaded) and gets as far as loading it otherwise, the two text writers of
mf_report_text.h give the texts tests/align_text.py states, and mf.indel_variants lists what it says.  band >= k and a protein set need a
set, and a set needs a device: tests/test_gpu_align.py holds those two."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_align", "mf_filter_fastq_files_aligned")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
        assert name in open(os.path.join(ROOT, "include", "mitofilter.h")).read()
    assert callable(mitofilter.align_reads) and callable(mitofilter.filter_fastq_files_aligned) and callable(mitofilter.indel_variants)
    assert mitofilter.ALIGN.names == ("compared", "mismatches", "insertions", "deletions", "ref_begin", "ref_end") and mitofilter.ALIGN.itemsize == 24
    assert all(mitofilter.ALIGN[f] == np.uint32 for f in mitofilter.ALIGN.names[:4]) and all(mitofilter.ALIGN[f] == np.int32 for f in mitofilter.ALIGN.names[4:])
    assert mitofilter.INDEL.names == ("del", "ins", "ins_bases") and mitofilter.INDEL.itemsize == 12
    assert mitofilter.ALIGN_RECORD.names == ("accepted", "rejected", "compared", "mismatches", "insertions", "deletions", "gapped", "hist")
    assert mitofilter.ALIGN_RECORD.itemsize == 8 * 39 and mitofilter.ALIGN_RECORD["hist"].shape == (32,)
    a = mitofilter.Aligned(kept=3, total=4)
    assert (a.kept, a.total, a.align, a.indels, a.score, a.keep_bits) == (3, 4, None, None, None, None)
    assert isinstance(a, mitofilter.Verified)
    assert lib.mf_abi_version() == 5


def test_null_handles_and_bad_arguments_are_refused(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    keep_bits = (C.c_uint32 * 2)(5, 5)
    place = (C.c_uint32 * 6)(*([8] * 6))
    align = (C.c_uint32 * 6)(*([7] * 6))
    depth = (C.c_uint32 * 4)(2, 2, 2, 2)
    precs = (C.c_uint64 * 6)(*([1] * 6))
    pile = (C.c_uint32 * 8)(*([4] * 8))
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 6)(*([3] * 6))
    indels = (C.c_uint32 * 12)(*([11] * 12))
    arecs = (C.c_uint64 * 39)(*([10] * 39))
    unplaced = (C.c_uint64 * 2)(6, 6)
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)

    def resident(min_depth, max_permille, keep, band):
        return lib.mf_align(None, None, 1, 0, min_depth, max_permille, keep, band, bits, keep_bits, place, align, depth, precs, pile, cons, recs, indels, arecs,
                            unplaced, None)

    def files(min_depth, max_permille, keep, band):
        return lib.mf_filter_fastq_files_aligned(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, min_depth, max_permille, keep, band, depth, precs, pile, cons,
                                                 recs, indels, arecs, unplaced, C.byref(kept), C.byref(total))

    for call in (resident, files):
        assert call(1, 1000, 0, 8) == MF_E_ARG
        assert b"NULL" in lib.mf_last_error()
        assert call(1, 1001, 0, 8) == MF_E_ARG
        assert b"max_permille" in lib.mf_last_error()
        assert call(0, 30, 0, 8) == MF_E_ARG
        assert b"min_depth" in lib.mf_last_error()
        for keep in (3, -1):
            assert call(1, 30, keep, 8) == MF_E_ARG
            assert b"keep" in lib.mf_last_error()
        for band in (32, 0xFFFFFFFF):
            assert call(1, 30, 0, band) == MF_E_ARG
            assert b"band" in lib.mf_last_error()
        assert call(1, 30, 2, 31) == MF_E_ARG and b"NULL" in lib.mf_last_error()          # (31 is a band: the handle is what is wrong)
    assert list(bits) == [9, 9] and list(keep_bits) == [5, 5] and list(place) == [8] * 6 and list(align) == [7] * 6 and list(depth) == [2] * 4
    assert list(precs) == [1] * 6 and list(pile) == [4] * 8 and list(cons) == [5] * 4 and list(recs) == [3] * 6 and list(indels) == [11] * 12
    assert list(arecs) == [10] * 39 and list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)


def test_the_wrappers_check_before_the_library(tmp_path):
    from mitoflex_amd import mitofilter
    from mitoflex_amd.bim import bim
    for band in (32, -1):
        with pytest.raises(ValueError, match="band"):
            mitofilter.align_reads(None, None, band=band)
        with pytest.raises(ValueError, match="band"):
            mitofilter.filter_fastq_files_aligned(None, "a.fq", None, "o.fq", None, band=band)
    with pytest.raises(ValueError, match="max_permille"):
        mitofilter.align_reads(None, None, max_permille=1001)
    with pytest.raises(ValueError, match="keep"):
        mitofilter.filter_fastq_files_aligned(None, "a.fq", None, "o.fq", None, keep=3)
    fa = str(tmp_path / "bait.fa")
    for band, kmer in ((32, 41), (21, 21), (-1, 31)):
        with pytest.raises(ValueError, match="band"):
            bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), kmer=kmer, band=band)
        with pytest.raises(ValueError, match="band"):
            bim.kmer_bait_map(1, fa, str(tmp_path), "p", "a.fq", "b.fq", kmer=kmer, keep=1, band=band)
    with pytest.raises(ValueError, match="keep"):
        bim.kmer_bait_map(1, fa, str(tmp_path), "p", "a.fq", "b.fq", band=8)
    assert not os.path.exists(str(tmp_path / "out.fa"))


def test_indel_variants_lists_the_positions_that_reach_the_cut():
    from mitoflex_amd import mitofilter as mf
    starts = np.array([0, 5, 5, 9], np.uint64)
    depth = np.array([10, 10, 0, 4, 2, 8, 8, 8, 1], np.uint32)
    indels = np.zeros(9, mf.INDEL)
    indels["del"] = [5, 4, 0, 0, 2, 0, 8, 0, 1]
    indels["ins"] = [0, 0, 0, 4, 0, 3, 0, 0, 0]
    indels["ins_bases"] = [0, 0, 0, 9, 0, 3, 0, 0, 0]
    v = mf.indel_variants(starts, depth, indels, min_depth=2, min_permille=500)
    assert v["record"].tolist() == [0, 0, 0, 2] and v["pos"].tolist() == [0, 3, 4, 1]
    assert v["depth"].tolist() == [10, 4, 2, 8] and v["del"].tolist() == [5, 0, 2, 8] and v["ins"].tolist() == [0, 4, 0, 0] and v["ins_bases"].tolist() == [0, 9, 0, 0]
    assert mf.indel_variants(starts, depth, indels, min_depth=1, min_permille=1000)["pos"].tolist() == [3, 4, 1, 3]
    assert len(mf.indel_variants(starts, depth, indels, min_depth=11)) == 0
    with pytest.raises(ValueError, match="min_depth"):
        mf.indel_variants(starts, depth, indels, min_depth=0)
    with pytest.raises(ValueError, match="one entry per position"):
        mf.indel_variants(starts, depth[:8], indels)


def test_the_text_writers_give_the_stated_formats(tmp_path):
    rng = np.random.RandomState(5)
    names, starts = ["mito", "empty", "rec_2"], [0, 7, 7, 12]
    recs = rng.randint(0, 5000, size=(3, 39)).astype(np.int64)
    recs[1] = 0
    recs[2, 2:7] = (1000, 3, 2, 1, 3)                                   # 6 edits on 1003 columns: 5.982
    depth = rng.randint(0, 40, size=12)
    indels = rng.randint(0, 3, size=(12, 3)) * (rng.rand(12, 1) < 0.5)
    indels[0], indels[11] = (1, 0, 0), (0, 2, 5)
    case = str(tmp_path / "case.txt")
    with open(case, "w") as f:
        f.write("3\n%s\n%s\n" % (" ".join(names), " ".join(map(str, starts))))
        f.writelines(" ".join(map(str, row)) + "\n" for row in recs.tolist())
        f.writelines("%d %d %d %d\n" % (depth[p], *indels[p]) for p in range(12))
    exe = str(tmp_path / "align_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "align_text_check.cpp"), "-o", exe])
    r = subprocess.run([exe, case, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "the writers returned true\n", (r.stdout, r.stderr[-3000:])
    want = align_text.align_report_text(names, starts, recs)
    assert open(str(tmp_path / "align.tsv")).read() == want
    assert want.splitlines()[3].split("\t")[:11] == ["2", "rec_2", "5"] + [str(v) for v in recs[2, :2]] + ["1000", "3", "2", "1", "3", "5.982"]
    assert want.splitlines()[2].split("\t")[10] == "0.000" and want.splitlines()[0].endswith("\ted30\ted31+")
    want = align_text.indels_text(names, starts, depth, indels)
    assert open(str(tmp_path / "indels.tsv")).read() == want
    assert want.splitlines()[1] == "mito\t1\t%d\t1\t0\t0" % depth[0] and want.splitlines()[-1] == "rec_2\t5\t%d\t0\t2\t5" % depth[11]


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


def _paths(tmp_path, extra):
    return [str(tmp_path / a) if a.endswith((".tsv", ".fa")) else a for a in extra]


def _run(tmp_path, bait, fq, extra, env=None, lib=True):
    return subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq")]
                          + (["--lib", str(tmp_path / "no_such_library.so")] if lib else []) + _paths(tmp_path, extra), capture_output=True, timeout=120, env=env)


FLAG_SETS = (["--band", "8", "--score-report", "s.tsv"],
             ["--band", "0", "--indels", "i.tsv"],
             ["--band", "31", "-k", "32", "--write", "accepted", "--max-mismatch", "30"],
             ["--band", "8", "--indels", "i.tsv", "--score-report", "s.tsv", "--consensus", "c.fa", "--variants", "v.tsv", "--min-depth", "3"],
             ["--band", "4", "--place-report", "d.tsv", "--base-depth", "b.tsv"])


@pytest.mark.parametrize("extra", [
    ["--band", "8"],                                                         # nothing that uses it
    ["--band", "8", "--report", "r.tsv"],
    ["--band", "8", "--depth-report", "k.tsv"],
    ["--band", "8", "--score-report", "s.tsv", "--protein"],
    ["--band", "32", "--score-report", "s.tsv"],
    ["--band", "-1", "--score-report", "s.tsv"],
    ["--band", "eight", "--score-report", "s.tsv"],
    ["--band", "8x", "--score-report", "s.tsv"],
    ["--band", "", "--score-report", "s.tsv"],
    ["--score-report", "s.tsv", "--band"],                                   # no value
    ["--band", "31", "--score-report", "s.tsv"],                             # not below k = 31
    ["--band", "21", "-k", "21", "--score-report", "s.tsv"],
    ["--indels", "i.tsv"],                                                   # no band
    ["--indels", "i.tsv", "--score-report", "s.tsv", "--max-mismatch", "30"],
    ["--band", "8", "--indels"],
])
def test_cli_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, extra)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert b"no_such_library" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") or n == "c.fa" for n in os.listdir(str(tmp_path)))


def test_cli_flags_reach_the_library(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    for extra in FLAG_SETS:
        p = _run(tmp_path, bait, fq, extra)
        assert p.returncode == 2 and b"no_such_library" in p.stderr, (extra, p.stderr)


def test_cli_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, FLAG_SETS[0], env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), lib=False)
    assert p.returncode != 0 and p.stdout == b"", p.stderr


def test_cli_usage_names_the_flags(built_lib):
    p = subprocess.run([CLI, "bait"], capture_output=True, timeout=60)
    assert p.returncode == 1
    for flag in (b"--band", b"--indels"):
        assert flag in p.stderr
