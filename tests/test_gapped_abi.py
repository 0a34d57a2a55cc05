"""The gapped-consensus entry points without a GPU: the two symbols load and are exported, the record type has the stated layout, NULL
handles and bad arguments are refused with MF_E_ARG before any device is touched and leave every output as it was, the wrappers check
their arguments before the library, `fastfilter bait --gapped-consensus / --insertions` exits 1 on a command line that cannot be run
(before the library is loaded) and gets as far as loading it otherwise, and the two text writers of mf_report_text.h give hand-written
bytes.  band >= k and a protein set need a set, and a set needs a device: tests/test_gpu_gapped.py holds those two."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gapped_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_align_gapped", "mf_filter_fastq_files_gapped")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    header = open(os.path.join(ROOT, "include", "mitofilter.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
        assert name in header
    assert "typedef struct { uint64_t length, deleted, insertions, inserted_bases; } mf_gapped_record_t;" in header
    assert mitofilter.GAPPED_RECORD.names == ("length", "deleted", "insertions", "inserted_bases") and mitofilter.GAPPED_RECORD.itemsize == 32
    assert all(mitofilter.GAPPED_RECORD[f] == np.uint64 for f in mitofilter.GAPPED_RECORD.names)
    assert callable(mitofilter.gapped_consensus)
    a = mitofilter.Aligned(kept=3, total=4)
    assert (a.ins_pile, a.gapped, a.gapped_starts, a.gapped_records, a.indels) == (None, None, None, None, None)
    assert lib.mf_abi_version() == 5
    import inspect
    for f in (mitofilter.align_reads, mitofilter.filter_fastq_files_aligned):
        p = list(inspect.signature(f).parameters.values())[-1]
        assert p.name == "gapped" and p.default is False          # the new keyword stands last


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
    ins = (C.c_uint32 * 16)(*([12] * 16))
    gapped = (C.c_uint8 * 8)(*([13] * 8))
    gstarts = (C.c_uint64 * 2)(14, 14)
    grecs = (C.c_uint64 * 4)(*([15] * 4))
    unplaced = (C.c_uint64 * 2)(6, 6)
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)

    def resident(min_depth, max_permille, keep, band, new=True):
        more = (ins, gapped, gstarts, grecs) if new else (None,) * 4
        return lib.mf_align_gapped(None, None, 1, 0, min_depth, max_permille, keep, band, bits, keep_bits, place, align, depth, precs, pile, cons, recs, indels,
                                   arecs, *more, unplaced, None)

    def files(min_depth, max_permille, keep, band, new=True):
        more = (ins, gapped, gstarts, grecs) if new else (None,) * 4
        return lib.mf_filter_fastq_files_gapped(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, min_depth, max_permille, keep, band, depth, precs, pile,
                                                cons, recs, indels, arecs, *more, unplaced, C.byref(kept), C.byref(total))

    for call in (resident, files):
        for new in (True, False):
            assert call(1, 1000, 0, 8, new) == MF_E_ARG
            assert b"NULL" in lib.mf_last_error()
            assert call(1, 1001, 0, 8, new) == MF_E_ARG
            assert b"max_permille" in lib.mf_last_error()
            assert call(0, 30, 0, 8, new) == MF_E_ARG
            assert b"min_depth" in lib.mf_last_error()
            for keep in (3, -1):
                assert call(1, 30, keep, 8, new) == MF_E_ARG
                assert b"keep" in lib.mf_last_error()
            for band in (32, 0xFFFFFFFF):
                assert call(1, 30, 0, band, new) == MF_E_ARG
                assert b"band" in lib.mf_last_error()
    assert list(bits) == [9, 9] and list(keep_bits) == [5, 5] and list(place) == [8] * 6 and list(align) == [7] * 6 and list(depth) == [2] * 4
    assert list(precs) == [1] * 6 and list(pile) == [4] * 8 and list(cons) == [5] * 4 and list(recs) == [3] * 6 and list(indels) == [11] * 12
    assert list(arecs) == [10] * 39 and list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)
    assert list(ins) == [12] * 16 and list(gapped) == [13] * 8 and list(gstarts) == [14, 14] and list(grecs) == [15] * 4


def test_the_wrappers_check_before_the_library(tmp_path):
    from mitoflex_amd import mitofilter
    from mitoflex_amd.bim import bim
    for band in (32, -1):
        with pytest.raises(ValueError, match="band"):
            mitofilter.align_reads(None, None, band=band, gapped=True)
        with pytest.raises(ValueError, match="band"):
            mitofilter.filter_fastq_files_aligned(None, "a.fq", None, "o.fq", None, band=band, gapped=True)
    with pytest.raises(ValueError, match="min_depth"):
        mitofilter.align_reads(None, None, min_depth=0, gapped=True)
    fa = str(tmp_path / "bait.fa")
    with pytest.raises(ValueError, match="gapped needs a band"):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), gapped=True)
    with pytest.raises(ValueError, match="gapped needs a band"):
        bim.kmer_bait_map(1, fa, str(tmp_path), "p", "a.fq", "b.fq", keep=1, gapped=True)
    with pytest.raises(ValueError, match="band"):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), kmer=21, band=21, gapped=True)
    assert not os.path.exists(str(tmp_path / "out.fa"))
    # gapped_consensus: what it is given has one entry per position
    starts = np.array([0, 3], np.uint64)
    depth, cons = np.zeros(3, np.uint32), np.frombuffer(b"acg", np.uint8)
    indels, ins = np.zeros(3, mitofilter.INDEL), np.zeros((3, 2), mitofilter.PILEUP)
    assert bytes(mitofilter.gapped_consensus(starts, depth, indels, ins, cons)[0]) == b"acg"
    with pytest.raises(ValueError, match="min_depth"):
        mitofilter.gapped_consensus(starts, depth, indels, ins, cons, min_depth=0)
    with pytest.raises(ValueError, match="one entry per position"):
        mitofilter.gapped_consensus(starts, depth[:2], indels, ins, cons)
    with pytest.raises(ValueError, match="PILEUP"):
        mitofilter.gapped_consensus(starts, depth, indels, np.zeros(6, mitofilter.PILEUP), cons)


def test_the_text_writers_give_the_stated_formats(tmp_path):
    names, starts, span = ["mito", "empty", "rec_2"], [0, 3, 3, 5], 2
    gstarts, gapped = [0, 63, 63, 64], "ACGTN" * 12 + "acg" + "T"          # 63 letters: a line of 60 and one of 3; an empty record; one letter
    depth = [7, 0, 4000000000, 9, 2]
    ins = np.zeros((5, span, 4), np.int64)
    ins[0, 1] = (0, 0, 0, 1)                                               # offset 1 alone: still a row
    ins[2, 0] = (4294967294, 1, 2, 3)
    ins[4, 0], ins[4, 1] = (1, 0, 0, 0), (0, 5, 0, 0)
    case = str(tmp_path / "case.txt")
    with open(case, "w") as f:
        f.write("3\n%s\n%s\n%d\n%s\n%s\n" % (" ".join(names), " ".join(map(str, starts)), span, " ".join(map(str, gstarts)), gapped))
        f.writelines("%d %s\n" % (depth[p], " ".join(str(int(v)) for v in ins[p].reshape(-1))) for p in range(5))
    exe = str(tmp_path / "gapped_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "gapped_text_check.cpp"), "-o", exe])
    r = subprocess.run([exe, case, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "the writers returned true\n", (r.stdout, r.stderr[-3000:])
    fasta = open(str(tmp_path / "gapped.fa")).read()
    assert fasta == ">mito\n" + "ACGTN" * 12 + "\nacg\n>empty\n>rec_2\nT\n"
    assert fasta == gapped_text.gapped_fasta(names, gstarts, gapped.encode())
    table = open(str(tmp_path / "insertions.tsv")).read()
    assert table == ("name\tpos\toffset\tdepth\tA\tC\tG\tT\n"
                     "mito\t1\t1\t7\t0\t0\t0\t1\n"
                     "mito\t3\t0\t4000000000\t4294967294\t1\t2\t3\n"
                     "rec_2\t2\t0\t2\t1\t0\t0\t0\n"
                     "rec_2\t2\t1\t2\t0\t5\t0\t0\n")
    assert table == gapped_text.insertions_text(names, starts, depth, ins)


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


def _run(tmp_path, bait, fq, extra):
    paths = [str(tmp_path / a) if a.endswith((".tsv", ".fa")) else a for a in extra]
    return subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")] + paths,
                          capture_output=True, timeout=120)


@pytest.mark.parametrize("extra", [
    ["--gapped-consensus", "g.fa"],                                          # no band
    ["--insertions", "i.tsv"],
    ["--gapped-consensus", "g.fa", "--consensus", "c.fa", "--min-depth", "3"],
    ["--insertions", "i.tsv", "--score-report", "s.tsv", "--max-mismatch", "30"],
    ["--band", "8", "--gapped-consensus"],                                   # no value
    ["--band", "8", "--insertions"],
    ["--band", "8", "--gapped-consensus", "g.fa", "--protein"],
    ["--band", "8", "--insertions", "i.tsv", "--report", "r.tsv"],
    ["--band", "8", "--gapped-consensus", "g.fa", "--depth-report", "k.tsv"],
    ["--band", "31", "--gapped-consensus", "g.fa"],                          # not below k = 31
    ["--band", "8", "--gapped-consensus", "g.fa", "--min-depth", "0"],
])
def test_cli_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, extra)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"error: "), p.stderr
    assert b"no_such_library" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") or n in ("c.fa", "g.fa") for n in os.listdir(str(tmp_path)))


@pytest.mark.parametrize("extra", [
    ["--band", "8", "--gapped-consensus", "g.fa"],
    ["--band", "0", "--insertions", "i.tsv"],
    ["--band", "8", "--gapped-consensus", "g.fa", "--min-depth", "3"],
    ["--band", "30", "--gapped-consensus", "g.fa", "--insertions", "i.tsv", "--indels", "d.tsv", "--consensus", "c.fa", "--write", "accepted", "--max-mismatch", "30"],
])
def test_cli_flags_reach_the_library(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, extra)
    assert p.returncode == 2 and b"no_such_library" in p.stderr, (extra, p.stderr)


def test_cli_usage_names_the_flags(built_lib):
    p = subprocess.run([CLI, "bait"], capture_output=True, timeout=60)
    assert p.returncode == 1
    for flag in (b"--gapped-consensus", b"--insertions"):
        assert flag in p.stderr
