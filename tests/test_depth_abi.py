"""The k-mer depth entry points of the C ABI without a GPU: the symbols load and are exported, NULL handles are refused with MF_E_ARG
before any device is touched, and `fastfilter bait --depth-report` exits non-zero without a device and 1 when combined with another
report (before the library is loaded)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_kmerset_record_starts", "mf_depth", "mf_filter_fastq_files_depth")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    assert hasattr(mitofilter.KmerSet, "record_starts")
    assert callable(mitofilter.record_depth) and callable(mitofilter.filter_fastq_files_depth)
    assert mitofilter.DEPTH_NONE == 0xFFFFFFFF
    assert mitofilter.DEPTH_RECORD.names == ("windows", "covered", "depth_sum", "depth_max")
    assert mitofilter.DEPTH_RECORD.itemsize == 32
    assert lib.mf_abi_version() == 5


def test_null_handles_are_refused(lib):
    starts = (C.c_uint64 * 4)(7, 7, 7, 7)
    need = C.c_size_t(99)
    assert lib.mf_kmerset_record_starts(None, starts, 4, C.byref(need)) == MF_E_ARG
    assert need.value == 99 and list(starts) == [7, 7, 7, 7]
    assert lib.mf_depth(None, None, 1, 0, None, None, None, None) == MF_E_ARG
    prof = (C.c_uint32 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 8)(*([3] * 8))
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)
    assert lib.mf_filter_fastq_files_depth(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, prof, recs, C.byref(kept), C.byref(total)) == MF_E_ARG
    assert list(prof) == [5, 5, 5, 5] and list(recs) == [3] * 8 and (kept.value, total.value) == (11, 12)
    assert b"NULL" in lib.mf_last_error()


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


def test_cli_depth_report_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for extra in (["--depth-report", str(tmp_path / "d.tsv")], ["--depth-profile", str(tmp_path / "p.tsv")],
                  ["--depth-report", str(tmp_path / "d.tsv"), "--depth-profile", str(tmp_path / "p.tsv")]):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq")] + extra, capture_output=True,
                           env=env, timeout=120)
        assert p.returncode != 0 and p.stdout == b"", p.stderr


@pytest.mark.parametrize("extra", [
    ["--depth-report", "d.tsv", "--report", "r.tsv"],
    ["--depth-report", "d.tsv", "--group-report", "g.tsv"],
    ["--depth-profile", "p.tsv", "--report", "r.tsv"],
    ["--depth-profile", "p.tsv", "--group-report", "g.tsv", "--group-field", "4"],
    ["--protein", "--depth-report", "d.tsv", "--group-report", "g.tsv"],
    ["--depth-report"],                                                     # no value
])
def test_cli_depth_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    extra = [str(tmp_path / a) if a.endswith(".tsv") else a for a in extra]
    p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                       + extra, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert not os.path.exists(str(tmp_path / "o.fq"))


def test_cli_depth_flags_reach_the_library(built_lib, tmp_path):
    """well-formed depth arguments, either flag alone, get as far as loading the library (exit 2 on a missing one)"""
    bait, fq = _inputs(tmp_path)
    for extra in (["--depth-report", str(tmp_path / "d.tsv")], ["--depth-profile", str(tmp_path / "p.tsv")],
                  ["--protein", "--depth-report", str(tmp_path / "d.tsv"), "--depth-profile", str(tmp_path / "p.tsv")]):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                           + extra, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"no_such_library" in p.stderr
