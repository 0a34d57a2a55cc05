"""The group-assignment entry points of the C ABI without a GPU: the symbols load, NULL handles and pointers are refused with MF_E_ARG
before any device is touched, and the argument errors of `fastfilter bait --group-report` exit 1 before the library is loaded."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_kmerset_group_records", "mf_kmerset_group_count", "mf_kmerset_group_name", "mf_assign_groups", "mf_filter_fastq_files_by_group")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    for name in ("group_records", "group_names"):
        assert hasattr(mitofilter.KmerSet, name)
    assert callable(mitofilter.assign_groups) and callable(mitofilter.filter_fastq_files_by_group)


def test_null_handles_and_pointers_are_refused(lib):
    assert lib.mf_kmerset_group_records(None, b"_", 4) == MF_E_ARG
    assert lib.mf_kmerset_group_records(None, None, 0) == MF_E_ARG
    n = C.c_uint64(7)
    assert lib.mf_kmerset_group_count(None, C.byref(n)) == MF_E_ARG and n.value == 7
    need = C.c_size_t(0)
    assert lib.mf_kmerset_group_name(None, 0, C.create_string_buffer(8), 8, C.byref(need)) == MF_E_ARG
    assert lib.mf_assign_groups(None, None, 1, 0, None, None, None, None) == MF_E_ARG
    counts = (C.c_uint64 * 4)()
    dev = (C.c_int * 1)(0)
    assert lib.mf_filter_fastq_files_by_group(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, counts, None, None) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()


def _inputs(tmp_path):
    from tests.util_data import make_protein_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_protein_bait()[0])
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


@pytest.mark.parametrize("extra", [
    ["--report", "r.tsv", "--group-report", "g.tsv"],                       # both reports
    ["--protein", "--report", "r.tsv", "--group-report", "g.tsv"],
    ["--group-field", "4"],                                                 # grouping without a group report
    ["--group-sep", "_"],
    ["--report", "r.tsv", "--group-field", "4"],
    ["--group-report", "g.tsv", "--group-field", "0"],                      # fields count from 1
    ["--group-report", "g.tsv", "--group-field", "x"],
    ["--group-report", "g.tsv", "--group-sep", ""],
    ["--group-report"],                                                     # no value
])
def test_cli_argument_errors_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    extra = [str(tmp_path / a) if a.endswith(".tsv") else a for a in extra]
    p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                       + extra, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert not os.path.exists(str(tmp_path / "o.fq"))


def test_cli_group_report_reaches_the_library(built_lib, tmp_path):
    """well-formed --group-report arguments get as far as loading the library (exit 2 on a missing one)"""
    bait, fq = _inputs(tmp_path)
    for extra in (["--protein", "--group-report", str(tmp_path / "g.tsv"), "--group-field", "4", "--group-sep", "_"],
                  ["--group-report", str(tmp_path / "g.tsv")]):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                           + extra, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"no_such_library" in p.stderr
