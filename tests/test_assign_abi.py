"""The record-assignment entry points of the C ABI without a GPU: the symbols load, NULL handles are refused with MF_E_ARG before any
device is touched, and `fastfilter bait --report` fails cleanly (no device: non-zero exit, nothing on stdout; with --protein: exit 1 before
the library is loaded)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mf_kmerset_record_count", "mf_kmerset_record_name", "mf_assign", "mf_filter_fastq_files_by_record")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    assert mitofilter.ASSIGN_AMBIGUOUS == 0xFFFFFFFE and mitofilter.ASSIGN_NONE == 0xFFFFFFFF


def test_null_handles_are_refused(lib):
    n = C.c_uint64(7)
    assert lib.mf_kmerset_record_count(None, C.byref(n)) == MF_E_ARG and n.value == 7
    need = C.c_size_t(0)
    assert lib.mf_kmerset_record_name(None, 0, C.create_string_buffer(8), 8, C.byref(need)) == MF_E_ARG
    assert lib.mf_assign(None, None, 1, 0, None, None, None, None) == MF_E_ARG
    counts = (C.c_uint64 * 4)()
    dev = (C.c_int * 1)(0)
    assert lib.mf_filter_fastq_files_by_record(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, counts, None, None) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()


def _inputs(tmp_path):
    from tests.util_data import make_bait, make_reads, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, make_reads(make_bait(), 50, seed=1), "a")
    return bait, fq


def test_cli_report_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    cli = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")          # (no device, also where the suite runs on a GPU box)
    p = subprocess.run([cli, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--report", str(tmp_path / "r.tsv")],
                       capture_output=True, env=env, timeout=120)
    assert p.returncode != 0 and p.stdout == b""


def test_cli_report_with_protein_exits_before_loading(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    cli = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
    p = subprocess.run([cli, "bait", "--protein", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--report", str(tmp_path / "r.tsv"),
                        "--lib", str(tmp_path / "no_such_library.so")], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"--protein" in p.stderr and p.stdout == b""          # (a library that cannot be loaded exits 2)
    p = subprocess.run([cli, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--report"], capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
