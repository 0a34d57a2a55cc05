"""The text writers of the extended records (mf_report_text.h) against tests/extend_text.py and hand-written bytes, without a device: a
stand-alone program (tests/native/extend_text_check.cpp) under ASan + UBSan.  And `fastfilter bait`'s three new flags: a command line
that cannot be run exits 1 before the library is loaded, one that can gets as far as loading it."""
import os
import subprocess

import numpy as np
import pytest

from tests import extend_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")


def test_the_text_writers_give_the_stated_formats(tmp_path):
    names, E = ["mito", "empty", "rec_2"], 3
    xstarts, extended = [0, 63, 63, 64], "ACGTN" * 12 + "acg" + "T"          # 63 letters: a line of 60 and one of 3; an empty record; one letter
    ext = np.zeros((3, 2, E, 4), np.int64)
    ext[0, 0, 2] = (0, 0, 0, 1)                                               # the farthest column alone: still a row
    ext[0, 1, 0] = (4294967294, 4294967294, 2, 3)                             # clamped counts: the depth is their 64-bit sum
    ext[2, 0, 0], ext[2, 1, 1] = (1, 0, 0, 0), (0, 5, 0, 0)
    case = str(tmp_path / "case.txt")
    with open(case, "w") as f:
        f.write("3\n%s\n%d\n%s\n%s\n" % (" ".join(names), E, " ".join(map(str, xstarts)), extended))
        f.writelines("%s\n" % " ".join(str(int(v)) for v in ext[j, side].reshape(-1)) for j in range(3) for side in (0, 1))
    exe = str(tmp_path / "extend_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "extend_text_check.cpp"), "-o", exe])
    r = subprocess.run([exe, case, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "the writers returned true\n", (r.stdout, r.stderr[-3000:])
    fasta = open(str(tmp_path / "extended.fa")).read()
    assert fasta == ">mito\n" + "ACGTN" * 12 + "\nacg\n>empty\n>rec_2\nT\n"
    assert fasta == extend_text.extended_fasta(names, xstarts, extended.encode())
    table = open(str(tmp_path / "extension.tsv")).read()
    assert table == ("name\tend\toffset\tdepth\tA\tC\tG\tT\n"
                     "mito\tbegin\t3\t1\t0\t0\t0\t1\n"
                     "mito\tend\t1\t8589934593\t4294967294\t4294967294\t2\t3\n"
                     "rec_2\tbegin\t1\t1\t1\t0\t0\t0\n"
                     "rec_2\tend\t2\t5\t0\t5\t0\t0\n")
    assert table == extend_text.extension_text(names, ext)


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
    ["--extend", "16"],                                                              # no band
    ["--extend", "16", "--extended-consensus", "x.fa"],
    ["--band", "8", "--extended-consensus", "x.fa"],                                 # no --extend
    ["--band", "8", "--extension-report", "x.tsv"],
    ["--band", "8", "--extend"],                                                     # no value
    ["--band", "8", "--extend", "0", "--extended-consensus", "x.fa"],
    ["--band", "8", "--extend", "4097", "--extended-consensus", "x.fa"],
    ["--band", "8", "--extend", "-3", "--extended-consensus", "x.fa"],
    ["--band", "8", "--extend", "16", "--extended-consensus"],
    ["--band", "8", "--extend", "16", "--extended-consensus", "x.fa", "--protein"],
    ["--band", "8", "--extend", "16", "--extension-report", "x.tsv", "--report", "r.tsv"],
    ["--band", "31", "--extend", "16", "--extended-consensus", "x.fa"],              # not below k = 31
    ["--band", "8", "--extend", "16", "--extended-consensus", "x.fa", "--min-depth", "0"],
])
def test_cli_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, extra)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"error: "), p.stderr
    assert b"no_such_library" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") or n == "x.fa" for n in os.listdir(str(tmp_path)))


@pytest.mark.parametrize("extra", [
    ["--band", "0", "--extend", "16"],
    ["--band", "0", "--extend", "16", "--extended-consensus", "x.fa"],
    ["--band", "8", "--extend", "4096", "--extension-report", "x.tsv", "--min-depth", "3", "--extended-consensus", "x.fa"],
    ["--band", "30", "--extend", "64", "--extended-consensus", "x.fa", "--gapped-consensus", "g.fa", "--insertions", "i.tsv", "--indels", "d.tsv", "--consensus", "c.fa",
     "--write", "accepted", "--max-mismatch", "30"],
])
def test_cli_flags_reach_the_library(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    p = _run(tmp_path, bait, fq, extra)
    assert p.returncode == 2 and b"no_such_library" in p.stderr, (extra, p.stderr)


def test_cli_usage_names_the_flags(built_lib):
    p = subprocess.run([CLI, "bait"], capture_output=True, timeout=60)
    assert p.returncode == 1
    for flag in (b"--extend E", b"--extended-consensus", b"--extension-report"):
        assert flag in p.stderr
