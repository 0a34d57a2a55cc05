"""The keep rule on the host pipeline without a GPU (tests/native/keep_check.cpp): a stand-in report amends each mate batch's pass bits
through PassReport::amend_bits -- the one door the ingest paths open for it -- with mf_score.h's keep_clears, and the written files and
`kept` are what the obvious Python computes from the FASTQ text.  Stand-in rules: a read passes iff its first base is A/a; a passing
read whose second base is C/c is "placed and rejected", one whose second base is G/g is "not placed"."""
import os
import random
import subprocess

import pytest

from tests.util_data import write_fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitoflex_amd", "csrc")
SRCS = ["mf_pipeline.cpp", "mf_host.cpp", "mf_inflate.cpp", "mf_pinflate.cpp"]
SANITIZERS = [("-fsanitize=address,undefined", "-fno-omit-frame-pointer"), ("-fsanitize=thread",)]


def build(tmp, name, flags=()):
    exe = os.path.join(str(tmp), name + "_".join(f.replace("=", "").replace(",", "") for f in flags))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "native", name + ".cpp"),
                           *[os.path.join(CSRC, s) for s in SRCS], "-lz", "-lpthread", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """600 and 640 records (pairs end with the shorter file); every stand-in class among the passing reads, reads of 0 and 1 bases,
    an N at the first and at the second base, lower case; and what pipeline_check (no report at all) writes for them."""
    d = tmp_path_factory.mktemp("keep")
    rng = random.Random(7)

    def seqs(n):
        out = []
        for _ in range(n):
            L = rng.choice([150, 151, 40, 2, 1, 0, 77])
            s = "".join(rng.choices("ACGT", k=L))
            if L and rng.random() < 0.6:
                s = rng.choice("Aa") + s[1:]
            if L > 1 and rng.random() < 0.15:
                s = s[0] + "N" + s[2:]
            if L and rng.random() < 0.05:
                s = "N" + s[1:]
            out.append(s if rng.random() < 0.9 else s.lower())
        return out
    s1, s2 = seqs(600), seqs(640)
    write_fastq(str(d / "k_1.fq"), s1, "a")
    write_fastq(str(d / "k_2.fq"), s2, "b")
    plain = build(d, "pipeline_check")
    base = {}
    for paired, mode in ((False, "either"), (True, "either"), (True, "both")):
        o1, o2 = str(d / "p1.fq"), str(d / "p2.fq")
        files = [str(d / "k_1.fq"), str(d / "k_2.fq"), o1, o2] if paired else [str(d / "k_1.fq"), "-", o1, "-"]
        p = subprocess.run([plain, *files, "100", "2", mode], capture_output=True, check=True)
        base[(paired, mode)] = (p.stdout.decode().split(), open(o1, "rb").read(), open(o2, "rb").read() if paired else None)
    return d, s1, s2, base


def keep_bit(s, keep):
    """the amended bit of a read under the stand-in rules, stated without the header's function"""
    if s[:1] not in ("A", "a"):
        return False
    rejected, unplaced = s[1:2] in ("C", "c"), s[1:2] in ("G", "g")
    if keep == 1:
        return not rejected
    if keep == 2:
        return not rejected and not unplaced
    return True


def expected(d, s1, s2, paired, both, keep):
    mates = [(s1, "k_1.fq")] + ([(s2, "k_2.fq")] if paired else [])
    n = min(len(m[0]) for m in mates)
    bits = [[keep_bit(m[0][i], keep) for i in range(n)] for m in mates]
    kept = [(all if both else any)(b[i] for b in bits) for i in range(n)]
    outs = []
    for _, name in mates:
        lines = open(d / name, "rb").read().split(b"\n")
        outs.append(b"".join(lines[4 * i] + b"\n" + lines[4 * i + 1] + b"\n+\n" + lines[4 * i + 3] + b"\n" for i in range(n) if kept[i]))
    return sum(kept), n, outs


@pytest.mark.parametrize("flags", SANITIZERS, ids=["asan_ubsan", "tsan"])
def test_keep_rule_on_the_host_pipeline(data, tmp_path, flags):
    d, s1, s2, base = data
    exe = build(tmp_path, "keep_check", flags)
    counts = {}
    for paired, mode in ((False, "either"), (True, "either"), (True, "both")):
        for batch, workers in ((100, 1), (64, 3)):
            for keep in (0, 1, 2):
                o1, o2 = str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq")
                files = [str(d / "k_1.fq"), str(d / "k_2.fq"), o1, o2] if paired else [str(d / "k_1.fq"), "-", o1, "-"]
                p = subprocess.run([exe, *files, str(batch), "2", mode, str(workers), str(keep)], capture_output=True)
                err, case = p.stderr.decode(), (paired, mode, batch, workers, keep)
                assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (case, err[:2000])
                kept, total, outs = expected(d, s1, s2, paired, mode == "both", keep)
                lines = p.stdout.decode().splitlines()
                assert lines[0].split() == [str(kept), str(total)], (case, lines, err[:500])
                # the hook ran once behind every mate batch's pass
                _, a, _, b = lines[1].split()
                assert a == b and int(a) >= (total + batch - 1) // batch * (2 if paired else 1), (case, lines)
                got = [open(o1, "rb").read()] + ([open(o2, "rb").read()] if paired else [])
                assert got == outs, case
                if keep == 0:          # nothing amended: what the pipeline writes with no report at all
                    assert lines[0].split() == base[(paired, mode)][0] and got[0] == base[(paired, mode)][1], case
                    assert not paired or got[1] == base[(paired, mode)][2], case
                counts[(paired, mode, keep)] = kept
    # the data tell the modes apart under every pair rule, and under `either` some pair is written through one mate alone
    for paired, mode in ((False, "either"), (True, "either"), (True, "both")):
        assert counts[(paired, mode, 0)] > counts[(paired, mode, 1)] > counts[(paired, mode, 2)] > 0
    assert counts[(True, "either", 2)] > counts[(True, "both", 2)]
