"""The pile-up's per-position call runs on the CPU: mitoflex_amd/csrc/mf_call.h holds the rule of pileup_call_kernel as plain integer
code (strict_most4, pileup_call_position, clamp_count), and tests/native/pileup_model_check.cpp holds it to cases that the plain-Python
oracle (tests/pileup_oracle.py, PileupOracle.call on a bait of one position) dumps: every count 4-tuple over {0, 1, 2, 3}, each of the
five bait letters (A, C, G, T, invalid), min_depth 1, 2 and 4; then tuples near 2^32, where the call goes by the unclamped counts while
the reported counters saturate at 0xFFFFFFFE.  The program is built and run twice, the second time under ASan + UBSan."""
import itertools
import os
import subprocess
import types

import numpy as np
import pytest

from tests import pileup_oracle as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pileup_model_check.cpp")

BIG = [(1 << 32, (1 << 32) - 1, 0, 0),                      # a strict winner whose clamped counters tie
       ((1 << 32) + 5, (1 << 32) + 5, 0, 0),                # a tie above the clamp
       (0xFFFFFFFE, 0xFFFFFFFF, 0, 0), (0xFFFFFFFD, 0xFFFFFFFE, 0, 0),          # around the clamp itself
       (0, 0, 0xFFFFFFFF, 1 << 32), (3, 2, 1, 1 << 40), ((1 << 33) + 1, 1 << 33, 1 << 33, 1 << 33)]


def case_line(counts, ref, min_depth):
    """one position through the oracle: a bait of one record of one letter"""
    o = pu.PileupOracle(types.SimpleNamespace(recs=[ref], starts=[0, 1], lens=[1]))
    table = np.array([counts], np.int64)
    cons, rec = o.call(table, min_depth)
    bases, matches, mismatches, called, ambiguous, variants = (int(v) for v in rec[0])
    assert bases == sum(counts)
    return " ".join(str(v) for v in [*counts, ref, min_depth, chr(cons[0]), called, ambiguous, variants, matches, mismatches, *pu.clamped(table)[0].tolist()])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lines = [case_line(c, ref, md) for c in [*itertools.product(range(4), repeat=4), *BIG] for ref in "ACGTN" for md in (1, 2, 4)]
    path = str(tmp_path_factory.mktemp("pileup_model") / "cases.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    return path, len(lines)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_model_calls_every_position_as_the_oracle_does(cases, tmp_path, flags):
    path, n = cases
    assert n == (4 ** 4 + len(BIG)) * 5 * 3
    exe = str(tmp_path / "pileup_model_check")
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("pileup model ok: "), (r.stdout[-2000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == n
