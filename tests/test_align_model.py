"""The banded alignment's rule runs on the CPU: mitoflex_amd/csrc/mf_align.h is plain integer code, and
tests/native/align_model_check.cpp holds two models over it -- the full table cell by cell, and the kernel's formulation lane by lane
(prefix minimum over the diagonals, packed direction bits, the traceback's word per read base) -- to cases that the plain-Python oracle
dumps: the hand-worked ones, random reads with indels, Ns and overhangs at every band the kernel instantiates a lane count for, and reads
of the GPU tests' inputs.  The program is built and run twice, the second time under ASan + UBSan."""
import os
import random
import subprocess

import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import place_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "align_model_check.cpp")


def case_line(x, rec, start, W, a):
    deleted = [c for mv, _, c in a["steps"] if mv == ao.DEL and 0 <= c < len(rec)]
    runs = [(c, n) for c, n in ao.insertion_runs(a["steps"]) if 0 <= c - 1 < len(rec)]
    fields = [W, start, x, rec, a["compared"], a["mismatches"], a["insertions"], a["deletions"], a["ref_begin"], a["ref_end"], len(deleted), *deleted,
              len(runs), *[v for run in runs for v in run]]
    return " ".join(str(f) for f in fields)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lines = []
    rec = "GCTAGGATCCATGCAAGTCTAGACCGTTAGACGTTCAGGA"
    hand = [("CGTC" + "A" * 7 + "GCTG", "CGTC" + "A" * 8 + "GCTG", 0, 2), ("GATC" + "TA" * 5 + "CGGA", "GATC" + "TA" * 4 + "CGGA", 0, 2),
            (rec[0:30] + rec[32:34], rec, 0, 4), (rec[8:10] + rec[12:40], rec, 10, 4), (rec[0:30] + rec[32:35], rec, 0, 4),
            ("TTGCA" + "ACGGTCATTGCAAGCTTAGC" + "GGACT", "ACGGTCATTGCAAGCTTAGC", -5, 3)]
    for x, r, start, W in hand:
        lines.append(case_line(x, r, start, W, ao.align(x, r, start, W)))
    rng = random.Random(17)
    for i in range(260):
        r = "".join(rng.choices("ACGTN" if rng.random() < 0.2 else "ACGT", k=rng.randint(40, 400)))
        L = rng.choice((21, 31, 32, 33, 63, 64, 65, 96, 97, 150)) if i % 2 else rng.randint(12, 200)
        a = rng.randrange(-12, max(len(r) - L // 2, 1))
        x = "".join(r[c] if 0 <= c < len(r) and rng.random() < 0.95 else rng.choice("ACGTN") for c in range(a, a + L))
        if rng.random() < 0.7:
            x = ad.with_indel(rng, x, rng.randrange(L), rng.randint(1, 9), rng.random() < 0.5)
        W = rng.choice((0, 1, 2, 4, 8, 16, 20, 30, 31))
        lines.append(case_line(x, r, a, W, (ao.align if len(x) * W < 2000 else ao.align_fast)(x, r, a, W)))
    text, parts = ad.align_bait()
    seqs, groups = ad.ragged_reads(parts)
    o = po.PlaceOracle(text, 31)
    A = ao.AlignOracle(o)
    picked = [i for g in ("indel", "over", "ns", "repeat", "ends") for i in range(*groups[g])][::7] + [groups["long"][0]]
    rows = o.place(o.tally([seqs[i] for i in picked]), 1)[1]
    for i, row in zip(picked, rows):
        if row[0] < po.AMBIGUOUS:
            W = (1, 4, 8, 30)[i % 4]
            lines.append(case_line(A.oriented(seqs[i], int(row[1])), o.recs[int(row[0])], int(row[2]), W, A.align_row(seqs[i], row, W)))
    path = str(tmp_path_factory.mktemp("align_model") / "cases.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    return path, len(lines)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_both_models_give_the_oracle_s_alignments(cases, tmp_path, flags):
    path, n = cases
    assert n > 350
    exe = str(tmp_path / "align_model_check")
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("align model ok: "), (r.stdout[-2000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == n
