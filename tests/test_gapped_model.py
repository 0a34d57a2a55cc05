"""The gapped consensus' scalar pieces run on the CPU: mitoflex_amd/csrc/mf_align.h holds the run-offset walk that align_adds stores
the inserted letters by and the per-position call of gapped_call_kernel as plain integer code, and tests/native/gapped_model_check.cpp
holds both to cases that the plain-Python oracle dumps -- the words the traceback leaves per read base are packed here from the oracle's
steps.  Among them a run of exactly span bases, and a corrupted word sequence whose walk would pass span at the last position of the
bait and must store nothing.  The program is built and run twice, the second time under ASan + UBSan."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import gapped_oracle as go
from tests import place_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gapped_model_check.cpp")


def pack(steps, L):
    """one word a read base, as the traceback leaves them: the column the path enters row b + 1 at, inserted (bit 32), the positions that
    row deletes behind it (from bit 33)"""
    ent = [0] * L
    for mv, i, c in steps:
        if mv == ao.DIAG:
            ent[i] = (c + 1) & 0xFFFFFFFF
        elif mv == ao.INS:
            ent[i] = (c & 0xFFFFFFFF) | (1 << 32)
        else:
            assert i >= 1
            ent[i - 1] += 1 << 33
    return ent


def walk_line(x, steps, s0, ln, total, span):
    pile = np.zeros((total, span, 4), np.int64)
    go.pile_steps(pile, x, steps, s0, ln, span)
    at = np.argwhere(pile)
    return " ".join(str(v) for v in ["R", span, s0, ln, total, len(x), x, *pack(steps, len(x)), len(at), *[v for p, t, l in at for v in (p, t, l, pile[p, t, l])]])


def call_line(span, min_depth, D, dels, cons, counts):
    pile = np.array(counts, np.int64).reshape(1, span, 4)
    g, _, recs = go.call([0, 1], [D], [dels], cons.encode(), pile, min_depth)
    return " ".join(str(v) for v in ["C", span, min_depth, D, dels, cons, *pile.reshape(-1).tolist(), recs[0][1], g.decode() or "-"])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lines = []
    rng = random.Random(29)
    # a run of exactly span bases: the part before it on diagonal +W, the part behind it on -W
    rec = "".join(rng.choices("ACGT", k=60))
    for W in (1, 2, 4):
        x = rec[10:25] + "".join(rng.choice([b for b in "ACGT" if b != rec[25]]) for _ in range(2 * W)) + rec[25:45]
        a = ao.align(x, rec, 10 - W, W)
        runs = ao.insertion_runs(a["steps"])
        assert a["insertions"] == 2 * W and max(n for _, n in runs) >= W          # (where the rule's order of moves leaves them whole)
        lines.append(walk_line(x, a["steps"], 5, len(rec), 5 + len(rec), 2 * W))
    rec2 = "ACGGTCATTGCAAGCTTAGCCATGACCTAG"
    x = rec2[:12] + "TTTT" + rec2[12:]
    a = ao.align(x, rec2, -2, 2)
    assert ao.insertion_runs(a["steps"]) == [(12, 4)]                              # exactly span = 4 bases, offsets 0 .. 3
    lines.append(walk_line(x, a["steps"], 0, len(rec2), len(rec2), 4))
    # an inserted N keeps its offset; a run before the first position counts nowhere, one behind the last position counts
    steps = [(ao.INS, 0, 0), (ao.DIAG, 1, 0), (ao.DIAG, 2, 1), (ao.INS, 3, 2), (ao.INS, 4, 2), (ao.INS, 5, 2), (ao.DIAG, 6, 2), (ao.INS, 7, 3), (ao.INS, 8, 3)]
    lines.append(walk_line("TACGNTAGC", steps, 4, 3, 7, 4))
    # a deletion between two insertions: two runs
    lines.append(walk_line("ACGT", [(ao.INS, 0, 3), (ao.DEL, 1, 3), (ao.INS, 1, 4), (ao.DIAG, 2, 4), (ao.DIAG, 3, 5)], 0, 10, 10, 2))
    # corrupted words: span + 3 inserted bases in a row at the LAST position of the bait; only offsets below span are stored
    for span in (2, 4, 62):
        ln, L = 9, span + 3
        ent = [(ln & 0xFFFFFFFF) | (1 << 32)] * L
        stored = [v for t in range(span) for v in (ln - 1, t, 1, 1)]
        lines.append(" ".join(str(v) for v in ["R", span, 0, ln, ln, L, "C" * L, *ent, span, *stored]))
    # ... and with no span at all nothing is stored
    lines.append(" ".join(str(v) for v in ["R", 0, 0, 9, 9, 3, "CCC", *[(9 | (1 << 32))] * 3, 0]))
    # reads of the GPU tests' inputs, through the alignment oracle
    text, parts = ad.align_bait()
    seqs, groups = ad.ragged_reads(parts)
    o = po.PlaceOracle(text, 31)
    A = ao.AlignOracle(o)
    picked = [i for g in ("indel", "over", "ns", "repeat", "ends") for i in range(*groups[g])][::5]
    rows = o.place(o.tally([seqs[i] for i in picked]), 1)[1]
    n_ins = 0
    for i, row in zip(picked, rows):
        if row[0] < po.AMBIGUOUS:
            W = (1, 4, 8, 30)[i % 4]
            a = A.align_row(seqs[i], row, W)
            j = int(row[0])
            n_ins += a["insertions"] > 0
            lines.append(walk_line(A.oriented(seqs[i], int(row[1])), a["steps"], int(o.starts[j]), o.lens[j], int(o.starts[-1]), 2 * W))
    assert n_ins > 30
    # the call: hand-worked, then random counters around the two thresholds
    lines += [call_line(4, 1, 4, 0, "G", [0, 0, 4, 0, 0, 0, 0, 4] + [0] * 8), call_line(4, 1, 4, 0, "G", [0, 0, 2, 0] + [0] * 12),
              call_line(4, 1, 4, 0, "G", [0, 0, 3, 0] + [0] * 12), call_line(4, 1, 4, 0, "G", [2, 2, 0, 0, 1, 0, 0, 3] + [0] * 8),
              call_line(4, 1, 4, 2, "T", [0] * 16), call_line(4, 1, 4, 3, "T", [0] * 16), call_line(4, 1, 4, 4, "G", [0, 0, 0, 4] + [0] * 12),
              call_line(4, 3, 2, 2, "t", [2, 0, 0, 0] + [0] * 12), call_line(0, 1, 4, 4, "A", []), call_line(2, 1, 0, 0, "a", [0] * 8),
              call_line(2, 1, 5, 0, "C", [3, 0, 0, 0, 0, 3, 0, 0]), call_line(2, 1, 1 << 40, 1 << 39, "C", [1 << 39, 1, 0, 0, 0, 0, 0, 0])]
    for _ in range(300):
        span = rng.choice((2, 4, 8, 62))
        D = rng.randint(0, 12)
        counts = [rng.randint(0, max(D // 2 + 1, 1)) if q < 3 * 4 else 0 for q in range(4 * span)]
        lines.append(call_line(span, rng.randint(1, 4), D, rng.randint(0, D), rng.choice("ACGTNacgtn"), counts))
    path = str(tmp_path_factory.mktemp("gapped_model") / "cases.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    return path, len(lines)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_model_gives_the_oracle_s_pile_and_calls(cases, tmp_path, flags):
    path, n = cases
    assert n > 400
    exe = str(tmp_path / "gapped_model_check")
    subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", exe])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("gapped model ok: "), (r.stdout[-2000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == n
