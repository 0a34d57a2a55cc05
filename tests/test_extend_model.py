"""The extended records' scalar pieces run on the CPU: mitoflex_amd/csrc/mf_call.h holds the (record, side, offset) indexing that
align_adds stores an overhanging base by and the column rule of extend_call_kernel as plain integer code, and
tests/native/extend_model_check.cpp holds both to cases that the plain-Python oracle dumps: the overhanging diagonal steps of the `ends`
set's accepted reads, hand-written coordinates around both ends of the first and the last record, and tables around the call's two
conditions.  The program is built through tests/native_host.build_check, plain and under ASan + UBSan."""
import random
import subprocess

import numpy as np
import pytest

from tests import align_oracle as ao
from tests import extend_data as xd
from tests import extend_oracle as xo
from tests import native_host as nh
from tests import place_oracle as po

_IDX = {c: i for i, c in enumerate("ACGTN")}


def pile_line(R, E, j, ln, x, steps):
    ext = np.zeros((R, 2, E, 4), np.int64)
    xo.pile_steps(ext, x, steps, j, ln, E)
    outside = [(c, _IDX[x[i]]) for mv, i, c in steps if mv == ao.DIAG and not 0 <= c < ln]
    flat = ext.reshape(-1)
    at = np.nonzero(flat)[0]
    return " ".join(str(v) for v in ["P", R, E, j, ln, len(outside), *[v for p in outside for v in p], len(at), *[v for a in at for v in (a, flat[a])]])


def call_line(table, min_depth):
    got = xo.call_end(np.array(table, np.int64).reshape(-1, 4), min_depth)
    return " ".join(str(v) for v in ["C", len(table) // 4, min_depth, *table, len(got), got or "-"])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lines = []
    # hand-written: a read of 12 bases on a record of 6 positions, from coordinate -4: four bases before it, two behind it
    steps = [(ao.DIAG, i, i - 4) for i in range(12)]
    for R, j in ((1, 0), (3, 0), (3, 2), (3, 1)):
        for E in (1, 2, 3, 4, 64):
            lines.append(pile_line(R, E, j, 6, "ACGTACGTACGT", steps))
            lines.append(pile_line(R, E, j, 6, "NCGNACGTACNT", steps))
    # the `ends` set through the alignment oracle
    text, _, _ = xd.ends_bait()
    seqs, _ = xd.ends_reads()
    o = po.PlaceOracle(text, 31)
    A = ao.AlignOracle(o)
    rows = o.place(o.tally(seqs), 1)[1]
    n_over = 0
    for i, (seq, row) in enumerate(zip(seqs, rows)):
        if row[0] < po.AMBIGUOUS:
            a = A.align_row(seq, row, (0, 4, 8)[i % 3])
            j = int(row[0])
            n_over += a["ref_begin"] < 0 or a["ref_end"] > o.lens[j]
            lines.append(pile_line(3, (1, 16, 64, 4096)[i % 4], j, o.lens[j], A.oriented(seq, int(row[1])), a["steps"]))
    assert n_over > 100
    # the call: hand-worked, then random tables around min_depth and around a tie
    lines += [call_line([3, 0, 0, 0, 0, 2, 1, 0, 0, 0, 0, 3], 3), call_line([3, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 3], 3), call_line([2, 2, 0, 0, 0, 5, 0, 0], 1),
              call_line([0, 0, 0, 0, 0, 5, 0, 0], 1), call_line([0, 0, 0, 1], 1), call_line([0, 0, 0, 1], 2), call_line([1 << 40, 1 << 40, 0, 0], 1),
              call_line([(1 << 40) + 1, 1 << 40, 0, 0, 0, 0, 1 << 33, 5], 1 << 20), call_line([1, 1, 1, 1], 1), call_line([0, 3, 3, 2], 3)]
    rng = random.Random(31)
    for _ in range(300):
        E = rng.choice((1, 2, 5, 64, 70))
        lines.append(call_line([rng.randint(0, 3) if q < 4 * 6 else 0 for q in range(4 * E)], rng.randint(1, 4)))
    path = str(tmp_path_factory.mktemp("extend_model") / "cases.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    return path, len(lines)


@pytest.mark.parametrize("flags", nh.FLAG_SETS[:2], ids=nh.FLAG_IDS[:2])
def test_the_model_gives_the_oracle_s_pile_and_calls(cases, flags):
    path, n = cases
    assert n > 400
    exe = nh.build_check(("extend_model_check.cpp",), flags)
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    nh.clean(r.stderr)
    assert r.returncode == 0 and r.stdout.decode().startswith("extend model ok: "), (r.stdout[-2000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == n
