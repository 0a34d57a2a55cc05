"""`fastfilter bait --score-report` writes its file with the pure function write_score_report (mitoflex_amd/csrc/mf_report_text.h:
arrays of the file-level call in, text out), so the format is held to its bytes without a device, as tests/test_report_text.py does for
the other eight: tests/native/score_text_check.cpp reads one case that this test writes as plain names and numbers and writes score.tsv
under ASan + UBSan, and the file is compared with text formatted here from the same numbers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 32
U64 = 2 ** 64 - 1

# an ordinary record; an empty record (length 0, nothing placed); a record whose accepted reads compared nothing (permille 0.000, not a
# division by zero); a record with counts that need 64 bits and a full last bin
NAMES = ["mito", "empty", "nothing_compared", "wide"]
STARTS = [0, 3000, 3000, 3040, 3040 + 16569]
RECS = [
    (400, 300, 50000, 37, [380, 15, 5] + [0] * 26 + [0, 0, 300]),
    (0, 0, 0, 0, [0] * BINS),
    (2, 1, 0, 0, [3] + [0] * (BINS - 1)),
    (2 ** 40, 2 ** 33, U64, 2 ** 63 + 5, [2 ** 40] + [7] * (BINS - 2) + [U64]),
]


def _case_text():
    rows = [[len(NAMES)], NAMES, STARTS] + [[a, r, c, m] + h for a, r, c, m, h in RECS]
    return "".join(" ".join(str(x) for x in row) + "\n" for row in rows)


def _expected():
    head = "record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tpermille" + "".join("\tmm%d" % b for b in range(BINS - 1)) + "\tmm31+\n"
    rows = []
    for j, (a, r, c, m, h) in enumerate(RECS):
        permille = "%.3f" % (1000.0 * float(m) / float(c) if c else 0.0)
        rows.append("%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s" % (j, NAMES[j], STARTS[j + 1] - STARTS[j], a, r, c, m, permille) + "".join("\t%d" % x for x in h) + "\n")
    return head + "".join(rows)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_text")
    exe, case = str(d / "score_text_check"), str(d / "case.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "score_text_check.cpp"), "-o", exe])
    with open(case, "w") as f:
        f.write(_case_text())
    return exe, case


def test_the_case_holds_what_it_is_for():
    text = _expected()
    assert STARTS[2] - STARTS[1] == 0 and RECS[1] == (0, 0, 0, 0, [0] * BINS)
    assert RECS[2][0] > 0 and RECS[2][2] == 0
    assert RECS[3][2] > 2 ** 63 and RECS[3][4][-1] == U64 and all(len(r[4]) == BINS for r in RECS)
    lines = text.split("\n")
    assert len(lines) == 6 and all(len(l.split("\t")) == 8 + BINS for l in lines[:5])
    assert lines[1].split("\t")[7] == "0.740" and lines[2].split("\t")[7] == "0.000" and lines[3].split("\t")[7] == "0.000"
    assert lines[4].split("\t")[7] == "500.000" and lines[4].endswith("\t%d" % U64)


def test_score_report_byte_for_byte(driver, tmp_path):
    exe, case = driver
    r = subprocess.run([exe, case, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("returned true") == 1, (r.stdout[-1000:], r.stderr[-2000:])
    assert os.listdir(tmp_path) == ["score.tsv"]
    with open(tmp_path / "score.tsv", "rb") as f:
        assert f.read() == _expected().encode()


UNWRITABLE = ["missing_directory/file"] + (["/dev/full"] if os.path.exists("/dev/full") else [])


@pytest.mark.parametrize("path", UNWRITABLE)
def test_an_unwritable_path_makes_the_writer_return_false(driver, tmp_path, path):
    exe, case = driver
    r = subprocess.run([exe, case, "--unwritable", os.path.join(str(tmp_path), path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("returned false") == 1 and "returned true" not in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
