"""The report files of `fastfilter bait` are written by pure functions (mitoflex_amd/csrc/mf_report_text.h: arrays of the file-level
calls in, text out), so their formats are held to their bytes without a device: tests/native/report_text_check.cpp reads one case that
this test writes as plain names and numbers, writes all eight formats under ASan + UBSan, and every file is compared with text formatted
here from the same numbers -- the consensus with mitofilter.consensus_fasta, the variants with the rows of mitofilter.pileup_variants.
The GPU suite's CLI tests compare the same files with what the library computes."""
import os
import subprocess

import numpy as np
import pytest

from mitoflex_amd import mitofilter as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 0xFFFFFFFF

# three records of 61, 0 and 5 positions: the 60-column wrap, an empty record in every format, a record shorter than a line
NAMES = ["rec61", "empty", "rec5"]
STARTS = [0, 61, 61, 66]
P = STARTS[-1]
RECORD_READS = [7, 0, 3, 2, 11]                       # records, ambiguous, unassigned
GROUPS, GROUP_READS = ["geneA", "geneB"], [10, 0, 2, 11]
# windows, covered, depth_sum, depth_max: the empty record has no window (mean 0.000)
DEPTH_RECS = [(31, 20, 12345, 999), (0, 0, 0, 0), (3, 3, 10, 5)]
PROFILE = [(7 * p) % 50 if p < 31 or 61 <= p < 64 else mf.DEPTH_NONE for p in range(P)]       # no valid window at a record's end
# forward, reverse, over_begin, over_end, covered, base_sum: the empty record has length 0 (mean 0.000)
PLACE_RECS = [(5, 4, 1, 2, 60, 1234), (0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 5, 13)]
BASE_DEPTH = [p % 17 for p in range(P)]
BASE_DEPTH[60], BASE_DEPTH[65] = 4000000000, 99       # the maximum on each record's last position
NOT_PLACED = 6
LETTERS = "ACGT" * 15 + "N" + "ACGTA"
PILE = [((3 * p) % 11, (5 * p) % 7, p % 5, (p * p) % 13) for p in range(P)]
PILE[0] = (U32, U32, U32, U32)                        # a depth that needs 64 bits
PILE[1] = (U32, 1, U32, 2)                            # ... in a variant row too
# position 0: the call is the bait letter; 1 .. 4: one variant for each alt letter; then the bait's letter in lower case, N where the
# most is tied; 60: a call over a bait N; the last record: a variant behind the empty record
CONSENSUS = "A" + "ACGT" + "cN" + LETTERS[7:60].lower() + "A" + "ACgNT"
assert len(LETTERS) == len(CONSENSUS) == len(PILE) == len(PROFILE) == P


def _case_text():
    rows = [[len(NAMES)], NAMES, STARTS, RECORD_READS, [len(GROUPS)], GROUPS, GROUP_READS]
    rows += [list(r) for r in DEPTH_RECS] + [PROFILE] + [list(r) for r in PLACE_RECS] + [BASE_DEPTH, [NOT_PLACED], [LETTERS]]
    rows += [list(c) for c in PILE] + [[CONSENSUS]]
    return "".join(" ".join(str(x) for x in row) + "\n" for row in rows)


def _positions():
    for j, name in enumerate(NAMES):
        for p in range(STARTS[j], STARTS[j + 1]):
            yield name, p - STARTS[j] + 1, p


def _reads_text(head, names, counts):
    rows = ["%s\tname\treads\n" % head] + ["%d\t%s\t%d\n" % (i, nm, counts[i]) for i, nm in enumerate(names)]
    return "".join(rows) + "-\t*ambiguous*\t%d\n-\t*unassigned*\t%d\n" % (counts[-2], counts[-1])


def _expected():
    length = [STARTS[j + 1] - STARTS[j] for j in range(len(NAMES))]
    depth_report = "record\tname\tlength\twindows\tcovered\tmean\tmax\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\t%.3f\t%d\n" % (j, NAMES[j], length[j], w, c, s / w if w else 0.0, m) for j, (w, c, s, m) in enumerate(DEPTH_RECS))
    place_report = "record\tname\tlength\tforward\treverse\tover_begin\tover_end\tcovered\tmean\tmax\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\t%d\n" % (j, NAMES[j], length[j], f, r, b, e, c, s / length[j] if length[j] else 0.0,
                                                      max(BASE_DEPTH[STARTS[j]:STARTS[j + 1]], default=0))
        for j, (f, r, b, e, c, s) in enumerate(PLACE_RECS)) + "-\t*unplaced*\t%d\n" % NOT_PLACED
    pile = np.array(PILE, dtype=np.uint32).view(mf.PILEUP).reshape(-1)
    variants = mf.pileup_variants(STARTS, LETTERS.encode(), pile, CONSENSUS.encode())
    return {
        "reads.tsv": _reads_text("record", NAMES, RECORD_READS),
        "groups.tsv": _reads_text("group", GROUPS, GROUP_READS),
        "depth_report.tsv": depth_report,
        "depth_profile.tsv": "".join("%s\t%d\t%d\n" % (nm, at, PROFILE[p]) for nm, at, p in _positions() if PROFILE[p] != mf.DEPTH_NONE),
        "place_report.tsv": place_report,
        "base_depth.tsv": "".join("%s\t%d\t%d\n" % (nm, at, BASE_DEPTH[p]) for nm, at, p in _positions()),
        "pileup.tsv": "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((nm, at, LETTERS[p], sum(PILE[p])) + PILE[p]) for nm, at, p in _positions()),
        "consensus.fa": mf.consensus_fasta(NAMES, STARTS, CONSENSUS.encode()),
        "variants.tsv": "".join("%s\t%d\t%s\t%s\t%d\t%d\n" % (NAMES[v["record"]], v["pos"] + 1, v["ref"].decode(), v["alt"].decode(), v["depth"], v["alt_count"])
                                for v in variants),
    }, variants


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("report_text")
    exe, case = str(d / "report_text_check"), str(d / "case.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "report_text_check.cpp"), "-o", exe])
    with open(case, "w") as f:
        f.write(_case_text())
    return exe, case


def test_the_case_holds_what_it_is_for():
    expected, variants = _expected()
    assert [STARTS[j + 1] - STARTS[j] for j in range(3)] == [61, 0, 5]
    assert mf.DEPTH_NONE in PROFILE and DEPTH_RECS[1][0] == 0
    assert BASE_DEPTH[60] == max(BASE_DEPTH[:61]) and BASE_DEPTH[65] == max(BASE_DEPTH[61:])
    assert sum(PILE[0]) == 4 * U32 > 2 ** 32
    assert any(c.isupper() and c != "N" for c in CONSENSUS) and any(c.islower() for c in CONSENSUS) and "N" in CONSENSUS
    assert LETTERS[60] == "N" and CONSENSUS[60] == "A" and CONSENSUS[0] == LETTERS[0]          # neither is a variant
    assert sorted(v["alt"].decode() for v in variants) == ["A", "C", "G", "T", "T"]
    assert [(int(v["record"]), int(v["pos"])) for v in variants] == [(0, 1), (0, 2), (0, 3), (0, 4), (2, 4)]
    assert "\t0.000\t" in expected["depth_report.tsv"] and "\t0.000\t0\n" in expected["place_report.tsv"]
    assert expected["consensus.fa"].split("\n")[:5] == [">rec61", CONSENSUS[:60], CONSENSUS[60], ">empty", ">rec5"]


def test_every_format_byte_for_byte(driver, tmp_path):
    exe, case = driver
    r = subprocess.run([exe, case, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("returned true") == 9, (r.stdout[-1000:], r.stderr[-2000:])
    expected, _ = _expected()
    assert sorted(os.listdir(tmp_path)) == sorted(expected)
    for name, text in expected.items():
        with open(tmp_path / name, "rb") as f:
            assert f.read() == text.encode(), name


# a file that cannot be opened, and (where the system has it) one that opens and takes no byte
UNWRITABLE = ["missing_directory/file"] + (["/dev/full"] if os.path.exists("/dev/full") else [])


@pytest.mark.parametrize("path", UNWRITABLE)
def test_an_unwritable_path_makes_the_writers_return_false(driver, tmp_path, path):
    exe, case = driver
    r = subprocess.run([exe, case, "--unwritable", os.path.join(str(tmp_path), path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("returned false") == 9 and "returned true" not in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
