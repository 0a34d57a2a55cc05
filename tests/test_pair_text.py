"""The pair report of `fastfilter pairs` is written by a pure function (mitoflex_amd/csrc/mf_report_text.h: write_pair_report), so its
format is held to its bytes without a device: tests/native/pair_text_check.cpp reads one case that this test writes as plain names and
numbers, writes the report under ASan + UBSan, and the file is compared with text formatted here from the same numbers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# three records of 900, 0 and 5 positions: one with every kind, an empty one (mean insert 0.000), one whose sums need 64 bits
NAMES = ["r0", "empty", "big"]
STARTS = [0, 900, 900, 905]
# proper, discordant, cross, rescued, single, insert_sum
RECS = [(7, 2, 1, 3, 4, 3001), (0, 0, 0, 0, 0, 0), (5000000000, 0, 0, 5000000000, 1, 3000000000000)]
NONE = 6


def expected():
    head = "record\tname\tlength\tproper\tdiscordant\tcross\trescued\tsingle\tmean_insert\n"
    rows = ["%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\n" % (j, NAMES[j], STARTS[j + 1] - STARTS[j], p, d, c, r, s, ins / (p + r) if p + r else 0.0)
            for j, (p, d, c, r, s, ins) in enumerate(RECS)]
    return head + "".join(rows) + "-\t*none*\t%d\n" % NONE


def test_the_pair_report_is_what_its_numbers_say(tmp_path):
    exe, out = str(tmp_path / "pair_text_check"), str(tmp_path / "pairs.tsv")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "pair_text_check.cpp"), "-o", exe])
    case = "\n".join([str(len(NAMES)), " ".join(NAMES), " ".join(map(str, STARTS))] + [" ".join(map(str, r)) for r in RECS] + [str(NONE)]) + "\n"
    r = subprocess.run([exe, out], input=case, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert open(out).read() == expected()
    assert expected().splitlines()[1] == "0\tr0\t900\t7\t2\t1\t3\t4\t300.100"          # the restatement itself, once by hand
