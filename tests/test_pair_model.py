"""The rescue of an unplaced mate runs on the CPU: mitoflex_amd/csrc/mf_rescue.h and mf_score.h are plain integer code, and
tests/native/pair_model_check.cpp runs them the way rescue_kernel does -- the staged copy of the read's words, candidates dealt to 64
lanes, the folds combined in the butterfly's order -- on exactly-sized heap arrays under ASan + UBSan, against a per-base loop over
strings: window widths 1, 63, 64, 65, 4096, L = k, 47, 48, 49, 150, 151, every b0 mod 16, both strands, the mate over both ends of the
first and of the last record, a bait N and a read N in the footprint, planted ties.  And the path of a read too long to stage (L = 993,
994, 995, 1200 beside the short ones): the candidates scored from the stream itself with the read's full b0, sixteen bases at a time
without an N and base by base around the Ns, against the staged copy's scores."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rescue_fold_equals_the_per_base_loop(tmp_path):
    exe = str(tmp_path / "pair_model_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "pair_model_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("pair model ok: "), (r.stdout[-1000:], r.stderr[-3000:])
    w = r.stdout.split()
    cases, rescued, ties, short, streamed_n = int(w[3]), int(w[5]), int(w[7]), int(w[9]), int(w[11])
    # lengths x records x bait N x tie x true positions x (widths x wheres, 10 of them with every b0 mod 16) x strands; the four long
    # lengths without ties and with 3 (width, where) each
    assert cases >= 6 * 2 * 2 * 2 * 7 * 10 * 2 * 16 + 4 * 2 * 2 * 7 * 3 * 2 * 16
    assert streamed_n >= 100000          # candidates of reads with an N scored from the stream
    assert rescued >= 1000 and ties >= 1000 and short >= 100
