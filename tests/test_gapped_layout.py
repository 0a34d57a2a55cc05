"""The insertion pile is a sixth section of the placement counters and the gapped call three sections more of the report scratch, all
plain arithmetic in mitoflex_amd/csrc/mf_placelayout.h: tests/native/gapped_layout_check.cpp holds their offsets to a restatement of its
own under ASan + UBSan, and the layouts that are not gapped to what they were."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gapped_sections_equal_their_restatement(tmp_path):
    exe = str(tmp_path / "gapped_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "gapped_layout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("gapped layout ok: "), (r.stdout[-1000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == 8 * 4 * 4 * 2 * 2 * 2          # positions x records x bands x pileup x gapped x place
