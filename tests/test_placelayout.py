"""The counter layout and the report scratch of the placement family (mf_place, mf_pileup, mf_verify) are plain arithmetic in
mitoflex_amd/csrc/mf_placelayout.h, which includes nothing of the device: tests/native/placelayout_check.cpp holds every offset to a
restatement of its own under ASan + UBSan -- positions 0 .. 2^31 - 2, records 0 .. 1000, every (pileup, verify) and every (placement
sections, pile-up sections) -- and the sizes to what mf_place, mf_pileup and mf_verify reserved when each laid its scratch out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_and_scratch_equal_their_restatement(tmp_path):
    exe = str(tmp_path / "placelayout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "placelayout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("place layout ok: "), (r.stdout[-1000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) == 7 * 4 * 2 * 2 * 2 * 2 * 2          # positions x records x pileup x verify x sections x tile counts
