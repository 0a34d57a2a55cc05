"""The 16-base compare of the verifying placement kernel runs on the CPU: mitoflex_amd/csrc/mf_score.h is plain integer code, and
tests/native/score_model_check.cpp calls it on exactly-sized heap arrays under ASan + UBSan against a per-base loop over strings --
every (b0 mod 16) x (start mod 16) x strand, lengths 21 .. 1500, starts around both ends of the LAST record, a bait N in the footprint,
mismatches planted at read offsets 0, L - 1, 15, 16, 17.  A wrong shift or an index one word too far shows here, not on a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_chunks_equal_the_per_base_loop(tmp_path):
    exe = str(tmp_path / "score_model_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "score_model_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("score model ok: "), (r.stdout[-1000:], r.stderr[-3000:])
    assert int(r.stdout.split()[3]) >= 8 * 2 * 2 * 66 * 2 * 16          # lengths x record lengths x bait N x starts x strands x b0 mod 16
