"""The keep rule's surface without a GPU: include/mitofilter.h declares the two calls and the three constants, the Python wrapper
exports them and defaults to KEEP_PASSING, and the rule itself (mf_score.h's keep_clears) is the table the header states."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mitofilter.h")).read(), flags=re.S)


def test_header_declares_the_keep_calls_and_constants():
    hdr = header()
    for name, value in (("MF_KEEP_PASSING", 0), ("MF_KEEP_ACCEPTED", 1), ("MF_KEEP_PLACED", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), hdr), name
    v = re.search(r"int\s+mf_verify_keep\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert re.search(r"uint32_t\s+max_permille\s*,\s*int\s+keep\s*,\s*uint32_t\s*\*\s*out_bits\s*,\s*uint32_t\s*\*\s*keep_bits\s*,\s*mf_place_t", v)
    f = re.search(r"int\s+mf_filter_fastq_files_verified_keep\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert re.search(r"uint32_t\s+max_permille\s*,\s*int\s+keep\s*,\s*uint32_t\s*\*\s*base_depth", f)
    # each is its older call with the new arguments and nothing else
    strip = lambda s: re.sub(r"\s+", " ", s).strip()
    old_v = re.search(r"int\s+mf_verify\s*\(([^;]*)\)\s*;", hdr).group(1)
    old_f = re.search(r"int\s+mf_filter_fastq_files_verified\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert strip(v).replace(" int keep,", "").replace(" uint32_t *keep_bits,", "") == strip(old_v)
    assert strip(f).replace(" int keep,", "") == strip(old_f)


def test_wrapper_exports_and_defaults():
    from mitoflex_amd import mitofilter as mf
    assert (mf.KEEP_PASSING, mf.KEEP_ACCEPTED, mf.KEEP_PLACED) == (0, 1, 2)
    assert "mf_verify_keep" in mf.EXPORTS and "mf_filter_fastq_files_verified_keep" in mf.EXPORTS
    for fn in (mf.verify_reads, mf.filter_fastq_files_verified):
        assert inspect.signature(fn).parameters["keep"].default == mf.KEEP_PASSING
    # a call without a keep mode returns the object it always returned, and its keep_bits read as None; with one, the object has the slot
    assert mf.Verified().keep_bits is None and mf.Verified(kept=1).kept == 1
    assert issubclass(mf.VerifiedKeep, mf.Verified) and "keep_bits" in mf.VerifiedKeep.__slots__
    v = mf.VerifiedKeep(keep_bits=5, total=2)
    assert (v.keep_bits, v.total, v.bits) == (5, 2, None) and repr(v) == "VerifiedKeep(total, keep_bits)"
    from mitoflex_amd.bim import bim
    p = inspect.signature(bim.kmer_bait_map).parameters
    assert p["keep"].default is None and p["max_permille"].default is None


def test_library_exports_the_keep_calls(built_lib):
    assert hasattr(built_lib, "mf_verify_keep") and hasattr(built_lib, "mf_filter_fastq_files_verified_keep")


def test_keep_clears_is_the_stated_table(tmp_path):
    """mf_score.h compiles on the host alone; placed x accepted x keep against the header's three sentences (and an unknown mode
    clears nothing)."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "mf_score.h"\n#include <stdio.h>\nint main() { for (int k = -1; k <= 3; k++) for (int p = 0; p < 2; p++) '
                   'for (int a = 0; a < 2; a++) printf("%d %d %d %d\\n", k, p, a, (int)mf::keep_clears(p, a, k)); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "mitoflex_amd", "csrc"), str(src), "-o", exe])
    got = {tuple(map(int, l.split()[:3])): int(l.split()[3]) for l in subprocess.check_output([exe]).decode().splitlines()}
    for k in (-1, 0, 1, 2, 3):
        for p in (0, 1):
            for a in (0, 1):
                want = (p and not a) if k == 1 else (not (p and a)) if k == 2 else False
                assert got[(k, p, a)] == int(bool(want)), (k, p, a)
