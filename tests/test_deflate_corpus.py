"""The DEFLATE corpus of tests/deflate_writer.py without a GPU: every stream the writer makes is valid for zlib, and its block boundaries
are the ones zlib's Z_BLOCK mode finds; the host decoders -- the streaming inflater and the parallel reader (tests/native/inflate_check.cpp),
the gap fill mf::inflate_gap (tests/native/gap_check.cpp) -- and the lane-walk model of the device decoder (tools/gzlane_model.cpp) give
zlib's text on all of it: full-window distances, overlapping copies, 15-bit codes, small alphabets, empty and stored blocks, fixed blocks'
top codes, extreme headers, and zlib's own strategies, memLevels and window sizes.  The device kernels get the same corpus in
tests/test_gpu_gzdev_kernels.py."""
import os
import subprocess

import pytest

from tests import deflate_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitoflex_amd", "csrc")
NAMES = sorted(W.WRITER_ITEMS) + sorted(W.ZLIB_VARIANTS)


@pytest.fixture(scope="module")
def exes(built_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("corpus")
    out = {}
    for name in ("inflate_check", "gap_check"):
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "native", name + ".cpp"),
                               os.path.join(CSRC, "build", "mf_inflate.o"), os.path.join(CSRC, "build", "mf_pinflate.o"), "-lz", "-lpthread", "-o", out[name]])
    out["model"] = str(d / "gzlane_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "gzlane_model.cpp"), "-lz", "-o", out["model"]])
    return out


def test_writer_codes():
    """the writer's own parts: length and distance codes at their edges, length-limited code lengths, the runs of code lengths"""
    assert W.len_code(258) == (285, 0, 0) and W.len_code(257) == (284, 30, 5) and W.len_code(3) == (257, 0, 0) and W.len_code(227) == (284, 0, 5)
    assert W.dist_code(32768) == (29, 8191, 13) and W.dist_code(24577) == (29, 0, 13) and W.dist_code(1) == (0, 0, 0)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    lens = W.limited_lengths(fib, 15)
    assert max(lens) == 15 and W.kraft(lens) == 32768
    assert W.limited_lengths([0, 5, 0], 15) == [0, 1, 0]
    runs = W.rle_code_lengths([0] * 140 + [4] * 7 + [0] * 10 + [5] * 3)
    assert [s for s, _, _ in runs] == [18, 0, 0, 4, 16, 17, 5, 5, 5] and runs[0][1] == 138 - 11 and runs[4][1] == 6 - 3 and runs[5][1] == 10 - 3
    assert all(s < 16 for s, _, _ in W.rle_code_lengths([0] * 140 + [4] * 7, rle=False))


@pytest.mark.parametrize("name", sorted(W.WRITER_ITEMS))
def test_writer_boundaries_are_zlibs(name):
    gz, text, bounds, _ = W.corpus()[name]
    zb, end, ztext = W.zlib_boundaries(gz[10:-8])
    assert ztext == text
    assert [(b - 80, off) for b, off, _ in bounds] == zb
    assert [f for _, _, f in bounds] == [False] * (len(bounds) - 1) + [True]
    assert end <= (len(gz) - 18) * 8 < end + 8


def test_corpus_reaches_its_edges():
    """what the items are there for is in their text: the full-window items repeat with their period (markers of index < 262 can only
    come from distances above 32 506), the stored item holds both 65 535-byte blocks, the tiny-block item has hundreds of blocks"""
    c = W.corpus()
    for p in (32768, 32767, 32600, 32507):
        text = c["full_window_%d" % p][1]
        same = sum(text[i] == text[i - p] for i in range(p, len(text), 97))
        assert same > 0.9 * len(range(p, len(text), 97)), p
    assert len(c["empty_and_stored"][1]) > 2 * 65535
    assert len(c["tiny_blocks"][2]) > 700 and len(c["small_alphabets"][2]) == 30


@pytest.mark.parametrize("name", NAMES)
def test_host_decoders_and_lane_model(exes, tmp_path, name):
    gz, text, _, _ = W.corpus()[name]
    f, w = tmp_path / "c.gz", tmp_path / "c.raw"
    f.write_bytes(gz)
    w.write_bytes(text)
    for chunk in ("1048576", "4099"):
        out = subprocess.run([exes["inflate_check"], str(f), str(w), chunk], capture_output=True, text=True, timeout=300).stdout.strip()
        assert out == "ok", (name, chunk, out)
    for threads, cchunk in (("4", "1024"), ("3", "4096"), ("8", "65536")):
        out = subprocess.run([exes["inflate_check"], str(f), str(w), "1048576", "--parallel", threads, cchunk], capture_output=True, text=True, timeout=300).stdout.strip()
        assert out.startswith("ok"), (name, threads, cchunk, out)
    for seed in ("1", "2"):
        r = subprocess.run([exes["gap_check"], str(f), seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and " 0 wrong" in r.stdout, (name, r.stdout[-1500:], r.stderr[-500:])
    r = subprocess.run([exes["model"], str(f), "768", "6", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (name, r.stdout[-1500:], r.stderr[-500:])
