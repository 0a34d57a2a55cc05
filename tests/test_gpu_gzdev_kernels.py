"""The kernels of the device DEFLATE decoder (mitoflex_amd/csrc/mf_gzdev.hip) called directly and held to zlib, through
tests/native/gzdev_kernel_check.cpp (one JSON line per case):
  * launch_gz_decode -- the lane-parallel kernel and, in a process of its own, the one-lane walk (MF_GZDEV_KERNEL=serial) -- on the
    corpus of tests/deflate_writer.py at the product's chunk sizes: every chunk that starts at a true block boundary (zlib's Z_BLOCK
    mode) has zlib's symbols, stops at a true boundary with the right count and status, whether or not the link walk keeps it; the
    exact chunk never fails; every accepted chunk starts at a true boundary; linked text and window equal zlib's.  Then the ring, a
    limit, exact restarts in front of stored / fixed / dynamic blocks and a symbol buffer that overflows;
  * launch_gz_link + launch_gz_resolve on synthetic chunks: every group size of the scan, short windows, bodies or none, a text base;
  * launch_gz_crc + gz_crc_finish and gz_crc_combine against zlib's crc32."""
import json
import os
import subprocess

import pytest

from tests import deflate_writer as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitoflex_amd", "csrc")
CHUNKS = "1024,4096,65536,196608"           # the product's range of chunk sizes


@pytest.fixture(scope="module")
def drv(built_lib, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gzdev") / "gzdev_kernel_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", CSRC, "-x", "hip", os.path.join(ROOT, "tests", "native", "gzdev_kernel_check.cpp"), "-x", "none",
                           os.path.join(CSRC, "build", "mf_gzdev.o"), "-lz", "-o", out])
    return out


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_corpus")
    for name, (gz, _, _, _) in W.corpus().items():
        (d / (name + ".gz")).write_bytes(gz)
    return d


def run(drv, args, kernel, timeout):
    env = dict(os.environ)
    env.pop("MF_GZDEV_KERNEL", None)
    if kernel == "serial":
        env["MF_GZDEV_KERNEL"] = "serial"
    r = subprocess.run([drv] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (args[:6], r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def item(rec):
    return os.path.basename(rec["file"])[:-3]


def assert_right(rec, need_verified=True):
    """what holds for every decode case: no wrong symbol or stop, nothing accepted that is not a true start, zlib's text and window"""
    ctx = json.dumps(rec)
    assert "error" not in rec, ctx
    assert rec["wrong"] == 0 and rec["bad_end"] == 0, ctx
    assert rec["accepted_not_true"] == 0 and rec["limit_violations"] == 0, ctx
    assert rec["text_wrong"] == 0 and rec["window_wrong"] == 0, ctx
    assert rec["verified"] >= 1 or not need_verified, ctx


@pytest.mark.parametrize("kernel", ["lanes", "serial"])
def test_decode_corpus(drv, corpus_dir, kernel):
    c = W.corpus()
    files = [str(corpus_dir / (n + ".gz")) for n in c]
    recs = run(drv, ["decode", "--chunks", CHUNKS] + files, kernel, 1200)
    assert len(recs) == 4 * len(files)
    for rec in recs:
        assert rec["kernel"] == kernel
        assert_right(rec)
        assert rec["exact_ok"], json.dumps(rec)
        tags = c[item(rec)][3]
        if rec["chunk"] <= 4096 and rec["chunks"] > 1:
            if "spec" in tags:          # chunks behind the first searched their range, found a true dynamic block and were verified from it
                assert rec["verified_nonfirst"] >= 1, json.dumps(rec)
                if not rec["hist"][4]:  # (and linked on the device, unless chunk 0 overflowed: a chunk of overlapping copies is 200 KB of text)
                    assert rec["linked_chunks"] >= 2, json.dumps(rec)
            if "far" in tags:           # a match that reaches back 32 507..32 768 bytes across a chunk's start: a marker below 262, resolved right
                assert 0 <= rec["min_marker"] < 262, json.dumps(rec)
    # the full-window items at 1 KiB: markers below 262 in several verified chunks, and everything they decode linked on the device
    for rec in recs:
        if item(rec) == "full_window_32768" and rec["chunk"] == 1024:
            assert rec["min_marker"] == 0 and rec["linked_chunks"] > 10, json.dumps(rec)


MODE_CASES = [
    # (args, items, what the case must reach)
    (["--ring", "65536", "--chunks", "4096"], ["full_window_32768", "overlapping_copies", "empty_and_stored", "zlib_level1", "tiny_blocks"], "ring"),
    (["--ring", "1048576", "--chunks", "65536"], ["zlib_mem1", "fixed_top_codes"], "ring"),
    (["--limit", "20000", "--chunks", "1024,4096"], ["full_window_32507", "long_lit_codes", "zlib_huffman_only", "empty_and_stored"], "limit"),
    (["--exact-kind", "stored", "--chunks", "1024,4096"], ["empty_and_stored", "tiny_blocks"], "exact"),
    (["--exact-kind", "fixed", "--chunks", "1024,4096"], ["fixed_top_codes", "tiny_blocks"], "exact"),
    (["--exact-kind", "dynamic", "--chunks", "1024,4096"], ["full_window_32600", "small_alphabets", "zlib_mem1"], "exact"),
    (["--cap", "20000", "--chunks", "4096,65536"], ["overlapping_copies", "full_window_32767", "empty_and_stored"], "overflow"),
]


@pytest.mark.parametrize("kernel", ["lanes", "serial"])
def test_decode_modes(drv, corpus_dir, kernel):
    """the ring (slab by slab, each with the bytes uploaded so far as its limit), a limit (the same chunks decoded with and without it
    must agree as the limit's rules say), exact restarts mid-stream in front of each block kind (chunk_lo > 0), and symbol buffers
    too small for a chunk's blocks (OVERFLOW at the last boundary that fitted)"""
    seen = {"ring": 0, "limit": 0, "exact": 0, "overflow": 0, "limit_failed": 0}
    for args, items, what in MODE_CASES:
        recs = run(drv, ["decode"] + args + [str(corpus_dir / (n + ".gz")) for n in items], kernel, 600)
        assert len(recs) == len(items) * len(args[-1].split(","))
        for rec in recs:
            assert_right(rec, what not in ("limit", "ring"))          # (behind a limit, every chunk of a file may need more bytes)
            if what in ("limit", "ring"):  # (the exact chunk may need bytes behind the limit: it fails with reason 8 and the host bridges)
                seen["limit_failed"] += rec["hist"][3] > 0
                assert rec["exact_ok"] or rec["exact_past_limit"], json.dumps(rec)
            else:
                assert rec["exact_ok"], json.dumps(rec)
            if what == "exact":
                assert rec["chunk_lo"] > 0 and rec["verified"] >= 1, json.dumps(rec)
            if what == "overflow" and rec["hist"][4]:
                assert rec["overflow_verified"] >= 1, json.dumps(rec)
                seen["overflow"] += 1
            seen[what] += what != "overflow"
    assert seen["overflow"] >= 2 and seen["limit_failed"] >= 1, seen


def test_link_kernels(drv):
    recs = run(drv, ["link", "1", "2", "3", "4", "5"], "lanes", 600)
    assert len(recs) == 5 * 19
    for rec in recs:
        assert rec["text_wrong"] == 0 and rec["window_wrong"] == 0, json.dumps(rec)
    groups = {rec["group"] for rec in recs}
    assert groups == {4, 8, 16, 32}
    assert {1, 4, 5, 16, 17, 64, 65, 512, 513} <= {rec["n_acc"] for rec in recs}
    assert any(rec["wlen_before"] < 32768 for rec in recs) and any(rec["wlen_before"] == 32768 for rec in recs)
    assert any(rec["max_sym"] <= 32768 for rec in recs) and any(rec["max_sym"] > 32768 for rec in recs)
    assert any(rec["text_base"] != 0 for rec in recs) and any(rec["text_base"] == 0 for rec in recs)
    assert any(rec["slabs"] > 1 for rec in recs) and sum(rec["far_markers"] for rec in recs) > 0


def test_crc_kernel(drv):
    (rec,) = run(drv, ["crc"], "lanes", 300)
    assert rec["crc_wrong"] == 0 and rec["combine_wrong"] == 0, rec
    assert rec["crc_cases"] >= 3 * (10 * 11 + 2 * 1) and rec["combine_cases"] == 25
