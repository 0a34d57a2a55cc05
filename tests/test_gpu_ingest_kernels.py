"""The kernels that take over from the device DEFLATE decoder -- all of mitoflex_amd/csrc/mf_ingest.hip (the u32 -> u64 scan, the newline
count and line index, the sequence lengths, the 2-bit pack with its list of invalid positions, the survivor gather, the quality filter's
scan / SipHash / decide / keep / gather, the small host <-> device byte copies) and the de-duplication set of mf_kernels.hip -- called
directly through tests/native/ingest_kernel_check.cpp and held to plain host loops, exactly: one JSON line per case, judged here.

The same driver is built twice:
  * with hipcc against build/mf_ingest.o and build/mf_kernels.o: the kernels, on the GPU (the tests marked gpu);
  * with g++ against the stand-in runtime (tests/native/hipstub) and the stand-in loops of tests/native/ingest_stub.cpp: the driver's
    references against a second plain implementation, on the CPU, so that a wrong reference is not met on the GPU first.  The stand-in's
    hash is FNV; there the driver's byte-wise SipHash-1-3 is what is held to oracle.filter_v2_ref.siphash13.
Besides "nothing wrong" every mode asserts that the branches its cases were built for were reached."""
import json
import os
import subprocess

import pytest

from oracle.filter_v2_ref import siphash13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitoflex_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
DRIVER = os.path.join(NATIVE, "ingest_kernel_check.cpp")
MODES = ["scan", "lines", "seqlens", "pack", "select", "qual", "hash", "decide", "dedup", "bytes"]
SCAN_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1, 3 * 256 * 4096 + 5]


def build_gpu(tmp):
    out = os.path.join(tmp, "ingest_kernel_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", CSRC, "-x", "hip", DRIVER, "-x", "none", os.path.join(CSRC, "build", "mf_ingest.o"),
                           os.path.join(CSRC, "build", "mf_kernels.o"), "-o", out])
    return out


def build_host(tmp):
    """the stand-ins of ingest_stub.cpp call the host decoder's speculative chunk: mf_pinflate.cpp is all of the product the link needs"""
    out = os.path.join(tmp, "ingest_kernel_check_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DINGEST_KERNEL_CHECK_STUB", "-I", os.path.join(NATIVE, "hipstub"), "-I", CSRC, DRIVER,
                           os.path.join(NATIVE, "ingest_stub.cpp"), os.path.join(NATIVE, "hipstub", "hipstub.cpp"),
                           os.path.join(CSRC, "mf_pinflate.cpp"), "-lz", "-lpthread", "-o", out])
    return out


def run(drv, mode, timeout):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}          # (MF_SMALL_*_ON_ENGINE would take the copy kernels out)
    r = subprocess.run([drv, mode], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert recs and recs[-1] == {"mode": mode, "done": 1}, (mode, r.stdout[-500:])
    return recs[:-1]


def all_right(recs, mode):
    """every case of a mode: every count of wrong values, whatever it counts, is 0, and so is canary_wrong"""
    assert recs
    for rec in recs:
        assert rec["mode"] == mode
        counts = [k for k in rec if k.endswith("_wrong") or k == "wrong"]
        assert "canary_wrong" in counts and len(counts) >= 2 or "fixed" in rec, rec
        for k in counts:
            assert rec[k] == 0, (k, json.dumps(rec))


def judge_scan(recs, device):
    all_right(recs, "scan")
    assert {(r["n"], r["values"]) for r in recs} == {(n, v) for n in SCAN_SIZES for v in ("zero", "one", "max", "random")}
    assert sum(r["partials"] > 256 for r in recs) >= 4 * 2          # the carry loop of scan_partials_kernel
    assert any(r["partials"] > 2 * 256 for r in recs)


def judge_lines(recs, device):
    all_right(recs, "lines")
    assert {r["n"] for r in recs} == {1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5, 1000003}
    assert {r["pattern"] for r in recs} == {"none", "all", "tile_edges", "lane_edges", "random_closed", "random_open"}
    assert all(r["offsets"] == 16 for r in recs)
    assert any(r["newlines"] == 0 for r in recs) and any(r["newlines"] == r["n"] for r in recs)
    assert any(not r["ends_in_newline"] and r["newlines"] for r in recs)


def judge_seqlens(recs, device):
    all_right(recs, "seqlens")
    assert {r["n_rec"] for r in recs} == {1, 63, 64, 65, 255, 256, 257, 1000}
    assert {(r["crlf"], r["open_end"]) for r in recs} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert sum(r["empty_lines"] for r in recs) > 0 and sum(r["cr_only_lines"] for r in recs) > 0


def judge_pack(recs, device):
    all_right(recs, "pack")
    bases = {0, 1, 15, 16, 17, 65533}
    assert {r["base"] for r in recs if r["uniform_len"] == 0} == bases and {r["base"] for r in recs if r["uniform_len"]} == bases
    assert {r["uniform_len"] for r in recs} == {0, 1, 15, 16, 17, 31, 150, 151, 5000}
    assert any(r["base"] & 15 and r["shared_word_invalid"] for r in recs)          # an invalid base in the word shared with the batch in front
    assert any(r["fast_words"] for r in recs) and any(r["border_words"] for r in recs)
    assert any(r["empty_runs"] >= 3 for r in recs) and any(r["blocks"] > 1 for r in recs)
    assert any(r["total_bases"] == 0 for r in recs) and any(r["invalid"] > 256 for r in recs)


def judge_select(recs, device):
    all_right(recs, "select")
    assert {r["sel_memory"] for r in recs} == {"pinned", "device"}
    assert {1, 3, 4, 5} <= {r["n_sel"] for r in recs}
    assert {r["text"] for r in recs} == {"lf", "crlf", "plus_text", "lf_open_end", "crlf_open_end"}
    assert {r["list"] for r in recs} >= {"one_first", "one_last", "all", "every_third"}


def judge_qual(recs, device):
    all_right(recs, "qual")
    full = 2 ** 64 - 1
    assert {(r["start"], r["cap"], r["quality"], r["ns"]) for r in recs} == {(s, c, q, n) for s in (0, 1, 5, 20000) for c in (0, 1, 7, full)
                                                                                  for q in (1, 33, 55, 100) for n in (0, 1, full)}
    for r in recs:
        assert r["plus_line_flagged"] == 0 and r["n_rec"] % 32 != 0 and r["flag_high"] >= 3, json.dumps(r)
    assert any(r["short_seq_only"] for r in recs) and any(r["short_qual_only"] for r in recs)
    assert any(r["flag_nfail"] for r in recs) and any(r["first_flag"] > 0 for r in recs)
    assert {r["with_dup"] for r in recs} == {0, 1} and {r["with_keep"] for r in recs} == {0, 1} and {r["crlf"] for r in recs} == {0, 1}


def judge_hash(recs, device):
    all_right(recs, "hash")
    runs = [r for r in recs if "fixed" not in r]
    assert {r["start"] for r in runs} == {0, 3} and any(r["short_records"] for r in runs)
    for r in runs:
        assert r["align_x_tail"] == 2 ** 32 - 1, json.dumps(r)          # every alignment of the cut's first byte x every tail length
    (fixed,) = [r["fixed"] for r in recs if "fixed" in r]
    assert len(fixed) >= 8 and {len(f["seq"]) % 8 for f in fixed} >= {0, 1, 4, 6, 7}
    for f in fixed:
        want = siphash13(f["seq"].encode() + b"\xff")
        assert int(f["reference"], 16) == want, f          # the driver's byte-wise SipHash-1-3
        if device:
            assert int(f["device"], 16) == want, f         # the kernel's value, as a value


def judge_decide(recs, device):
    all_right(recs, "decide")
    assert {(r["pe"], r["trunc"]) for r in recs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r["limit"] for r in recs} == {"0", "0.1", "0.2", "0.25", "0.99", "1", "-1", "nan", "1e+30"}
    assert any(r["product_on_integer"] for r in recs if r["limit"] in ("0.1", "0.2"))
    for r in recs:
        assert r["alive"] == r["n"] if r["trunc"] else r["alive"] < r["n"], json.dumps(r)


def judge_dedup(recs, device):
    all_right(recs, "dedup")
    assert len(recs) >= 5 and recs[0]["slots"] == 16 and recs[0]["same_slot_keys"] >= 4
    assert any(r["rehashes"] and r["keys_before"] for r in recs) and recs[-1]["rehashes_with_keys"] >= 1          # a rehash with keys in the table
    assert recs[-1]["max_copies"] >= 200 and recs[-1]["zero_seen"] == 1 and sum(r["duplicates"] for r in recs) > 500
    for r in recs:
        assert 2 * r["keys_after"] <= r["slots"] and 2 * (r["keys_before"] + r["n"]) <= r["slots"], json.dumps(r)


def judge_bytes(recs, device):
    all_right(recs, "bytes")
    assert {r["n"] for r in recs} == {1, 8, 15, 16, 17, 4096, 2 ** 20, 2 ** 20 + 3}
    assert {(r["direction"], r["path"]) for r in recs} == {(d, p) for d in ("to_host", "from_host") for p in ("uint4", "byte")}


JUDGES = {"scan": judge_scan, "lines": judge_lines, "seqlens": judge_seqlens, "pack": judge_pack, "select": judge_select, "qual": judge_qual,
          "hash": judge_hash, "decide": judge_decide, "dedup": judge_dedup, "bytes": judge_bytes}


@pytest.fixture(scope="module")
def drv(built_lib, tmp_path_factory):
    return build_gpu(str(tmp_path_factory.mktemp("ingest_kernels")))


@pytest.fixture(scope="module")
def host_drv(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("ingest_kernels_host")))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_ingest_kernels(drv, mode):
    """(the time limit is a safety cap: a mode needs seconds)"""
    JUDGES[mode](run(drv, mode, 600), True)


@pytest.mark.parametrize("mode", MODES)
def test_driver_references_on_the_host(host_drv, mode):
    JUDGES[mode](run(host_drv, mode, 600), False)
