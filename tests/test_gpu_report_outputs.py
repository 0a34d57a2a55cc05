"""The optional outputs of the placement family -- mf_place, mf_pileup, mf_verify and their file-level calls -- which share one report
(mitoflex_amd/csrc/mf_report.cpp: placement_report).  The C functions are called directly: a call that leaves an output NULL gives
every other output bit for bit as the call with every output does, and touches nothing of what it was not given.  What the outputs
hold is pinned elsewhere (test_gpu_place.py, test_gpu_pileup.py, test_gpu_verify.py); nothing here has a tolerance or a timing."""
import ctypes as C

import numpy as np
import pytest

from tests.report_data import fasta, mf, mutate, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_place import place_bait, place_reads
from tests.test_gpu_verify import drawn

pytestmark = pytest.mark.gpu

K, THR, MIN_DEPTH, GUARD = 21, 1, 2, 0xA5
PLACE_OUT = ("base_depth", "place_records", "unplaced")
PILEUP_OUT = ("pileup", "consensus", "pileup_records", "unplaced")
VERIFY_OUT = ("base_depth", "place_records", "pileup", "consensus", "pileup_records", "score_records", "unplaced")
# family: (resident call, its outputs in C order, file-level call, its outputs in C order, takes min_depth, takes max_permille)
FAMILIES = {
    "place": ("mf_place", ("bits", "place") + PLACE_OUT, "mf_filter_fastq_files_placed", PLACE_OUT, False, False),
    "pileup": ("mf_pileup", ("bits",) + PILEUP_OUT, "mf_filter_fastq_files_pileup", PILEUP_OUT, True, False),
    "verify": ("mf_verify", ("bits", "place", "score") + VERIFY_OUT, "mf_filter_fastq_files_verified", VERIFY_OUT, True, True),
}
CASES = [("place", 1000), ("pileup", 1000), ("verify", 1000), ("verify", 20)]


def byte_sizes(ks, n):
    """bytes of every output for a set and n reads"""
    starts = ks.record_starts
    P, R = int(starts[-1]), len(starts) - 1
    return {"bits": 4 * ((n + 31) // 32), "place": 24 * n, "score": 8 * n, "base_depth": 4 * P, "place_records": 48 * R, "pileup": 16 * P,
            "consensus": P, "pileup_records": 48 * R, "score_records": 8 * (4 + 32) * R, "unplaced": 16}


def call(lib, fn, head, names, sizes, tail, null=()):
    """fn(*head, outputs.., *tail) with the outputs of `null` NULL -> {name: its bytes, or None}; a NULL output's guard array is untouched"""
    bufs = {f: np.full(max(sizes[f], 1), GUARD, dtype=np.uint8) for f in names}
    rc = getattr(lib, fn)(*head, *[None if f in null else bufs[f].ctypes.data for f in names], *tail)
    assert rc == 0, (fn, sorted(null), lib.mf_last_error().decode(errors="replace"))
    for f in null:
        assert (bufs[f] == GUARD).all(), (fn, f, "was NULL and its guard array changed")
    return {f: None if f in null else bufs[f][:sizes[f]] for f in names}


def equal_where_given(got, full, what):
    for f, b in got.items():
        assert b is None or np.array_equal(b, full[f]), (what, f)


def cuts(family, max_permille):
    return ((MIN_DEPTH,) if FAMILIES[family][4] else ()) + ((max_permille,) if FAMILIES[family][5] else ())


@pytest.fixture(scope="module")
def data(mf, ol):
    """the placement tests' bait at k = 21, their special reads, 200 ragged ones and 24 of a copy mutated at 2 %, which a cut rejects"""
    text, parts = place_bait()
    _, seqs = place_reads(text, parts, K, 200, seed=2101, uniform=False)
    seqs = [s or "A" for s in seqs] + drawn(mutate(parts["g"], 0.02, 5), 24, seed=6)
    ks = mf.KmerSet.from_text(text, K)
    reads = upload(mf, ol, seqs)
    yield ks, reads, seqs
    reads.close()
    ks.close()


def resident_full(mf, ks, reads, n, family, max_permille):
    fn, names = FAMILIES[family][:2]
    head = (ks._h, reads._h, THR, mf.MODE_SCREENED) + cuts(family, max_permille)
    sizes = byte_sizes(ks, n)
    return fn, names, head, sizes, call(mf.load(), fn, head, names, sizes, (None,))


@pytest.mark.parametrize("family,max_permille", CASES)
def test_resident_call_with_an_output_left_out(mf, data, family, max_permille):
    ks, reads, seqs = data
    fn, names, head, sizes, full = resident_full(mf, ks, reads, len(seqs), family, max_permille)
    unplaced = full["unplaced"].view(np.uint64)
    assert unplaced[0] >= 1 and unplaced[1] >= 1          # the input holds a passing read that is not placed and a read that does not pass
    if family == "verify":
        rejected = int(full["score_records"].view(mf.SCORE_RECORD)["rejected"].sum())
        assert (rejected > 0) == (max_permille == 20)          # the cut cuts
    for left_out in [(f,) for f in names] + [tuple(f for f in names if f != "unplaced")]:
        got = call(mf.load(), fn, head, names, sizes, (None,), null=left_out)
        equal_where_given(got, full, (fn, max_permille, left_out))


@pytest.mark.parametrize("family,max_permille", CASES)
def test_file_level_call_with_only_unplaced(mf, data, tmp_path, monkeypatch, family, max_permille):
    """one plain-text pair on the host ingest path: every mate that passes is placed, so the full call gives what the resident call on
    all the mates gives; the call with only `unplaced` gives the same `unplaced`, the same counts and the same files"""
    from tests.util_data import write_fastq
    monkeypatch.setenv("MF_INGEST", "host")
    ks, reads, seqs = data
    half = len(seqs) // 2
    fq1, fq2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    write_fastq(fq1, seqs[:half], "a")
    write_fastq(fq2, seqs[half:2 * half], "b")
    assert 2 * half == len(seqs)
    fn, names = FAMILIES[family][2:4]
    sizes = byte_sizes(ks, 0)
    devices = (C.c_int * 1)(0)
    results = []
    for tag, null in (("full", ()), ("only", tuple(f for f in names if f != "unplaced"))):
        out1, out2 = str(tmp_path / (tag + "_1.fq")), str(tmp_path / (tag + "_2.fq"))
        kept, total = C.c_uint64(), C.c_uint64()
        head = (ks._h, fq1.encode(), fq2.encode(), out1.encode(), out2.encode(), THR, mf.PAIR_EITHER, devices, 1) + cuts(family, max_permille)
        got = call(mf.load(), fn, head, names, sizes, (C.byref(kept), C.byref(total)), null=null)
        assert mf.last_ingest_stats()["path"] == 0
        results.append((got, kept.value, total.value, open(out1, "rb").read(), open(out2, "rb").read()))
    (full, *rest_full), (only, *rest_only) = results
    assert rest_full == rest_only and rest_full[1] == half
    equal_where_given(only, full, (fn, max_permille))
    resident = resident_full(mf, ks, reads, len(seqs), family, max_permille)[4]
    equal_where_given(full, resident, (fn, max_permille, "against the resident call"))


def test_set_with_an_empty_last_record(mf, ol):
    """two records, the second empty: one call of each resident function with every output, against the Python wrappers'"""
    text, parts = place_bait()
    g = parts["g"][:600]
    ks = mf.KmerSet.from_text(fasta([("one", g), ("void", "")]), K)
    assert ks.record_starts.tolist() == [0, 600, 600]
    seqs = drawn(g, 40, seed=9, lo=60, hi=120) + drawn(parts["left"], 8, seed=10, lo=60, hi=120) + [g[100:160] + "N" + g[400:460]]
    reads = upload(mf, ol, seqs)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).ravel()
    want = {}
    bits, place, base_depth, place_records, unplaced = mf.place_reads(ks, reads, THR)
    want["place"] = dict(bits=bits, place=place, base_depth=base_depth, place_records=place_records, unplaced=unplaced)
    bits, pileup, consensus, pileup_records, unplaced = mf.pileup_reads(ks, reads, THR, min_depth=MIN_DEPTH)
    want["pileup"] = dict(bits=bits, pileup=pileup, consensus=consensus, pileup_records=pileup_records, unplaced=unplaced)
    v = mf.verify_reads(ks, reads, THR, min_depth=MIN_DEPTH, max_permille=1000)
    want["verify"] = {f: getattr(v, f) for f in FAMILIES["verify"][1]}
    assert int(want["place"]["place_records"]["forward"][0] + want["place"]["place_records"]["reverse"][0]) > 0
    assert not raw(want["place"]["place_records"][1:]).any() and not raw(want["pileup"]["pileup_records"][1:]).any()
    for family in ("place", "pileup", "verify"):
        full = resident_full(mf, ks, reads, len(seqs), family, 1000)[4]
        for f, b in full.items():
            assert np.array_equal(b, raw(want[family][f])), (family, f)
    reads.close()
    ks.close()
