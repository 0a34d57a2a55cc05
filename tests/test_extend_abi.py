"""The extended-record entry points without a GPU: the two symbols load and are exported, the record type has the stated layout, NULL
handles and bad arguments -- extend above MF_EXTEND_MAX, extend == 0 with one of the four new outputs -- are refused with MF_E_ARG before
any device is touched and leave every output as it was, the wrappers check their arguments before the library, and mf.extended_consensus
is held to the oracle's call.  A protein set needs a set, and a set needs a device: tests/test_gpu_extend.py holds that refusal."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import extend_data as xd
from tests import extend_oracle as xo
from tests import place_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mf_align_extended", "mf_filter_fastq_files_extended")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    header = open(os.path.join(ROOT, "include", "mitofilter.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
        assert name in header
    assert "typedef struct { uint64_t length, begin_bases, end_bases, begin_piled, end_piled; } mf_extend_record_t;" in header
    assert "#define MF_EXTEND_MAX 4096" in header and mitofilter.EXTEND_MAX == 4096
    assert mitofilter.EXTEND_RECORD.names == ("length", "begin_bases", "end_bases", "begin_piled", "end_piled")
    assert mitofilter.EXTEND_RECORD.itemsize == 40          # sizeof(mf_extend_record_t)
    assert all(mitofilter.EXTEND_RECORD[f] == np.uint64 for f in mitofilter.EXTEND_RECORD.names)
    assert callable(mitofilter.extended_consensus)
    a = mitofilter.Aligned(kept=3, total=4)
    assert (a.ext_pile, a.extended, a.extended_starts, a.extend_records, a.gapped) == (None, None, None, None, None)
    assert lib.mf_abi_version() == 5
    for f in (mitofilter.align_reads, mitofilter.filter_fastq_files_aligned):
        p = inspect.signature(f).parameters["extend"]
        assert p.default == 0


def test_null_handles_and_bad_arguments_are_refused(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    keep_bits = (C.c_uint32 * 2)(5, 5)
    place = (C.c_uint32 * 6)(*([8] * 6))
    align = (C.c_uint32 * 6)(*([7] * 6))
    depth = (C.c_uint32 * 4)(2, 2, 2, 2)
    precs = (C.c_uint64 * 6)(*([1] * 6))
    pile = (C.c_uint32 * 8)(*([4] * 8))
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 6)(*([3] * 6))
    indels = (C.c_uint32 * 12)(*([11] * 12))
    arecs = (C.c_uint64 * 39)(*([10] * 39))
    ins = (C.c_uint32 * 16)(*([12] * 16))
    gapped = (C.c_uint8 * 8)(*([13] * 8))
    gstarts = (C.c_uint64 * 2)(14, 14)
    grecs = (C.c_uint64 * 4)(*([15] * 4))
    ext = (C.c_uint32 * 16)(*([16] * 16))
    extended = (C.c_uint8 * 8)(*([17] * 8))
    xstarts = (C.c_uint64 * 2)(18, 18)
    xrecs = (C.c_uint64 * 5)(*([19] * 5))
    unplaced = (C.c_uint64 * 2)(6, 6)
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)
    new = (ext, extended, xstarts, xrecs)

    def resident(min_depth, max_permille, keep, band, extend, more=new):
        return lib.mf_align_extended(None, None, 1, 0, min_depth, max_permille, keep, band, extend, bits, keep_bits, place, align, depth, precs, pile, cons, recs,
                                     indels, arecs, ins, gapped, gstarts, grecs, *more, unplaced, None)

    def files(min_depth, max_permille, keep, band, extend, more=new):
        return lib.mf_filter_fastq_files_extended(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, min_depth, max_permille, keep, band, extend, depth, precs,
                                                  pile, cons, recs, indels, arecs, ins, gapped, gstarts, grecs, *more, unplaced, C.byref(kept), C.byref(total))

    for call in (resident, files):
        assert call(1, 1000, 0, 8, 64) == MF_E_ARG
        assert b"NULL handle" in lib.mf_last_error()
        assert call(1, 1000, 0, 8, 4096) == MF_E_ARG
        assert b"NULL handle" in lib.mf_last_error()
        assert call(1, 1000, 0, 8, 0, (None,) * 4) == MF_E_ARG          # extend == 0: the gapped call, which a NULL handle stops
        assert b"NULL handle" in lib.mf_last_error()
        for extend in (4097, 0xFFFFFFFF):
            assert call(1, 1000, 0, 8, extend) == MF_E_ARG
            assert b"extend" in lib.mf_last_error()
        for i in range(4):                                               # extend == 0 with any one of the four new outputs
            one = tuple(new[q] if q == i else None for q in range(4))
            assert call(1, 1000, 0, 8, 0, one) == MF_E_ARG
            assert b"extend is 0" in lib.mf_last_error()
        assert call(1, 1001, 0, 8, 64) == MF_E_ARG
        assert b"max_permille" in lib.mf_last_error()
        assert call(0, 30, 0, 8, 64) == MF_E_ARG
        assert b"min_depth" in lib.mf_last_error()
        assert call(1, 30, 3, 8, 64) == MF_E_ARG
        assert b"keep" in lib.mf_last_error()
        assert call(1, 30, 0, 32, 64) == MF_E_ARG
        assert b"band" in lib.mf_last_error()
    assert list(bits) == [9, 9] and list(keep_bits) == [5, 5] and list(place) == [8] * 6 and list(align) == [7] * 6 and list(depth) == [2] * 4
    assert list(precs) == [1] * 6 and list(pile) == [4] * 8 and list(cons) == [5] * 4 and list(recs) == [3] * 6 and list(indels) == [11] * 12
    assert list(arecs) == [10] * 39 and list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)
    assert list(ins) == [12] * 16 and list(gapped) == [13] * 8 and list(gstarts) == [14, 14] and list(grecs) == [15] * 4
    assert list(ext) == [16] * 16 and list(extended) == [17] * 8 and list(xstarts) == [18, 18] and list(xrecs) == [19] * 5


def test_the_wrappers_check_before_the_library(tmp_path):
    from mitoflex_amd import mitofilter
    from mitoflex_amd.bim import bim
    for extend in (4097, -1):
        with pytest.raises(ValueError, match="extend"):
            mitofilter.align_reads(None, None, band=4, extend=extend)
        with pytest.raises(ValueError, match="extend"):
            mitofilter.filter_fastq_files_aligned(None, "a.fq", None, "o.fq", None, band=4, extend=extend)
    with pytest.raises(ValueError, match="band"):
        mitofilter.align_reads(None, None, band=32, extend=16)
    fa = str(tmp_path / "bait.fa")
    with pytest.raises(ValueError, match="extend needs a band"):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), extend=64)
    with pytest.raises(ValueError, match="extend needs a band"):
        bim.kmer_bait_map(1, fa, str(tmp_path), "p", "a.fq", "b.fq", keep=1, extend=64)
    with pytest.raises(ValueError, match="extend"):
        bim.consensus_bait(fa, "a.fq", "b.fq", str(tmp_path / "out.fa"), band=4, extend=5000)
    assert not os.path.exists(str(tmp_path / "out.fa"))
    gstarts = np.array([0, 3], np.uint64)
    ext = np.zeros((1, 2, 4), mitofilter.PILEUP)
    got = mitofilter.extended_consensus(np.frombuffer(b"acg", np.uint8), gstarts, ext)
    assert bytes(got[0]) == b"acg" and got[1].tolist() == [0, 3] and got[2].tolist() == [(3, 0, 0, 0, 0)]
    with pytest.raises(ValueError, match="min_depth"):
        mitofilter.extended_consensus(np.frombuffer(b"acg", np.uint8), gstarts, ext, min_depth=0)
    with pytest.raises(ValueError, match="PILEUP"):
        mitofilter.extended_consensus(np.frombuffer(b"acg", np.uint8), gstarts, np.zeros((2, 2, 4), mitofilter.PILEUP))
    with pytest.raises(ValueError, match="shorter"):
        mitofilter.extended_consensus(np.frombuffer(b"ac", np.uint8), gstarts, ext)


@pytest.mark.parametrize("E,min_depth", [(1, 1), (16, 3), (64, 1), (64, 3), (4096, 3)])
def test_extended_consensus_is_the_oracles_call(E, min_depth):
    """the wrapper's restatement of the call against the oracle's, on the oracle's own sums of the `ends` set"""
    from mitoflex_amd import mitofilter
    text, _, _ = xd.ends_bait()
    seqs, _ = xd.ends_reads()
    o = po.PlaceOracle(text, 31)
    want = xo.ExtendOracle(o).run(seqs, o.tally(seqs), 1, xd.CUT, 8, min_depth, E)
    got = mitofilter.extended_consensus(np.frombuffer(want["gapped"], np.uint8), want["gapped_starts"], xd.structured(mitofilter, want["ext_pile"]), min_depth)
    assert bytes(got[0]) == want["extended"] and got[1].tolist() == want["extended_starts"]
    assert [list(map(int, r)) for r in got[2].tolist()] == want["extend_records"]
    assert sum(r[1] + r[2] for r in want["extend_records"]) > 0
