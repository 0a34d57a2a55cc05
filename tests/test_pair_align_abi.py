"""The aligning paired entry point of the C ABI without a GPU: the symbol loads and is exported, and every refusal that needs no handle --
everything mf_place_pairs refuses on its numbers, a band above 31, an extend above MF_EXTEND_MAX, extension outputs with extend == 0 --
comes back as MF_E_ARG with a message that names the value, before any device is touched, with no output written and with the numbers
checked before the handles.  The Python surfaces refuse the same with ValueError before they reach the library.  (A band that is not
below k, a protein set, unequal n_reads and sets on different devices need handles, which need a device: tests/test_gpu_pair_align.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

MF_E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_the_symbol_loads_and_the_abi_is_5(lib):
    from mitoflex_amd import mitofilter as mf
    assert hasattr(lib, "mf_align_pairs") and "mf_align_pairs" in mf.EXPORTS and callable(mf.align_pairs)
    assert lib.mf_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "mitofilter.h")).read()
    assert "#define MF_ABI_VERSION 5" in header and "int mf_align_pairs(" in header
    assert header.index("int mf_place_pairs(") < header.index("pairs with a band") < header.index("int mf_align_pairs(")
    p = mf.AlignedPairs(pairs_none=3)
    assert p.pairs_none == 3 and p.align1 is None and p.gapped is None and p.bits is None and p.keep_bits is None and isinstance(p, mf.Aligned)
    assert len(lib.mf_align_pairs.argtypes) == 39


def test_bad_arguments_are_refused_before_any_device_work(lib):
    u32 = lambda n, v: (C.c_uint32 * n)(*([v] * n))
    bits, place, align, pairs, depth = u32(2, 9), u32(6, 8), u32(6, 7), u32(2, 5), u32(4, 2)
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    indels, arec, prec = u32(12, 4), (C.c_uint64 * 39)(*([1] * 39)), (C.c_uint64 * 6)(*([3] * 6))
    ext, extended, xstarts, xrec = u32(64, 6), (C.c_uint8 * 64)(*([6] * 64)), (C.c_uint64 * 2)(6, 6), (C.c_uint64 * 5)(*([6] * 5))
    none = C.c_uint64(11)
    unplaced = (C.c_uint64 * 2)(6, 6)

    def call(min_insert=200, max_insert=400, rescue=1, rescue_permille=100, min_depth=1, max_permille=1000, band=8, extend=0, outs=(None, None, None, None)):
        return lib.mf_align_pairs(None, None, None, 1, 0, min_depth, max_permille, band, extend, min_insert, max_insert, rescue, rescue_permille, bits, bits,
                                  place, place, align, align, pairs, depth, None, None, cons, None, indels, arec, None, None, None, None, *outs, prec,
                                  C.byref(none), unplaced, None)

    def refused(word, **kw):
        assert call(**kw) == MF_E_ARG, kw
        assert word in lib.mf_last_error(), (kw, lib.mf_last_error())

    refused(b"NULL")
    # everything mf_place_pairs refuses
    refused(b"insert", min_insert=0)
    refused(b"insert", min_insert=401)
    refused(b"insert", min_insert=1, max_insert=4097)
    refused(b"NULL", min_insert=1, max_insert=4096)
    refused(b"insert", min_insert=2 ** 31 - 4095, max_insert=2 ** 31)
    refused(b"rescue is 2", rescue=2)
    refused(b"rescue is -1", rescue=-1)
    refused(b"NULL", rescue=0)
    refused(b"rescue_permille is 1001", rescue_permille=1001)
    refused(b"max_permille is 1001", max_permille=1001)
    refused(b"min_depth is 0", min_depth=0)
    # what the aligning, gapped and extending requests refuse
    refused(b"band is 32", band=32)
    refused(b"NULL", band=31)
    refused(b"NULL", band=0)
    refused(b"extend is 4097", extend=4097)
    refused(b"NULL", extend=4096, outs=(ext, extended, xstarts, xrec))
    for i in range(4):          # any extension output with extend == 0
        outs = [None] * 4
        outs[i] = (ext, extended, xstarts, xrec)[i]
        refused(b"extend is 0", outs=tuple(outs))
    # the numbers before the handles, in the order the calls check them: the pair numbers, the family's, then the handles
    refused(b"insert", min_insert=0, band=32)
    refused(b"band is 32", band=32, extend=4097)
    assert list(bits) == [9, 9] and list(place) == [8] * 6 and list(align) == [7] * 6 and list(pairs) == [5, 5] and list(depth) == [2] * 4
    assert list(cons) == [5] * 4 and list(indels) == [4] * 12 and list(arec) == [1] * 39 and list(prec) == [3] * 6 and none.value == 11
    assert list(unplaced) == [6, 6] and list(ext) == [6] * 64 and list(extended) == [6] * 64 and list(xstarts) == [6, 6] and list(xrec) == [6] * 5


def test_the_python_surfaces_check_their_numbers_before_the_library(tmp_path):
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.bim import bim
    window = {"min_insert": 1, "max_insert": 10}
    for kw, word in (({"min_insert": 0, "max_insert": 10}, "insert"), ({"min_insert": 11, "max_insert": 10}, "insert"), ({"min_insert": 1, "max_insert": 4097}, "insert"),
                     (dict(window, rescue_permille=1001), "rescue_permille"), (dict(window, max_permille=1001), "max_permille"), (dict(window, min_depth=0), "min_depth"),
                     (dict(window, band=32), "band"), (dict(window, band=-1), "band"), (dict(window, extend=4097), "extend"), (dict(window, extend=-1), "extend")):
        with pytest.raises(ValueError, match=word):
            mf.align_pairs(None, None, None, **kw)
    bait, out = str(tmp_path / "bait.fa"), str(tmp_path / "out.fa")
    for kw, word in (({"band": 32}, "band"), ({"band": 31, "kmer": 31}, "band"), ({"band": None}, "band"), ({"extend": 4097}, "extend"), ({"min_insert": 5}, "together"),
                     ({"min_insert": 0, "max_insert": 5}, "insert"), ({"min_insert": 1, "max_insert": 4097}, "insert"), ({"rescue_permille": 1001}, "rescue_permille"),
                     ({"max_permille": 1001}, "max_permille"), ({"min_depth": 0}, "min_depth")):
        with pytest.raises(ValueError, match=word):
            bim.consensus_bait_pairs(bait, "a.fq", "b.fq", out, **kw)
    with pytest.raises(ValueError, match="two files"):
        bim.consensus_bait_pairs(bait, "a.fq", None, out)
    with pytest.raises(ValueError, match="overwrite"):
        bim.consensus_bait_pairs(bait, "a.fq", "b.fq", bait)
    assert not os.path.exists(out)
