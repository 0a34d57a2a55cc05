"""The paired entry point of the C ABI without a GPU: the symbol loads and is exported, the pair types have the stated layout, and
every refusal that needs no handle -- NULL handles, the insert window, rescue, rescue_permille, max_permille, min_depth -- comes back as
MF_E_ARG with a message that names the argument, before any device is touched and with no output written.  (A protein set, unequal
n_reads and sets on different devices need handles, which need a device: tests/test_gpu_pairs.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

MF_E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_the_symbol_loads_and_the_types_have_the_stated_layout(lib):
    from mitoflex_amd import mitofilter as mf
    assert hasattr(lib, "mf_place_pairs") and "mf_place_pairs" in mf.EXPORTS and callable(mf.place_pairs)
    assert mf.PAIR.names == ("kind", "insert") and mf.PAIR.itemsize == 8 and mf.PAIR["kind"] == np.uint32 and mf.PAIR["insert"] == np.int32
    assert mf.PAIR_RECORD.names == ("proper", "discordant", "cross", "rescued", "single", "insert_sum") and mf.PAIR_RECORD.itemsize == 48
    assert all(mf.PAIR_RECORD[f] == np.uint64 for f in mf.PAIR_RECORD.names)
    assert (mf.PAIR_NONE, mf.PAIR_PROPER, mf.PAIR_DISCORDANT, mf.PAIR_RESCUED_1, mf.PAIR_RESCUED_2, mf.PAIR_SINGLE_1, mf.PAIR_SINGLE_2) == tuple(range(7))
    assert mf.RESCUE_MAX == 4096
    header = open(os.path.join(ROOT, "include", "mitofilter.h")).read()
    assert "#define MF_RESCUE_MAX 4096" in header and "MF_PAIR_SINGLE_2 = 6" in header
    p = mf.Paired(pairs_none=3)
    assert p.pairs_none == 3 and p.place1 is None and p.bits is None and p.keep_bits is None
    assert lib.mf_abi_version() == 5


def test_bad_arguments_are_refused_before_any_device_work(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    place = (C.c_uint32 * 6)(*([8] * 6))
    score = (C.c_uint32 * 2)(7, 7)
    pairs = (C.c_uint32 * 2)(5, 5)
    depth = (C.c_uint32 * 4)(2, 2, 2, 2)
    precs = (C.c_uint64 * 6)(*([1] * 6))
    cons = (C.c_uint8 * 4)(5, 5, 5, 5)
    prec = (C.c_uint64 * 6)(*([3] * 6))
    none = C.c_uint64(11)
    unplaced = (C.c_uint64 * 2)(6, 6)

    def call(min_insert=200, max_insert=400, rescue=1, rescue_permille=100, min_depth=1, max_permille=1000):
        return lib.mf_place_pairs(None, None, None, 1, 0, min_depth, max_permille, min_insert, max_insert, rescue, rescue_permille, bits, bits, place, place,
                                  score, score, pairs, depth, precs, None, cons, None, None, prec, C.byref(none), unplaced, None)

    def refused(word, **kw):
        assert call(**kw) == MF_E_ARG, kw
        assert word in lib.mf_last_error(), (kw, lib.mf_last_error())

    refused(b"NULL")
    refused(b"insert", min_insert=0)
    refused(b"insert", min_insert=401)                          # max_insert < min_insert
    refused(b"insert", min_insert=1, max_insert=4097)           # MF_RESCUE_MAX + 1 inserts
    refused(b"NULL", min_insert=1, max_insert=4096)             # MF_RESCUE_MAX of them pass the window's check
    refused(b"NULL", min_insert=2 ** 31 - 4096, max_insert=2 ** 31 - 1)
    refused(b"insert", min_insert=2 ** 31 - 4095, max_insert=2 ** 31)
    refused(b"rescue", rescue=2)
    refused(b"rescue", rescue=-1)
    refused(b"NULL", rescue=0)
    refused(b"rescue_permille", rescue_permille=1001)
    refused(b"NULL", rescue_permille=0)
    refused(b"max_permille", max_permille=1001)
    refused(b"min_depth", min_depth=0)                          # with a consensus asked for
    assert list(bits) == [9, 9] and list(place) == [8] * 6 and list(score) == [7, 7] and list(pairs) == [5, 5] and list(depth) == [2] * 4
    assert list(precs) == [1] * 6 and list(cons) == [5] * 4 and list(prec) == [3] * 6 and none.value == 11 and list(unplaced) == [6, 6]


def test_the_wrapper_checks_its_numbers_before_the_library():
    from mitoflex_amd import mitofilter as mf
    for kw, word in (({"min_insert": 0, "max_insert": 10}, "insert"), ({"min_insert": 11, "max_insert": 10}, "insert"),
                     ({"min_insert": 1, "max_insert": 4097}, "insert"), ({"min_insert": 1, "max_insert": 10, "rescue_permille": 1001}, "rescue_permille"),
                     ({"min_insert": 1, "max_insert": 10, "max_permille": 1001}, "max_permille"), ({"min_insert": 1, "max_insert": 10, "min_depth": 0}, "min_depth")):
        with pytest.raises(ValueError, match=word):
            mf.place_pairs(None, None, None, **kw)
