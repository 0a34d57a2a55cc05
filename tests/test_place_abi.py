"""The placement entry points of the C ABI without a GPU: the symbols load and are exported, the record types have the stated layout, NULL
handles are refused with MF_E_ARG before any device is touched, `fastfilter bait --place-report / --base-depth` exits non-zero without a
device and 1 when combined with another report (before the library is loaded), and mitofilter.pair_inserts joins hand-made placements
by the rules of bim.estimate_insert_sizes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
NEW = ("mf_place", "mf_filter_fastq_files_placed")
MF_E_ARG = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def test_new_symbols_load_and_are_exported(lib):
    from mitoflex_amd import mitofilter
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in mitofilter.EXPORTS
    assert callable(mitofilter.place_reads) and callable(mitofilter.filter_fastq_files_placed) and callable(mitofilter.pair_inserts)
    assert mitofilter.PLACE_AMBIGUOUS == 0xFFFFFFFE and mitofilter.PLACE_NONE == 0xFFFFFFFF
    assert mitofilter.PLACE.names == ("record", "strand", "start", "end", "votes", "windows")
    assert mitofilter.PLACE.itemsize == 24
    assert mitofilter.PLACE["start"] == np.int32 and mitofilter.PLACE["end"] == np.int32 and mitofilter.PLACE["record"] == np.uint32
    assert mitofilter.PLACE_RECORD.names == ("forward", "reverse", "over_begin", "over_end", "covered", "base_sum")
    assert mitofilter.PLACE_RECORD.itemsize == 48
    assert lib.mf_abi_version() == 5


def test_null_handles_are_refused(lib):
    bits = (C.c_uint32 * 2)(9, 9)
    place = (C.c_uint32 * 12)(*([4] * 12))
    depth = (C.c_uint32 * 4)(5, 5, 5, 5)
    recs = (C.c_uint64 * 12)(*([3] * 12))
    unplaced = (C.c_uint64 * 2)(6, 6)
    assert lib.mf_place(None, None, 1, 0, bits, place, depth, recs, unplaced, None) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()
    kept, total = C.c_uint64(11), C.c_uint64(12)
    dev = (C.c_int * 1)(0)
    assert lib.mf_filter_fastq_files_placed(None, b"a.fq", None, b"o.fq", None, 1, 0, dev, 1, depth, recs, unplaced, C.byref(kept),
                                            C.byref(total)) == MF_E_ARG
    assert b"NULL" in lib.mf_last_error()
    assert list(bits) == [9, 9] and list(place) == [4] * 12 and list(depth) == [5] * 4 and list(recs) == [3] * 12
    assert list(unplaced) == [6, 6] and (kept.value, total.value) == (11, 12)


def _inputs(tmp_path):
    from tests.util_data import make_bait, write_fastq
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(make_bait())
    fq = str(tmp_path / "a.fq")
    write_fastq(fq, ["ACGT" * 30] * 5, "a")
    return bait, fq


def test_cli_place_report_without_a_device(built_lib, tmp_path):
    bait, fq = _inputs(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for extra in (["--place-report", str(tmp_path / "d.tsv")], ["--base-depth", str(tmp_path / "p.tsv")],
                  ["--place-report", str(tmp_path / "d.tsv"), "--base-depth", str(tmp_path / "p.tsv")]):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq")] + extra, capture_output=True,
                           env=env, timeout=120)
        assert p.returncode != 0 and p.stdout == b"", p.stderr


@pytest.mark.parametrize("extra", [
    ["--place-report", "d.tsv", "--report", "r.tsv"],
    ["--place-report", "d.tsv", "--group-report", "g.tsv"],
    ["--place-report", "d.tsv", "--depth-report", "k.tsv"],
    ["--place-report", "d.tsv", "--depth-profile", "k.tsv"],
    ["--place-report", "d.tsv", "--protein"],
    ["--base-depth", "p.tsv", "--report", "r.tsv"],
    ["--base-depth", "p.tsv", "--group-report", "g.tsv", "--group-field", "4"],
    ["--base-depth", "p.tsv", "--depth-report", "k.tsv"],
    ["--base-depth", "p.tsv", "--depth-profile", "k.tsv"],
    ["--protein", "--base-depth", "p.tsv"],
    ["--place-report"],                                                     # no value
    ["--base-depth"],
])
def test_cli_place_conflicts_exit_before_loading(built_lib, tmp_path, extra):
    bait, fq = _inputs(tmp_path)
    extra = [str(tmp_path / a) if a.endswith(".tsv") else a for a in extra]
    p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                       + extra, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"", p.stderr          # (a library that cannot be loaded exits 2)
    assert not os.path.exists(str(tmp_path / "o.fq"))
    assert not any(n.endswith(".tsv") for n in os.listdir(str(tmp_path)))


def test_cli_place_flags_reach_the_library(built_lib, tmp_path):
    """well-formed placement arguments, either flag alone, get as far as loading the library (exit 2 on a missing one)"""
    bait, fq = _inputs(tmp_path)
    for extra in (["--place-report", str(tmp_path / "d.tsv")], ["--base-depth", str(tmp_path / "p.tsv")],
                  ["--place-report", str(tmp_path / "d.tsv"), "--base-depth", str(tmp_path / "p.tsv")]):
        p = subprocess.run([CLI, "bait", "--bait", bait, "--fq1", fq, "--out1", str(tmp_path / "o.fq"), "--lib", str(tmp_path / "no_such_library.so")]
                           + extra, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"no_such_library" in p.stderr


def _place(rows):
    from mitoflex_amd import mitofilter
    a = np.zeros(len(rows), dtype=mitofilter.PLACE)
    for i, (record, strand, start, end) in enumerate(rows):
        a[i] = (record, strand, start, end, 5, 5)
    return a


def test_pair_inserts_on_hand_made_placements():
    from mitoflex_amd import mitofilter as mf
    A, N = mf.PLACE_AMBIGUOUS, mf.PLACE_NONE
    cases = [                                                    # (mate 1, mate 2, insert size)
        ((0, 0, 100, 250), (0, 1, 300, 450), 350),               # forward mate is mate 1
        ((0, 1, 300, 450), (0, 0, 100, 250), 350),               # forward mate is mate 2
        ((2, 0, -20, 130), (2, 1, 200, 350), 370),               # a forward mate that hangs over the record's begin
        ((0, 0, 100, 250), (0, 0, 300, 450), -1),                # same strand
        ((0, 1, 100, 250), (0, 1, 300, 450), -1),
        ((0, 0, 100, 250), (1, 1, 300, 450), -1),                # different records
        ((0, 0, 100, 250), (A, 0, 0, 0), -1),                    # an ambiguous mate
        ((A, 0, 0, 0), (A, 0, 0, 0), -1),
        ((N, 0, 0, 0), (0, 1, 300, 450), -1),                    # a mate that did not pass
        ((N, 0, 0, 0), (N, 0, 0, 0), -1),
        ((0, 0, 450, 600), (0, 1, 300, 450), -1),                # size 0
        ((0, 0, 500, 650), (0, 1, 300, 450), -1),                # negative
        ((0, 0, 0, 150), (0, 1, 99850, 100000), 100000),         # the largest size kept
        ((0, 0, 0, 150), (0, 1, 99851, 100001), -1),             # size > 100 000
        ((0, 0, 449, 599), (0, 1, 300, 450), 1),
    ]
    got = mf.pair_inserts(_place([c[0] for c in cases]), _place([c[1] for c in cases]))
    assert got.dtype == np.int64
    assert got.tolist() == [c[2] for c in cases]
    assert mf.pair_inserts(_place([]), _place([])).tolist() == []
    with pytest.raises(ValueError):
        mf.pair_inserts(_place([(0, 0, 1, 2)]), _place([]))


def test_bim_anchors_argument_is_checked():
    from mitoflex_amd.bim import bim
    assert callable(bim.estimate_insert_sizes_device)
    with pytest.raises(ValueError):
        bim.kmer_bait_map(1, "bait.fa", ".", "p", "a.fq", "b.fq", anchors="nowhere")
