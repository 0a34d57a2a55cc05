"""ctypes binding of libmitofilter_hip.so (include/mitofilter.h).

Host code stays Python behind this thin shim, as BASELINE.json's north_star
asks; there is no PyTorch and no CPU fallback here: if the shared library is
missing, or no gfx950 device is visible, calls raise `MitoFilterError`.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmitofilter_hip.so")

KIND_NUCLEOTIDE, KIND_PROTEIN = 0, 1
MODE_SCREENED = 0
MODE_EXHAUSTIVE = 1
PAIR_EITHER = 0
PAIR_BOTH = 1
# which mates a verifying call writes (include/mitofilter.h, the keep rule): every passing one, those the cut does not reject, or only
# those that are placed and accepted
KEEP_PASSING, KEEP_ACCEPTED, KEEP_PLACED = 0, 1, 2
# record assignment of a read that passes but that no record wins / of a read that does not pass (mf_assign)
ASSIGN_AMBIGUOUS = 0xFFFFFFFE
ASSIGN_NONE = 0xFFFFFFFF
# profile entry of a position where no valid window starts (mf_depth)
DEPTH_NONE = 0xFFFFFFFF
# per-record k-mer depth summary (mf_depth_record_t)
DEPTH_RECORD = np.dtype([("windows", np.uint64), ("covered", np.uint64), ("depth_sum", np.uint64), ("depth_max", np.uint64)])
# placement of a read that passes but that no candidate wins / of a read that does not pass (mf_place)
PLACE_AMBIGUOUS = 0xFFFFFFFE
PLACE_NONE = 0xFFFFFFFF
# per-read placement (mf_place_t) and per-record placement summary (mf_place_record_t)
PLACE = np.dtype([("record", np.uint32), ("strand", np.uint32), ("start", np.int32), ("end", np.int32), ("votes", np.uint32),
                  ("windows", np.uint32)])
PLACE_RECORD = np.dtype([("forward", np.uint64), ("reverse", np.uint64), ("over_begin", np.uint64), ("over_end", np.uint64),
                         ("covered", np.uint64), ("base_sum", np.uint64)])
# per-position base counts (mf_pileup_t) and per-record pile-up summary (mf_pileup_record_t)
PILEUP = np.dtype([("a", np.uint32), ("c", np.uint32), ("g", np.uint32), ("t", np.uint32)])
PILEUP_RECORD = np.dtype([("bases", np.uint64), ("matches", np.uint64), ("mismatches", np.uint64), ("called", np.uint64),
                          ("ambiguous", np.uint64), ("variants", np.uint64)])
# per-read score of a placed read against the bait (mf_score_t) and per-record summary of the scores and the cut (mf_score_record_t)
SCORE_BINS = 32
SCORE = np.dtype([("compared", np.uint32), ("mismatches", np.uint32)])
SCORE_RECORD = np.dtype([("accepted", np.uint64), ("rejected", np.uint64), ("compared", np.uint64), ("mismatches", np.uint64),
                         ("hist", np.uint64, (SCORE_BINS,))])
# banded alignment of a placed read (mf_align_t), the indel counters of a bait position (mf_indel_t), the per-record summary
# (mf_align_record_t), and an indel position (indel_variants): pos is 0-based inside the record
ALIGN_MAX_BAND = 31
ALIGN = np.dtype([("compared", np.uint32), ("mismatches", np.uint32), ("insertions", np.uint32), ("deletions", np.uint32),
                  ("ref_begin", np.int32), ("ref_end", np.int32)])
INDEL = np.dtype([("del", np.uint32), ("ins", np.uint32), ("ins_bases", np.uint32)])
ALIGN_RECORD = np.dtype([("accepted", np.uint64), ("rejected", np.uint64), ("compared", np.uint64), ("mismatches", np.uint64),
                         ("insertions", np.uint64), ("deletions", np.uint64), ("gapped", np.uint64), ("hist", np.uint64, (SCORE_BINS,))])
# the per-record summary of the gapped consensus (mf_gapped_record_t)
GAPPED_RECORD = np.dtype([("length", np.uint64), ("deleted", np.uint64), ("insertions", np.uint64), ("inserted_bases", np.uint64)])
# the per-record summary of the extended records (mf_extend_record_t); EXTEND_MAX: the most columns an end grows by in one call
EXTEND_RECORD = np.dtype([("length", np.uint64), ("begin_bases", np.uint64), ("end_bases", np.uint64), ("begin_piled", np.uint64),
                          ("end_piled", np.uint64)])
EXTEND_MAX = 4096
INDEL_VARIANT = np.dtype([("record", np.uint32), ("pos", np.uint64), ("depth", np.uint64), ("del", np.uint64), ("ins", np.uint64),
                          ("ins_bases", np.uint64)])
# a variant position (pileup_variants): pos is 0-based inside the record, ref / alt are letters
VARIANT = np.dtype([("record", np.uint32), ("pos", np.uint64), ("ref", "S1"), ("alt", "S1"), ("depth", np.uint64), ("alt_count", np.uint64)])
# the largest insert size pair_inserts keeps (bim.estimate_insert_sizes' rule)
MAX_INSERT = 100000
# pair-aware placement (include/mitofilter.h, pairs): the most inserts a rescue window holds, the kinds of a pair, a pair, a record's pairs
RESCUE_MAX = 4096
PAIR_NONE, PAIR_PROPER, PAIR_DISCORDANT, PAIR_RESCUED_1, PAIR_RESCUED_2, PAIR_SINGLE_1, PAIR_SINGLE_2 = range(7)
PAIR = np.dtype([("kind", np.uint32), ("insert", np.int32)])
PAIR_RECORD = np.dtype([("proper", np.uint64), ("discordant", np.uint64), ("cross", np.uint64), ("rescued", np.uint64), ("single", np.uint64),
                        ("insert_sum", np.uint64)])

# every symbol include/mitofilter.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "mf_abi_version", "mf_last_error", "mf_device_count", "mf_device_name", "mf_device_synchronize",
    "mf_kmerset_build_from_fasta", "mf_kmerset_build_from_text", "mf_kmerset_build_protein_from_fasta",
    "mf_kmerset_build_protein_from_text", "mf_kmerset_info", "mf_kmerset_export",
    "mf_kmerset_free", "mf_reads_from_packed", "mf_reads_from_fastq", "mf_reads_synth", "mf_reads_synth_ex", "mf_free_host",
    "mf_reads_info", "mf_reads_free", "mf_filter", "mf_filter_resident", "mf_filter_resident_passes", "mf_filter_resident_bits", "mf_filter_packed",
    "mf_filter_fastq_files", "mf_filter_fastq_files_on", "mf_last_ingest_stats", "mf_h2d_bandwidth", "mf_set_option", "mf_qualfilter_files", "mf_release_cached",
    "mf_kmerset_record_count", "mf_kmerset_record_name", "mf_assign", "mf_filter_fastq_files_by_record",
    "mf_kmerset_group_records", "mf_kmerset_group_count", "mf_kmerset_group_name", "mf_assign_groups", "mf_filter_fastq_files_by_group",
    "mf_kmerset_record_starts", "mf_depth", "mf_filter_fastq_files_depth",
    "mf_place", "mf_filter_fastq_files_placed",
    "mf_pileup", "mf_filter_fastq_files_pileup", "mf_kmerset_bait_letters",
    "mf_verify", "mf_filter_fastq_files_verified",
    "mf_verify_keep", "mf_filter_fastq_files_verified_keep",
    "mf_align", "mf_filter_fastq_files_aligned",
    "mf_align_gapped", "mf_filter_fastq_files_gapped",
    "mf_align_extended", "mf_filter_fastq_files_extended",
    "mf_place_pairs",
    "mf_align_pairs",
)


class MitoFilterError(RuntimeError):
    pass


class KmerSetInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("key_words", C.c_int32), ("slots", C.c_uint64), ("n_keys", C.c_uint64),
                ("n_windows", C.c_uint64), ("screen_s", C.c_int32), ("screen_stride", C.c_int32),
                ("bloom_words", C.c_uint32), ("smer_slots", C.c_uint32), ("n_smers", C.c_uint64),
                ("kind", C.c_int32), ("genetic_code", C.c_int32),
                ("front_mode", C.c_uint32), ("front2_log2_blocks", C.c_uint32), ("front3_log2_blocks", C.c_uint32), ("canonical_screen", C.c_uint32)]


class ReadsInfo(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("total_bases", C.c_uint64), ("n_invalid", C.c_uint64),
                ("uniform_len", C.c_uint32), ("device", C.c_int32)]


class FilterStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_pass", C.c_uint64), ("n_candidates", C.c_uint64),
                ("ms_total", C.c_float), ("ms_screen", C.c_float), ("ms_mark", C.c_float), ("ms_exact", C.c_float),
                ("algorithmic_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class IngestStats(C.Structure):
    _fields_ = [("path", C.c_int32), ("n_devices", C.c_int32), ("consumers", C.c_int32), ("reserved", C.c_int32),
                ("input_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("records", C.c_uint64),
                ("seconds", C.c_double), ("decode_busy_seconds", C.c_double),
                ("pool_bytes_peak", C.c_uint64), ("device_bytes_peak", C.c_uint64),
                ("chunks", C.c_uint64), ("chunks_linked", C.c_uint64), ("gaps", C.c_uint64), ("gap_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


_lib = None


def load(path: Optional[str] = None):
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("MITOFILTER_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise MitoFilterError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
    L = C.CDLL(path)
    vp, u32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.mf_abi_version.restype = C.c_int
    L.mf_last_error.restype = C.c_char_p
    L.mf_device_count.restype = C.c_int
    L.mf_device_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.mf_device_synchronize.argtypes = [C.c_int]
    L.mf_kmerset_build_from_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.mf_kmerset_build_from_text.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
    L.mf_kmerset_build_protein_from_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.mf_kmerset_build_protein_from_text.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.mf_kmerset_info.argtypes = [vp, C.POINTER(KmerSetInfo)]
    L.mf_kmerset_export.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.mf_kmerset_free.argtypes = [vp]
    L.mf_reads_from_packed.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.mf_reads_from_fastq.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mf_reads_synth.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp),
                                 C.POINTER(u32p), u64p, C.POINTER(u64p), u64p]
    L.mf_reads_synth_ex.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp),
                                    C.POINTER(u32p), u64p, C.POINTER(u64p), u64p]
    L.mf_free_host.argtypes = [vp]
    L.mf_free_host.restype = None
    L.mf_reads_info.argtypes = [vp, C.POINTER(ReadsInfo)]
    L.mf_reads_free.argtypes = [vp]
    L.mf_filter.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_resident.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, C.POINTER(FilterStats)]
    L.mf_filter_resident_passes.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, vp, C.POINTER(FilterStats)]
    L.mf_filter_resident_bits.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_packed.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp]
    L.mf_filter_fastq_files.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                        C.c_int, u64p, u64p]
    L.mf_filter_fastq_files_on.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                           C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mf_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.mf_last_ingest_stats.argtypes = [C.POINTER(IngestStats)]
    L.mf_h2d_bandwidth.argtypes = [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.mf_release_cached.argtypes = [u64p]
    L.mf_qualfilter_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                      C.c_uint32, C.c_float, C.c_int, C.c_uint64, C.c_int, C.c_int, u64p, u64p,
                                      C.POINTER(C.c_int)]
    L.mf_kmerset_record_count.argtypes = [vp, u64p]
    L.mf_kmerset_record_name.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mf_assign.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_by_record.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                  C.POINTER(C.c_int), C.c_int, vp, u64p, u64p]
    L.mf_kmerset_group_records.argtypes = [vp, C.c_char_p, C.c_int]
    L.mf_kmerset_group_count.argtypes = [vp, u64p]
    L.mf_kmerset_group_name.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mf_assign_groups.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_by_group.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                 C.POINTER(C.c_int), C.c_int, vp, u64p, u64p]
    L.mf_kmerset_record_starts.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mf_depth.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_depth.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                              C.POINTER(C.c_int), C.c_int, vp, vp, u64p, u64p]
    L.mf_place.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_placed.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                               C.POINTER(C.c_int), C.c_int, vp, vp, vp, u64p, u64p]
    L.mf_pileup.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_pileup.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                               C.POINTER(C.c_int), C.c_int, C.c_uint32, vp, vp, vp, vp, u64p, u64p]
    L.mf_kmerset_bait_letters.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mf_verify.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_verified.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                 C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, u64p, u64p]
    L.mf_verify_keep.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                 C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_verified_keep.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                      C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                      u64p, u64p]
    L.mf_align.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                           C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_aligned.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                                vp, vp, u64p, u64p]
    L.mf_align_gapped.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, vp, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_gapped.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                               C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                               vp, vp, vp, vp, vp, vp, u64p, u64p]
    L.mf_align_extended.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(FilterStats)]
    L.mf_filter_fastq_files_extended.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int,
                                                 C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp,
                                                 vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64p, u64p]
    L.mf_place_pairs.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                 vp, vp, vp, vp, vp, vp, vp, vp, u64p, vp, C.POINTER(FilterStats)]
    L.mf_align_pairs.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                                 *([vp] * 23), u64p, vp, C.POINTER(FilterStats)]
    if L.mf_abi_version() != 5:
        raise MitoFilterError("libmitofilter_hip ABI version mismatch")
    _lib = L
    return L


def _chk(rc: int):
    if rc != 0:
        raise MitoFilterError(f"libmitofilter_hip error {rc}: {load().mf_last_error().decode(errors='replace')}")


def device_count() -> int:
    n = load().mf_device_count()
    if n < 0:
        _chk(n)
    return n


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    _chk(load().mf_device_name(device, buf, 256))
    return buf.value.decode()


def device_synchronize(device: int = 0):
    _chk(load().mf_device_synchronize(device))


def _enc(p):
    return None if p is None else os.fsencode(p)


class KmerSet:
    """Bait canonical-k-mer set resident on the GPU (rows B3/B5)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_fasta(cls, path: str, k: int = 31, device: int = 0) -> "KmerSet":
        h = C.c_void_p()
        _chk(load().mf_kmerset_build_from_fasta(_enc(path), k, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_text(cls, fasta_text, k: int = 31, device: int = 0) -> "KmerSet":
        if isinstance(fasta_text, str):
            fasta_text = fasta_text.encode()
        h = C.c_void_p()
        _chk(load().mf_kmerset_build_from_text(fasta_text, len(fasta_text), k, device, C.byref(h)))
        return cls(h)

    @classmethod
    def protein_from_fasta(cls, path: str, kp: int = 9, genetic_code: int = 5, device: int = 0) -> "KmerSet":
        """Peptide k-mer set of a protein FASTA (e.g. the reference's profile/MT_database/<clade>.fa); reads
        filtered against it are translated in six frames with NCBI table `genetic_code`."""
        h = C.c_void_p()
        _chk(load().mf_kmerset_build_protein_from_fasta(_enc(path), kp, genetic_code, device, C.byref(h)))
        return cls(h)

    @classmethod
    def protein_from_text(cls, fasta_text, kp: int = 9, genetic_code: int = 5, device: int = 0) -> "KmerSet":
        if isinstance(fasta_text, str):
            fasta_text = fasta_text.encode()
        h = C.c_void_p()
        _chk(load().mf_kmerset_build_protein_from_text(fasta_text, len(fasta_text), kp, genetic_code, device, C.byref(h)))
        return cls(h)

    @property
    def info(self) -> KmerSetInfo:
        i = KmerSetInfo()
        _chk(load().mf_kmerset_info(self._h, C.byref(i)))
        return i

    @property
    def record_names(self) -> list:
        """Names of the bait's records in FASTA order (header text up to the first space, tab or CR; "" for sequence before any header)."""
        L = load()
        n = C.c_uint64()
        _chk(L.mf_kmerset_record_count(self._h, C.byref(n)))
        names = []
        for i in range(n.value):
            need = C.c_size_t()
            L.mf_kmerset_record_name(self._h, i, None, 0, C.byref(need))
            buf = C.create_string_buffer(max(need.value, 1))
            _chk(L.mf_kmerset_record_name(self._h, i, buf, len(buf), None))
            names.append(buf.value.decode(errors="replace"))
        return names

    def group_records(self, sep: Optional[str] = "_", field: int = 4) -> None:
        """Group the records by the `field`-th `sep`-separated token of their names (from 1; a name with fewer fields is its own
        group); sep None or field 0: each record its own group (the default).  Protein and nucleotide sets alike.  Must not run
        while another call uses the set."""
        _chk(load().mf_kmerset_group_records(self._h, None if sep is None else sep.encode(), int(field)))

    @property
    def group_names(self) -> list:
        """Names of the groups, numbered in order of first appearance (the record names under the identity grouping)."""
        L = load()
        n = C.c_uint64()
        _chk(L.mf_kmerset_group_count(self._h, C.byref(n)))
        names = []
        for i in range(n.value):
            need = C.c_size_t()
            L.mf_kmerset_group_name(self._h, i, None, 0, C.byref(need))
            buf = C.create_string_buffer(max(need.value, 1))
            _chk(L.mf_kmerset_group_name(self._h, i, buf, len(buf), None))
            names.append(buf.value.decode(errors="replace"))
        return names

    @property
    def record_starts(self) -> np.ndarray:
        """u64[R + 1]: record j holds positions (bases, or residues of a protein set) starts[j] .. starts[j + 1] - 1."""
        L = load()
        need = C.c_size_t()
        L.mf_kmerset_record_starts(self._h, None, 0, C.byref(need))
        out = np.zeros(max(need.value, 1), dtype=np.uint64)
        _chk(L.mf_kmerset_record_starts(self._h, out.ctypes.data, out.size, None))
        return out

    @property
    def bait_letters(self) -> np.ndarray:
        """u8[positions]: the bait's letter at every position of a nucleotide set, one of A C G T, N for an invalid one."""
        L = load()
        need = C.c_size_t()
        L.mf_kmerset_bait_letters(self._h, None, 0, C.byref(need))
        out = np.zeros(max(need.value, 1), dtype=np.uint8)
        _chk(L.mf_kmerset_bait_letters(self._h, out.ctypes.data, out.size, None))
        return out[:need.value]

    def export_table(self, device: int = 0) -> np.ndarray:
        i = self.info
        out = np.empty(i.slots * i.key_words, dtype=np.uint64)
        _chk(load().mf_kmerset_export(self._h, device, out.ctypes.data, out.size))
        return out

    def close(self):
        if self._h:
            load().mf_kmerset_free(self._h)
            self._h = None

    __del__ = close


class Reads:
    """One packed read set resident in one GPU's HBM (row B1)."""

    def __init__(self, handle):
        self._h = handle
        self.host_words: Optional[np.ndarray] = None
        self.host_npos: Optional[np.ndarray] = None

    @classmethod
    def from_packed(cls, words: np.ndarray, offsets: np.ndarray, npos: np.ndarray, device: int = 0) -> "Reads":
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npos = np.ascontiguousarray(npos, dtype=np.uint64)
        h = C.c_void_p()
        _chk(load().mf_reads_from_packed(words.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                         npos.ctypes.data if npos.size else None, npos.size, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_fastq(cls, path: str, device: int = 0) -> "Reads":
        h = C.c_void_p()
        _chk(load().mf_reads_from_fastq(_enc(path), device, C.byref(h)))
        return cls(h)

    @classmethod
    def synth(cls, n_reads: int, read_len: int, seed: int, bait_text, mito_ppm=5000, sub_ppm=10000,
              n_read_ppm=10000, n_base_ppm=1000, device: int = 0, keep_host: bool = False,
              msat_ppm: int = 0, numt_ppm: int = 0, numt_div_ppm: int = 150000) -> "Reads":
        if isinstance(bait_text, str):
            bait_text = bait_text.encode()
        h = C.c_void_p()
        L = load()
        if keep_host:
            wp, np_ = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
            nw, nn = C.c_uint64(), C.c_uint64()
            _chk(L.mf_reads_synth_ex(n_reads, read_len, seed, bait_text, len(bait_text), mito_ppm, sub_ppm, n_read_ppm,
                                     n_base_ppm, msat_ppm, numt_ppm, numt_div_ppm, device, C.byref(h), C.byref(wp), C.byref(nw), C.byref(np_), C.byref(nn)))
            self = cls(h)
            self.host_words = np.ctypeslib.as_array(wp, shape=(nw.value + 8,)).copy()
            self.host_npos = (np.ctypeslib.as_array(np_, shape=(nn.value,)).copy() if nn.value
                              else np.zeros(0, np.uint64))
            L.mf_free_host(wp)
            L.mf_free_host(np_)
            return self
        _chk(L.mf_reads_synth_ex(n_reads, read_len, seed, bait_text, len(bait_text), mito_ppm, sub_ppm, n_read_ppm,
                                 n_base_ppm, msat_ppm, numt_ppm, numt_div_ppm, device, C.byref(h), None, None, None, None))
        return cls(h)

    @property
    def info(self) -> ReadsInfo:
        i = ReadsInfo()
        _chk(load().mf_reads_info(self._h, C.byref(i)))
        return i

    def close(self):
        if self._h:
            load().mf_reads_free(self._h)
            self._h = None

    __del__ = close


def filter_reads(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED,
                 want_hits: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray], FilterStats]:
    """Run the hot path once.  -> (bits u32[ceil(n/32)], hits u32[n] | None, stats)."""
    n = reads.info.n_reads
    bits = np.zeros((n + 31) // 32, dtype=np.uint32)
    hits = np.zeros(max(n, 1), dtype=np.uint32) if want_hits else None
    st = FilterStats()
    _chk(load().mf_filter(ks._h, reads._h, threshold, mode, bits.ctypes.data,
                          hits.ctypes.data if want_hits else None, C.byref(st)))
    return bits, (hits[:n] if want_hits else None), st


def _n_records(ks: KmerSet) -> int:
    n = C.c_uint64()
    _chk(load().mf_kmerset_record_count(ks._h, C.byref(n)))
    return n.value


def assign_reads(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED):
    """One filter pass, then the bait record of every passing read.  -> (bits u32[ceil(n/32)], assign u32[n], counts u64[R + 2]):
    assign holds a record index, ASSIGN_AMBIGUOUS or ASSIGN_NONE; counts are the reads of each record, then ambiguous, then unassigned."""
    n = reads.info.n_reads
    R = _n_records(ks)
    bits = np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)
    assign = np.full(max(n, 1), ASSIGN_NONE, dtype=np.uint32)
    counts = np.zeros(R + 2, dtype=np.uint64)
    _chk(load().mf_assign(ks._h, reads._h, threshold, mode, bits.ctypes.data, assign.ctypes.data, counts.ctypes.data, None))
    return bits[:(n + 31) // 32], assign[:n], counts


def _n_groups(ks: KmerSet) -> int:
    n = C.c_uint64()
    _chk(load().mf_kmerset_group_count(ks._h, C.byref(n)))
    return n.value


def assign_groups(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED):
    """assign_reads by group of records (KmerSet.group_records), for protein sets too.  -> (bits u32[ceil(n/32)], assign u32[n],
    counts u64[G + 2]): assign holds a group index, ASSIGN_AMBIGUOUS or ASSIGN_NONE; counts are the reads of each group, then
    ambiguous, then unassigned."""
    n = reads.info.n_reads
    G = _n_groups(ks)
    bits = np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)
    assign = np.full(max(n, 1), ASSIGN_NONE, dtype=np.uint32)
    counts = np.zeros(G + 2, dtype=np.uint64)
    _chk(load().mf_assign_groups(ks._h, reads._h, threshold, mode, bits.ctypes.data, assign.ctypes.data, counts.ctypes.data, None))
    return bits[:(n + 31) // 32], assign[:n], counts


def record_depth(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED):
    """One filter pass, then the k-mer depth of the bait positions (include/mitofilter.h: mf_depth).  -> (bits u32[ceil(n/32)],
    profile u32[positions]: depth of the valid window starting at each position, DEPTH_NONE where none does, records: DEPTH_RECORD[R]
    with the fields windows, covered, depth_sum, depth_max)."""
    n = reads.info.n_reads
    starts = ks.record_starts
    bits = np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)
    profile = np.zeros(max(int(starts[-1]), 1), dtype=np.uint32)
    records = np.zeros(max(len(starts) - 1, 1), dtype=DEPTH_RECORD)
    _chk(load().mf_depth(ks._h, reads._h, threshold, mode, bits.ctypes.data, profile.ctypes.data, records.ctypes.data, None))
    return bits[:(n + 31) // 32], profile[:int(starts[-1])], records[:len(starts) - 1]


def _read_outputs(reads: Reads, *dtypes):
    """the pass bitmap of a resident call and, for each dtype, an array of one entry a read: their pointers in that order, and what
    gives them trimmed to the read set"""
    n = reads.info.n_reads
    a = [np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)] + [np.zeros(max(n, 1), dtype=d) for d in dtypes]
    return [x.ctypes.data for x in a], lambda: [a[0][:(n + 31) // 32]] + [x[:n] for x in a[1:]]


def _report_outputs(ks: KmerSet, fields, leave_out=()):
    """the per-position and per-record arrays `fields` (named as Verified names them, in the C order of the call) of a placement-family
    call: their pointers in that order (NULL for those in leave_out), and what gives {field: the array trimmed to the set, or None}"""
    starts = ks.record_starts
    P, R = int(starts[-1]), len(starts) - 1
    shape = {"base_depth": (P, np.uint32), "place_records": (R, PLACE_RECORD), "pileup": (P, PILEUP), "consensus": (P, np.uint8),
             "pileup_records": (R, PILEUP_RECORD), "score_records": (R, SCORE_RECORD), "unplaced": (2, np.uint64),
             "indels": (P, INDEL), "align_records": (R, ALIGN_RECORD)}
    a = {f: None if f in leave_out else np.zeros(max(shape[f][0], 1), dtype=shape[f][1]) for f in fields}
    ptrs = [x.ctypes.data if x is not None else None for x in a.values()]
    return ptrs, lambda: {f: (x[:shape[f][0]] if x is not None else None) for f, x in a.items()}


_PLACE_FIELDS = ("base_depth", "place_records", "unplaced")
_PILEUP_FIELDS = ("pileup", "consensus", "pileup_records", "unplaced")
_VERIFY_FIELDS = ("base_depth", "place_records", "pileup", "consensus", "pileup_records", "score_records", "unplaced")
_ALIGN_FIELDS = ("base_depth", "place_records", "pileup", "consensus", "pileup_records", "indels", "align_records", "unplaced")


def place_reads(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED):
    """One filter pass, then where every passing read lies on the bait (include/mitofilter.h: mf_place).  -> (bits u32[ceil(n/32)],
    place PLACE[n]: record (or PLACE_AMBIGUOUS / PLACE_NONE), strand, start, end, votes, windows, base_depth u32[positions],
    records PLACE_RECORD[R], unplaced u64[2]: passing reads that are not placed, reads that do not pass)."""
    per_read, read_results = _read_outputs(reads, PLACE)
    ptrs, results = _report_outputs(ks, _PLACE_FIELDS)
    _chk(load().mf_place(ks._h, reads._h, threshold, mode, *per_read, *ptrs, None))
    return (*read_results(), *results().values())


def pileup_reads(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED, min_depth: int = 1):
    """One filter pass, then the placed reads' bases piled on the bait (include/mitofilter.h: mf_pileup).  -> (bits u32[ceil(n/32)],
    pileup PILEUP[positions]: bases a, c, g, t in the bait's forward letters, consensus u8[positions]: the called letter in upper case,
    N where the most is tied, the bait's letter in lower case below min_depth, records PILEUP_RECORD[R], unplaced u64[2] as place_reads)."""
    per_read, read_results = _read_outputs(reads)
    ptrs, results = _report_outputs(ks, _PILEUP_FIELDS)
    _chk(load().mf_pileup(ks._h, reads._h, threshold, mode, min_depth, *per_read, *ptrs, None))
    return (*read_results(), *results().values())


class Verified:
    """What a verifying call gives (include/mitofilter.h, verification).  verify_reads fills bits, place PLACE[n] and score SCORE[n];
    filter_fastq_files_verified fills kept and total; the fields a call does not fill are None.  Both give base_depth u32[positions],
    place_records PLACE_RECORD[R], score_records SCORE_RECORD[R], unplaced u64[2] and, unless the call ran with pileup=False (then
    None), pileup PILEUP[positions], consensus u8[positions] and pileup_records PILEUP_RECORD[R].  keep_bits is None here: verify_reads
    with a keep mode other than KEEP_PASSING gives a VerifiedKeep, which holds them."""
    __slots__ = ("bits", "kept", "total", "place", "score", "base_depth", "place_records", "pileup", "consensus", "pileup_records",
                 "score_records", "unplaced")

    keep_bits = None          # (no slot: a call without a keep mode returns the object it always returned)

    @classmethod
    def _names(cls):
        return [name for c in reversed(cls.__mro__) for name in getattr(c, "__slots__", ())]

    def __init__(self, **fields):
        for name in self._names():
            setattr(self, name, fields.pop(name, None))
        if fields:
            raise TypeError("unknown field(s): %s" % ", ".join(sorted(fields)))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join(name for name in self._names() if getattr(self, name) is not None))


class VerifiedKeep(Verified):
    """Verified plus the keep_bits slot: u32[ceil(n/32)], the pass bits amended by the keep rule (include/mitofilter.h, "which mates are
    written"), laid out like bits.  What verify_reads gives for keep = KEEP_ACCEPTED or KEEP_PLACED."""
    __slots__ = ("keep_bits",)


def _check_cut(min_depth: int, max_permille: int, keep: int = KEEP_PASSING):
    if not 0 <= int(max_permille) <= 1000:
        raise ValueError("max_permille is a number from 0 to 1000")
    if int(min_depth) < 1:
        raise ValueError("min_depth is at least 1")
    if int(keep) not in (KEEP_PASSING, KEEP_ACCEPTED, KEEP_PLACED):
        raise ValueError("keep is KEEP_PASSING, KEEP_ACCEPTED or KEEP_PLACED")


def verify_reads(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED, min_depth: int = 1, max_permille: int = 1000,
                 pileup: bool = True, keep: int = KEEP_PASSING) -> Verified:
    """One filter pass, then every placed read scored against the bait along its placement and cut at max_permille mismatches per
    thousand compared bases; what is accepted gives base depth and (pileup=True) the pile-up (include/mitofilter.h: mf_verify).
    keep = KEEP_ACCEPTED / KEEP_PLACED: keep_bits are the pass bits without the reads the keep rule does not write (mf_verify_keep);
    nothing else depends on it.  -> Verified (VerifiedKeep with a keep mode) with bits, place, score and the shared fields."""
    _check_cut(min_depth, max_permille, keep)
    per_read, read_results = _read_outputs(reads, PLACE, SCORE)
    ptrs, results = _report_outputs(ks, _VERIFY_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    if int(keep) == KEEP_PASSING:
        _chk(load().mf_verify(ks._h, reads._h, threshold, mode, min_depth, max_permille, *per_read, *ptrs, None))
        bits, place, score = read_results()
        return Verified(bits=bits, place=place, score=score, **results())
    n = reads.info.n_reads
    keep_bits = np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)
    _chk(load().mf_verify_keep(ks._h, reads._h, threshold, mode, min_depth, max_permille, int(keep), per_read[0], keep_bits.ctypes.data,
                               *per_read[1:], *ptrs, None))
    bits, place, score = read_results()
    return VerifiedKeep(bits=bits, keep_bits=keep_bits[:(n + 31) // 32], place=place, score=score, **results())


class Aligned(Verified):
    """What an aligning call gives (include/mitofilter.h, banded alignment): Verified's fields with score and score_records None, and
    align ALIGN[n] (align_reads only), indels INDEL[positions], align_records ALIGN_RECORD[R] and keep_bits u32[ceil(n/32)] (align_reads
    only; the pass bits under KEEP_PASSING).  A call with gapped=True (include/mitofilter.h, gapped consensus) also gives ins_pile
    PILEUP[positions, 2 * band], gapped u8[its length], gapped_starts u64[R + 1] and gapped_records GAPPED_RECORD[R]; None otherwise.
    A call with extend=E > 0 (include/mitofilter.h, extended records) also gives ext_pile PILEUP[R, 2, E] ([record, begin / end, offset
    from the record]), extended u8[its length], extended_starts u64[R + 1] and extend_records EXTEND_RECORD[R]; None otherwise."""
    __slots__ = ("keep_bits", "align", "indels", "align_records", "ins_pile", "gapped", "gapped_starts", "gapped_records",
                 "ext_pile", "extended", "extended_starts", "extend_records")


def _gapped_outputs(ks: KmerSet, band: int):
    """the four outputs of a gapped call: their pointers in the C order, and what gives them as Aligned names them"""
    starts = ks.record_starts
    P, R, span = int(starts[-1]), len(starts) - 1, 2 * int(band)
    ins = np.zeros((max(P, 1), max(span, 1)), dtype=PILEUP)
    gapped = np.zeros(max(P * (1 + span), 1), dtype=np.uint8)
    gstarts = np.zeros(R + 1, dtype=np.uint64)
    grec = np.zeros(max(R, 1), dtype=GAPPED_RECORD)
    ptrs = [ins.ctypes.data if span else None, gapped.ctypes.data, gstarts.ctypes.data, grec.ctypes.data]
    return ptrs, lambda: {"ins_pile": ins[:P, :span], "gapped": gapped[:int(gstarts[-1])], "gapped_starts": gstarts, "gapped_records": grec[:R]}


def _extend_outputs(ks: KmerSet, band: int, extend: int):
    """the four outputs of an extending call, as _gapped_outputs gives the gapped call's"""
    starts = ks.record_starts
    P, R, span, E = int(starts[-1]), len(starts) - 1, 2 * int(band), int(extend)
    ext = np.zeros((max(R, 1), 2, E), dtype=PILEUP)
    extended = np.zeros(max(P * (1 + span) + 2 * R * E, 1), dtype=np.uint8)
    xstarts = np.zeros(R + 1, dtype=np.uint64)
    xrec = np.zeros(max(R, 1), dtype=EXTEND_RECORD)
    ptrs = [ext.ctypes.data, extended.ctypes.data, xstarts.ctypes.data, xrec.ctypes.data]
    return ptrs, lambda: {"ext_pile": ext[:R], "extended": extended[:int(xstarts[-1])], "extended_starts": xstarts, "extend_records": xrec[:R]}


def _check_extend(extend: int):
    if not 0 <= int(extend) <= EXTEND_MAX:
        raise ValueError("extend is a number from 0 to %d" % EXTEND_MAX)


def _check_band(band: int):
    if not 0 <= int(band) <= ALIGN_MAX_BAND:
        raise ValueError("band is a number from 0 to %d (and below k)" % ALIGN_MAX_BAND)


def align_reads(ks: KmerSet, reads: Reads, band: int = 8, min_depth: int = 1, max_permille: int = 1000, keep: int = KEEP_PASSING,
                pileup: bool = True, threshold: int = 1, mode: int = MODE_SCREENED, extend: int = 0, gapped: bool = False) -> Aligned:
    """One filter pass, then every placed read aligned to its record inside the band of 2 * band + 1 diagonals around its placement and
    cut at max_permille edits per thousand alignment columns; base depth, the records, the keep bits and (pileup=True) the pile-up
    follow the alignment, and indels counts deletions and insertions per bait position (include/mitofilter.h: mf_align).  band = 0 is
    verify_reads.  gapped=True: the letters of the inserted bases and the consensus that calls deletions and insertions too
    (mf_align_gapped).  extend=E > 0: the bases that hang over the records' ends piled up to E columns from them, both ends called and
    the extended records (mf_align_extended); the gapped fields are filled only with gapped=True.  -> Aligned with bits, keep_bits, place,
    align and the shared fields."""
    _check_cut(min_depth, max_permille, keep)
    _check_band(band)
    _check_extend(extend)
    per_read, read_results = _read_outputs(reads, PLACE, ALIGN)
    ptrs, results = _report_outputs(ks, _ALIGN_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    n = reads.info.n_reads
    keep_bits = np.zeros(max((n + 31) // 32, 1), dtype=np.uint32)
    more = {}
    if int(extend) > 0:
        gptrs, gresults = _gapped_outputs(ks, band) if gapped else ([None] * 4, dict)
        xptrs, xresults = _extend_outputs(ks, band, extend)
        _chk(load().mf_align_extended(ks._h, reads._h, threshold, mode, min_depth, max_permille, int(keep), int(band), int(extend), per_read[0],
                                      keep_bits.ctypes.data, *per_read[1:], *ptrs[:-1], *gptrs, *xptrs, ptrs[-1], None))
        more = {**gresults(), **xresults()}
    elif gapped:
        gptrs, gresults = _gapped_outputs(ks, band)
        _chk(load().mf_align_gapped(ks._h, reads._h, threshold, mode, min_depth, max_permille, int(keep), int(band), per_read[0],
                                    keep_bits.ctypes.data, *per_read[1:], *ptrs[:-1], *gptrs, ptrs[-1], None))
        more = gresults()
    else:
        _chk(load().mf_align(ks._h, reads._h, threshold, mode, min_depth, max_permille, int(keep), int(band), per_read[0], keep_bits.ctypes.data,
                             *per_read[1:], *ptrs, None))
    bits, place, align = read_results()
    return Aligned(bits=bits, keep_bits=keep_bits[:(n + 31) // 32], place=place, align=align, **results(), **more)


def gapped_consensus(record_starts, base_depth, indels, ins_pile, consensus, min_depth: int = 1):
    """The call rule of the gapped consensus (include/mitofilter.h) over the downloaded outputs of an aligning call, valid where no
    counter is clamped: a position is deleted where more than half of its base depth deletes it (and the depth reaches min_depth, the
    call's), else it keeps its consensus byte; behind it the insertion columns that more than half of the depth carries, up to the first
    that fewer do, each the letter with strictly the most bases or N.  ins_pile: PILEUP[positions, span].
    -> (gapped u8, gapped_starts u64[R + 1], gapped_records GAPPED_RECORD[R]).  Needs no device."""
    if int(min_depth) < 1:
        raise ValueError("min_depth is at least 1")
    starts = np.asarray(record_starts, dtype=np.uint64)
    P, R = int(starts[-1]), len(starts) - 1
    depth = np.asarray(base_depth)[:P].astype(np.int64)
    cons = np.asarray(consensus, dtype=np.uint8)[:P]
    ins = np.asarray(ins_pile)
    if ins.dtype != PILEUP or ins.ndim != 2:
        raise ValueError("ins_pile is PILEUP[positions, span]")
    span = ins.shape[1]
    ins = ins[:P]
    dels = np.asarray(indels)[:P]["del"].astype(np.int64) if span else np.zeros(P, np.int64)
    if not (len(depth) == len(cons) == len(ins) == len(dels) == P):
        raise ValueError("base_depth, indels, ins_pile and consensus hold one entry per position")
    counts = np.stack([ins[f].astype(np.int64) for f in ("a", "c", "g", "t")], axis=2) if span else np.zeros((P, 0, 4), np.int64)
    deep = depth >= int(min_depth)
    deleted = deep & (2 * dels > depth)
    carried = deep[:, None] & (2 * counts.sum(axis=2) > depth[:, None])
    n_cols = np.minimum.accumulate(carried, axis=1).sum(axis=1) if span else np.zeros(P, np.int64)          # up to the first that is not
    most = counts.max(axis=2) if span else counts.sum(axis=2)
    alone = (counts == most[:, :, None]).sum(axis=2) == 1
    letters = np.where(alone, np.frombuffer(b"ACGT", np.uint8)[counts.argmax(axis=2)] if span else 0, ord("N")).astype(np.uint8)
    out, gstarts, rec = bytearray(), np.zeros(R + 1, np.uint64), np.zeros(R, dtype=GAPPED_RECORD)
    for j in range(R):
        gstarts[j] = len(out)
        for p in range(int(starts[j]), int(starts[j + 1])):
            if not deleted[p]:
                out.append(int(cons[p]))
            out += letters[p, :n_cols[p]].tobytes()
        lo, hi = int(starts[j]), int(starts[j + 1])
        rec[j] = (len(out) - int(gstarts[j]), int(deleted[lo:hi].sum()), int((n_cols[lo:hi] > 0).sum()), int(n_cols[lo:hi].sum()))
    gstarts[R] = len(out)
    return np.frombuffer(bytes(out), np.uint8), gstarts, rec


def extended_consensus(gapped, gapped_starts, ext_pile, min_depth: int = 1):
    """The call rule of the extended records (include/mitofilter.h) over the downloaded outputs of an extending call, valid where no
    counter is clamped: per record and end the columns from the record outwards that hold at least min_depth bases and one letter with
    strictly the most, up to the first that does not; the begin columns from the farthest, the record's gapped bytes, the end columns.
    ext_pile: PILEUP[R, 2, E].  -> (extended u8, extended_starts u64[R + 1], extend_records EXTEND_RECORD[R]).  Needs no device."""
    if int(min_depth) < 1:
        raise ValueError("min_depth is at least 1")
    gstarts = np.asarray(gapped_starts, dtype=np.uint64)
    R = len(gstarts) - 1
    ext = np.asarray(ext_pile)
    if ext.dtype != PILEUP or ext.ndim != 3 or ext.shape[:2] != (R, 2):
        raise ValueError("ext_pile is PILEUP[R, 2, E]")
    body = np.asarray(gapped, dtype=np.uint8)
    if len(body) < int(gstarts[-1]):
        raise ValueError("gapped is shorter than gapped_starts says")
    counts = np.stack([ext[f].astype(np.int64) for f in ("a", "c", "g", "t")], axis=3)          # [R, 2, E, 4]
    most = counts.max(axis=3)
    emit = (counts.sum(axis=3) >= int(min_depth)) & ((counts == most[..., None]).sum(axis=3) == 1)
    n_cols = np.minimum.accumulate(emit, axis=2).sum(axis=2)                                    # up to the first that is not
    letters = np.frombuffer(b"ACGT", np.uint8)[counts.argmax(axis=3)]
    out, xstarts, rec = bytearray(), np.zeros(R + 1, np.uint64), np.zeros(R, dtype=EXTEND_RECORD)
    for j in range(R):
        xstarts[j] = len(out)
        nb, ne = int(n_cols[j, 0]), int(n_cols[j, 1])
        out += letters[j, 0, :nb][::-1].tobytes()
        out += body[int(gstarts[j]):int(gstarts[j + 1])].tobytes()
        out += letters[j, 1, :ne].tobytes()
        rec[j] = (len(out) - int(xstarts[j]), nb, ne, int(counts[j, 0].sum()), int(counts[j, 1].sum()))
    xstarts[R] = len(out)
    return np.frombuffer(bytes(out), np.uint8), xstarts, rec


def indel_variants(record_starts, base_depth, indels, min_depth: int = 1, min_permille: int = 500) -> np.ndarray:
    """The indel positions of an aligning call: positions of at least min_depth base depth whose del or ins, per thousand of that depth,
    reaches min_permille.  -> INDEL_VARIANT[n]: record, pos (0-based inside the record; an insertion lies behind it), depth, del, ins,
    ins_bases.  Needs no device."""
    if int(min_depth) < 1:
        raise ValueError("min_depth is at least 1")
    if not 0 <= int(min_permille) <= 1000:
        raise ValueError("min_permille is a number from 0 to 1000")
    starts = np.asarray(record_starts, dtype=np.uint64)
    P = int(starts[-1])
    depth = np.asarray(base_depth)[:P].astype(np.uint64)
    indels = np.asarray(indels)[:P]
    if not (len(depth) == len(indels) == P):
        raise ValueError("base_depth and indels hold one entry per position")
    most = np.maximum(indels["del"], indels["ins"]).astype(np.uint64)
    at = np.nonzero((depth >= np.uint64(min_depth)) & (most > 0) & (most * np.uint64(1000) >= np.uint64(min_permille) * depth))[0]
    out = np.zeros(at.size, dtype=INDEL_VARIANT)
    rec = np.searchsorted(starts, at, side="right") - 1
    out["record"] = rec
    out["pos"] = at - starts[rec].astype(np.int64) if at.size else at
    out["depth"] = depth[at]
    for f in ("del", "ins", "ins_bases"):
        out[f] = indels[f][at]
    return out


def consensus_fasta(names, starts, consensus, width: int = 60) -> str:
    """FASTA text of a consensus (u8[positions] or bytes) under the records' names: lines of `width` letters; an empty record gives a
    header and no sequence line.  Needs no device."""
    if width < 1:
        raise ValueError("width is at least 1")
    if len(starts) != len(names) + 1:
        raise ValueError("starts has one more entry than names")
    text = bytes(bytearray(np.asarray(consensus, dtype=np.uint8))) if not isinstance(consensus, (bytes, bytearray)) else bytes(consensus)
    if len(text) < int(starts[-1]):
        raise ValueError("the consensus is shorter than the records")
    out = []
    for j, name in enumerate(names):
        out.append(">%s\n" % name)
        seq = text[int(starts[j]):int(starts[j + 1])].decode("ascii")
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out)


def pileup_variants(starts, letters, pileup, consensus) -> np.ndarray:
    """The variant positions of a pile-up: called positions (an upper-case A, C, G or T in `consensus`) whose bait letter (`letters`, as
    KmerSet.bait_letters) is valid and differs from the call.  -> VARIANT[n]: record, pos (0-based inside the record), ref, alt,
    depth = a + c + g + t, alt_count = the bases of the called letter.  Needs no device."""
    starts = np.asarray(starts, dtype=np.uint64)
    P = int(starts[-1])
    letters = np.frombuffer(bytes(letters), dtype=np.uint8)[:P] if isinstance(letters, (bytes, bytearray)) else np.asarray(letters, dtype=np.uint8)[:P]
    cons = np.frombuffer(bytes(consensus), dtype=np.uint8)[:P] if isinstance(consensus, (bytes, bytearray)) else np.asarray(consensus, dtype=np.uint8)[:P]
    pileup = np.asarray(pileup)[:P]
    if not (len(letters) == len(cons) == len(pileup) == P):
        raise ValueError("letters, pileup and consensus hold one entry per position")
    counts = np.stack([pileup[f].astype(np.uint64) for f in ("a", "c", "g", "t")], axis=1) if P else np.zeros((0, 4), np.uint64)
    code = np.full(256, 4, dtype=np.int64)
    code[list(b"ACGT")] = range(4)
    call, ref = code[cons], code[letters]
    at = np.nonzero((call < 4) & (ref < 4) & (call != ref))[0]
    out = np.zeros(at.size, dtype=VARIANT)
    rec = np.searchsorted(starts, at, side="right") - 1          # (empty records share a start: the last record that starts at or before)
    out["record"] = rec
    out["pos"] = at - starts[rec].astype(np.int64) if at.size else at
    out["ref"] = letters[at].view("S1")
    out["alt"] = cons[at].view("S1")
    out["depth"] = counts[at].sum(axis=1)
    out["alt_count"] = counts[at, call[at]]
    return out


def pair_inserts(place1: np.ndarray, place2: np.ndarray) -> np.ndarray:
    """Insert size of every pair from the placements of its mates (PLACE arrays of equal length): int64, -1 where there is none.  A
    pair has one when both mates are placed on the same record on opposite strands: `end` of the reverse mate - `start` of the
    forward mate, kept when 0 < size <= MAX_INSERT."""
    if len(place1) != len(place2):
        raise ValueError("the mates' placements differ in length")
    rec1, rec2 = place1["record"], place2["record"]
    ok = (rec1 < PLACE_AMBIGUOUS) & (rec1 == rec2) & (place1["strand"] != place2["strand"])
    fwd1 = place1["strand"] == 0
    start = np.where(fwd1, place1["start"], place2["start"]).astype(np.int64)
    end = np.where(fwd1, place2["end"], place1["end"]).astype(np.int64)
    size = end - start
    ok &= (size > 0) & (size <= MAX_INSERT)
    return np.where(ok, size, -1).astype(np.int64)


def _check_pairs(min_insert: int, max_insert: int, rescue_permille: int):
    if not 1 <= int(min_insert) <= int(max_insert) < 2 ** 31 or int(max_insert) - int(min_insert) + 1 > RESCUE_MAX:
        raise ValueError("the insert window is 1 <= min_insert <= max_insert, at most RESCUE_MAX inserts wide")
    if not 0 <= int(rescue_permille) <= 1000:
        raise ValueError("rescue_permille is a number from 0 to 1000")


class Paired(Verified):
    """What place_pairs gives (include/mitofilter.h, pairs): Verified's report fields over BOTH mate sets, and per set bits1 / bits2
    u32[ceil(n/32)], place1 / place2 PLACE[n], score1 / score2 SCORE[n]; pairs PAIR[n] (kind, insert), pair_records PAIR_RECORD[R] and
    pairs_none, the pairs without a settled mate.  A rescued mate's place row holds votes == 0.  bits, place, score, kept and total are
    None."""
    __slots__ = ("bits1", "bits2", "place1", "place2", "score1", "score2", "pairs", "pair_records", "pairs_none")


def place_pairs(ks: KmerSet, reads1: Reads, reads2: Reads, min_insert: int, max_insert: int, rescue: bool = True, rescue_permille: int = 100,
                min_depth: int = 1, max_permille: int = 1000, pileup: bool = True, threshold: int = 1, mode: int = MODE_SCREENED) -> Paired:
    """Both mate sets verified as verify_reads does it, into one set of counters; then pair by pair the insert and the kind of the pair
    and, with rescue=True, the rescue of a mate the vote cannot place: every insert d in [min_insert, max_insert] (at most RESCUE_MAX
    of them) gives one candidate on the settled mate's record and on the opposite strand, scored by the verification rule; the mate is
    placed on the one admissible candidate (compared >= k, mismatches * 1000 <= rescue_permille * compared) with strictly the fewest
    mismatches, and from there on counts as an accepted placed read (include/mitofilter.h: mf_place_pairs).  The default
    rescue_permille of 100, one base in ten, is a policy choice and not a measured value.  -> Paired."""
    _check_cut(min_depth, max_permille)
    _check_pairs(min_insert, max_insert, rescue_permille)
    n = reads1.info.n_reads
    if reads2.info.n_reads != n:
        raise ValueError("the mate sets differ in length")
    per1, results1 = _read_outputs(reads1, PLACE, SCORE)
    per2, results2 = _read_outputs(reads2, PLACE, SCORE)
    pairs = np.zeros(max(n, 1), dtype=PAIR)
    R = len(ks.record_starts) - 1
    pair_records = np.zeros(max(R, 1), dtype=PAIR_RECORD)
    none = C.c_uint64()
    ptrs, results = _report_outputs(ks, _VERIFY_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    _chk(load().mf_place_pairs(ks._h, reads1._h, reads2._h, threshold, mode, min_depth, max_permille, int(min_insert), int(max_insert), int(bool(rescue)),
                               int(rescue_permille), per1[0], per2[0], per1[1], per2[1], per1[2], per2[2], pairs.ctypes.data, *ptrs[:-1],
                               pair_records.ctypes.data, C.byref(none), ptrs[-1], None))
    bits1, place1, score1 = results1()
    bits2, place2, score2 = results2()
    return Paired(bits1=bits1, bits2=bits2, place1=place1, place2=place2, score1=score1, score2=score2, pairs=pairs[:n], pair_records=pair_records[:R],
                  pairs_none=none.value, **results())


class AlignedPairs(Aligned):
    """What align_pairs gives (include/mitofilter.h, pairs with a band): Aligned's report fields over BOTH mate sets -- indels,
    align_records and, when asked, the gapped and the extended fields among them -- and per set bits1 / bits2 u32[ceil(n/32)], place1 /
    place2 PLACE[n], align1 / align2 ALIGN[n]; pairs PAIR[n], pair_records PAIR_RECORD[R] and pairs_none as Paired holds them.  A
    rescued mate's place row holds votes == 0 and its align row the alignment around the seed.  bits, place, align and keep_bits are
    None: the paired call has no keep mode."""
    __slots__ = ("bits1", "bits2", "place1", "place2", "align1", "align2", "pairs", "pair_records", "pairs_none")


def align_pairs(ks: KmerSet, reads1: Reads, reads2: Reads, min_insert: int, max_insert: int, band: int = 8, rescue: bool = True,
                rescue_permille: int = 100, min_depth: int = 1, max_permille: int = 1000, pileup: bool = True, gapped: bool = False, extend: int = 0,
                threshold: int = 1, mode: int = MODE_SCREENED) -> AlignedPairs:
    """place_pairs with a band: both mate sets aligned as align_reads does it, into one set of counters; a mate is settled when the
    aligned cut accepts it; the rescue's candidates are scored ungapped exactly as place_pairs scores them, and the rescued mate is then
    aligned inside the band around the winning candidate and counts as an accepted aligned read (include/mitofilter.h: mf_align_pairs).
    The seed is ungapped: a mate with an indel well inside it is found only with a looser rescue_permille, since only its longer side
    matches on the seed's diagonal; the default of 100 is a policy choice and not a measured value.  gapped and extend as in align_reads.
    band = 0 is place_pairs.  -> AlignedPairs."""
    _check_cut(min_depth, max_permille)
    _check_band(band)
    _check_extend(extend)
    _check_pairs(min_insert, max_insert, rescue_permille)
    n = reads1.info.n_reads
    if reads2.info.n_reads != n:
        raise ValueError("the mate sets differ in length")
    per1, results1 = _read_outputs(reads1, PLACE, ALIGN)
    per2, results2 = _read_outputs(reads2, PLACE, ALIGN)
    pairs = np.zeros(max(n, 1), dtype=PAIR)
    R = len(ks.record_starts) - 1
    pair_records = np.zeros(max(R, 1), dtype=PAIR_RECORD)
    none = C.c_uint64()
    ptrs, results = _report_outputs(ks, _ALIGN_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    gptrs, gresults = _gapped_outputs(ks, band) if gapped else ([None] * 4, dict)
    xptrs, xresults = _extend_outputs(ks, band, extend) if int(extend) > 0 else ([None] * 4, dict)
    _chk(load().mf_align_pairs(ks._h, reads1._h, reads2._h, threshold, mode, min_depth, max_permille, int(band), int(extend), int(min_insert),
                               int(max_insert), int(bool(rescue)), int(rescue_permille), per1[0], per2[0], per1[1], per2[1], per1[2], per2[2],
                               pairs.ctypes.data, *ptrs[:-1], *gptrs, *xptrs, pair_records.ctypes.data, C.byref(none), ptrs[-1], None))
    bits1, place1, align1 = results1()
    bits2, place2, align2 = results2()
    return AlignedPairs(bits1=bits1, bits2=bits2, place1=place1, place2=place2, align1=align1, align2=align2, pairs=pairs[:n],
                        pair_records=pair_records[:R], pairs_none=none.value, **results(), **gresults(), **xresults())


def filter_resident(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED, steps: int = 1) -> FilterStats:
    st = FilterStats()
    _chk(load().mf_filter_resident(ks._h, reads._h, threshold, mode, steps, C.byref(st)))
    return st


def filter_resident_passes(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED, steps: int = 1):
    """`steps` passes back to back; -> (passing reads of every pass, stats)"""
    st = FilterStats()
    per = np.zeros(steps, dtype=np.uint64)
    _chk(load().mf_filter_resident_passes(ks._h, reads._h, threshold, mode, steps, per.ctypes.data, C.byref(st)))
    return per, st


def filter_resident_bits(ks: KmerSet, reads: Reads, threshold: int = 1, mode: int = MODE_SCREENED, steps: int = 1):
    """`steps` passes back to back; -> (bits[steps, words]: the result bitmap every pass left in its own buffer set, passing reads of every
    pass, stats).  Test support for the pipelined pass."""
    st = FilterStats()
    bits = np.zeros((max(steps, 1), (reads.info.n_reads + 31) // 32), dtype=np.uint32)          # (steps < 1: the library's error)
    per = np.zeros(max(steps, 1), dtype=np.uint64)
    _chk(load().mf_filter_resident_bits(ks._h, reads._h, threshold, mode, steps, bits.ctypes.data, per.ctypes.data, C.byref(st)))
    return bits, per, st


def filter_packed(ks: KmerSet, words, offsets, npos, threshold: int = 1, device: int = 0) -> np.ndarray:
    words = np.ascontiguousarray(words, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    npos = np.ascontiguousarray(npos, dtype=np.uint64)
    n = len(offsets) - 1
    bits = np.zeros((n + 31) // 32, dtype=np.uint32)
    _chk(load().mf_filter_packed(ks._h, device, words.ctypes.data, offsets.ctypes.data, n,
                                 npos.ctypes.data if npos.size else None, npos.size, threshold, bits.ctypes.data))
    return bits


def filter_fastq_files(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                       threshold: int = 1, pair_mode: int = PAIR_EITHER, n_devices: int = 1,
                       devices: Optional[Sequence[int]] = None) -> Tuple[int, int]:
    """-> (kept, total) reads (SE) or pairs (PE).  devices: an explicit list of device indices (instead of 0 .. n_devices - 1)."""
    kept, total = C.c_uint64(), C.c_uint64()
    if devices is not None:
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        _chk(load().mf_filter_fastq_files_on(ks._h, _enc(fq1), _enc(fq2), _enc(out1), _enc(out2), threshold, pair_mode,
                                             arr, len(devices), C.byref(kept), C.byref(total)))
    else:
        _chk(load().mf_filter_fastq_files(ks._h, _enc(fq1), _enc(fq2), _enc(out1), _enc(out2), threshold, pair_mode,
                                          n_devices, C.byref(kept), C.byref(total)))
    return kept.value, total.value


def _files_call(name: str, ks: KmerSet, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, *outs) -> Tuple[int, int]:
    """The file-level call `name` on `devices` (default 0 .. n_devices - 1); outs: what it takes between the device list and the
    counts.  -> (kept, total)."""
    if devices is None:
        devices = list(range(n_devices))
    arr = (C.c_int * len(devices))(*[int(d) for d in devices])
    kept, total = C.c_uint64(), C.c_uint64()
    _chk(getattr(load(), name)(ks._h, _enc(fq1), _enc(fq2), _enc(out1), _enc(out2), threshold, pair_mode, arr, len(devices), *outs,
                               C.byref(kept), C.byref(total)))
    return kept.value, total.value


def filter_fastq_files_by_record(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                                 threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                                 n_devices: int = 1):
    """filter_fastq_files plus the bait record of every kept read.  -> (kept, total, counts u64[R + 2]): kept reads (mates one by
    one) of each record, then ambiguous, then unassigned (a mate kept only through its partner).  devices: an explicit list of
    device indices (instead of 0 .. n_devices - 1)."""
    counts = np.zeros(_n_records(ks) + 2, dtype=np.uint64)
    kept, total = _files_call("mf_filter_fastq_files_by_record", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                              counts.ctypes.data)
    return kept, total, counts


def filter_fastq_files_by_group(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                                threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                                n_devices: int = 1):
    """filter_fastq_files_by_record by group of records.  -> (kept, total, counts u64[G + 2])."""
    counts = np.zeros(_n_groups(ks) + 2, dtype=np.uint64)
    kept, total = _files_call("mf_filter_fastq_files_by_group", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                              counts.ctypes.data)
    return kept, total, counts


def filter_fastq_files_depth(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                             threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                             n_devices: int = 1):
    """filter_fastq_files plus the k-mer depth of the bait positions over every mate that passes its own threshold (the pair rule
    decides only what is written).  -> (kept, total, profile u32[positions], records DEPTH_RECORD[R])."""
    starts = ks.record_starts
    P, R = int(starts[-1]), len(starts) - 1
    profile = np.zeros(max(P, 1), dtype=np.uint32)
    records = np.zeros(max(R, 1), dtype=DEPTH_RECORD)
    kept, total = _files_call("mf_filter_fastq_files_depth", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                              profile.ctypes.data, records.ctypes.data)
    return kept, total, profile[:P], records[:R]


def filter_fastq_files_placed(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                              threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                              n_devices: int = 1):
    """filter_fastq_files plus the placement on the bait of every mate that passes its own threshold (the pair rule decides only what
    is written).  -> (kept, total, base_depth u32[positions], records PLACE_RECORD[R], unplaced u64[2]: passing mates that are not
    placed, mates that do not pass)."""
    ptrs, results = _report_outputs(ks, _PLACE_FIELDS)
    kept, total = _files_call("mf_filter_fastq_files_placed", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, *ptrs)
    return (kept, total, *results().values())


def filter_fastq_files_pileup(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                              threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                              n_devices: int = 1, min_depth: int = 1):
    """filter_fastq_files plus the pile-up on the bait of every mate that passes its own threshold (the pair rule decides only what is
    written).  -> (kept, total, pileup PILEUP[positions], consensus u8[positions], records PILEUP_RECORD[R], unplaced u64[2]: passing
    mates that are not placed, mates that do not pass)."""
    ptrs, results = _report_outputs(ks, _PILEUP_FIELDS)
    kept, total = _files_call("mf_filter_fastq_files_pileup", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                              min_depth, *ptrs)
    return (kept, total, *results().values())


def filter_fastq_files_verified(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str],
                                threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                                n_devices: int = 1, min_depth: int = 1, max_permille: int = 1000, pileup: bool = True,
                                keep: int = KEEP_PASSING) -> Verified:
    """filter_fastq_files plus verified placement and (pileup=True) pile-up of every mate that passes its own threshold: the placed
    mates are scored against the bait and cut at max_permille.  keep = KEEP_PASSING: the pair rule decides only what is written and
    a rejected mate is still written.  KEEP_ACCEPTED: a rejected mate loses its bit before the pair rule; KEEP_PLACED: so does a passing
    mate that is not placed (mf_filter_fastq_files_verified_keep); the reports are the same under every keep mode.
    -> Verified with kept (what was written), total and the shared fields."""
    _check_cut(min_depth, max_permille, keep)
    ptrs, results = _report_outputs(ks, _VERIFY_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    if int(keep) == KEEP_PASSING:
        kept, total = _files_call("mf_filter_fastq_files_verified", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                                  min_depth, max_permille, *ptrs)
    else:
        kept, total = _files_call("mf_filter_fastq_files_verified_keep", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices,
                                  n_devices, min_depth, max_permille, int(keep), *ptrs)
    return Verified(kept=kept, total=total, **results())


def filter_fastq_files_aligned(ks: KmerSet, fq1: str, fq2: Optional[str], out1: str, out2: Optional[str], band: int = 8,
                               threshold: int = 1, pair_mode: int = PAIR_EITHER, devices: Optional[Sequence[int]] = None,
                               n_devices: int = 1, min_depth: int = 1, max_permille: int = 1000, pileup: bool = True,
                               keep: int = KEEP_PASSING, extend: int = 0, gapped: bool = False) -> Aligned:
    """filter_fastq_files_verified behind the banded alignment (mf_filter_fastq_files_aligned): the cut, the keep rule and the reports
    are those of align_reads, added over the mates.  gapped=True: the insertion pile added over the mates and the gapped consensus
    called from the sums (mf_filter_fastq_files_gapped).  extend=E > 0: the extension pile added over the mates and both ends of every
    record called from the sums (mf_filter_fastq_files_extended).  -> Aligned with kept, total and the shared fields."""
    _check_cut(min_depth, max_permille, keep)
    _check_band(band)
    _check_extend(extend)
    ptrs, results = _report_outputs(ks, _ALIGN_FIELDS, () if pileup else _PILEUP_FIELDS[:3])
    if int(extend) > 0:
        gptrs, gresults = _gapped_outputs(ks, band) if gapped else ([None] * 4, dict)
        xptrs, xresults = _extend_outputs(ks, band, extend)
        kept, total = _files_call("mf_filter_fastq_files_extended", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                                  min_depth, max_permille, int(keep), int(band), int(extend), *ptrs[:-1], *gptrs, *xptrs, ptrs[-1])
        return Aligned(kept=kept, total=total, **results(), **gresults(), **xresults())
    if not gapped:
        kept, total = _files_call("mf_filter_fastq_files_aligned", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                                  min_depth, max_permille, int(keep), int(band), *ptrs)
        return Aligned(kept=kept, total=total, **results())
    gptrs, gresults = _gapped_outputs(ks, band)
    kept, total = _files_call("mf_filter_fastq_files_gapped", ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices,
                              min_depth, max_permille, int(keep), int(band), *ptrs[:-1], *gptrs, ptrs[-1])
    return Aligned(kept=kept, total=total, **results(), **gresults())


def set_option(name: str, value) -> None:
    """Process-wide switch of how a filter pass is run (pass=default|split|serial, adapt, finish_streams, screen_streams, split_pipe,
    exact_co): the library does not read these from the environment unless MF_ENV_KNOBS=1."""
    _chk(load().mf_set_option(_enc(name), _enc(str(value))))


def last_ingest_stats() -> dict:
    """What this thread's last filter_fastq_files call did: which ingest path, bytes, seconds, device memory, decoder counters."""
    st = IngestStats()
    _chk(load().mf_last_ingest_stats(C.byref(st)))
    return st.as_dict()


def release_cached() -> int:
    """Give the device buffers, pinned staging and read sets the file-level calls keep between calls back to the runtime; returns
    the device bytes released (the library does the same by itself when one of its allocations finds a device full)."""
    v = C.c_uint64()
    _chk(load().mf_release_cached(C.byref(v)))
    return v.value


def h2d_bandwidth(device: int = 0, nbytes: int = 1 << 30, reps: int = 3) -> float:
    """GB/s of a pinned host-to-device copy on this box (the roof of the device ingest path)."""
    v = C.c_double()
    _chk(load().mf_h2d_bandwidth(device, nbytes, reps, C.byref(v)))
    return v.value


def qualfilter_files(fq1: Optional[str], fq2: Optional[str], out1: str, out2: Optional[str], start: int = 0, end: int = 0,
                     ns: int = 10, quality: int = 55, limit: float = 0.2, dedup: bool = False, trim: int = 0,
                     truncate_only: bool = False, device: int = 0) -> Tuple[int, int, bool]:
    """The reference's `filter_v2` rules (filter/filter_bin/src/main.rs) with GPU counting.
    -> (kept, total, panicked)."""
    kept, total, pan = C.c_uint64(), C.c_uint64(), C.c_int()
    _chk(load().mf_qualfilter_files(_enc(fq1), _enc(fq2), _enc(out1), _enc(out2), start, end, ns, quality, limit, int(dedup),
                                    trim, int(truncate_only), device, C.byref(kept), C.byref(total), C.byref(pan)))
    return kept.value, total.value, bool(pan.value)


def unpack_bits(bits: np.ndarray, n: int) -> np.ndarray:
    """u32 bitmap -> bool[n] (bit r of word r>>5)."""
    return np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
