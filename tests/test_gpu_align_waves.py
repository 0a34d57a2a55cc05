"""align_kernel with several reads a wave.  launch_align starts at most 32 waves a CU -- 8 192 on an MI355X --, so on the sets of
test_gpu_align.py every wave aligns one read and nothing it carries from a read to the next is ever used: its slice of work memory
(direction words and per-base entries, written again by a read of another length), lane 0's run of record sums and its flush when the
record changes, the histogram in LDS, the keep bits.  Here a wave sees four reads and more: about 400 distinct reads of every kind tiled
to 4 x 8 192 listed reads in a seeded shuffle, and the ragged set of test_gpu_align.py with a 29 999-base read in its middle, for which
the work memory allows 372 waves.  Everything is compared exactly through test_gpu_align.check with tests/align_oracle.py; the oracle runs on
the distinct reads only (tests/test_align_data.py holds the sets to their conditions without a device)."""
import functools

import numpy as np
import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import place_oracle as po
from tests.report_data import mf, ol, upload  # noqa: F401  (fixtures)
from tests.test_gpu_align import check, inputs, placement

pytestmark = pytest.mark.gpu

WAVES = 32 * 256          # what launch_align starts on an MI355X when the reads are more


def tiled_want(want, index, copies):
    """what AlignOracle.run gives for the tile from what it gave for the distinct reads: per-read outputs through the index, every
    additive output times copies; covered (place_rec[:, 4]) counts positions, not reads"""
    out = {f: want[f][index] for f in ("passes", "rows", "aligns", "accepted")}
    for f in ("depth", "counts", "indels", "footprints", "align_rec"):
        out[f] = want[f] * (np.uint64(copies) if want[f].dtype == np.uint64 else copies)
    out["place_rec"] = want["place_rec"] * np.array([copies] * 4 + [1, copies], np.uint64)
    out["unplaced"] = [u * copies for u in want["unplaced"]]
    return out


@functools.lru_cache(maxsize=None)
def distinct_tile():
    parts = inputs()[1]
    distinct, _ = ad.distinct_reads(parts)
    return (distinct,) + ad.tiled_reads(distinct, ad.TILE_COPIES, seed=5)


@pytest.mark.parametrize("k,band,keep", [(31, 8, "KEEP_ACCEPTED"), (21, 4, "KEEP_PLACED")])
def test_tiled_reads_match_oracle(mf, ol, k, band, keep):
    text = inputs()[0]
    distinct, seqs, index = distinct_tile()
    o = placement(k)[0]
    want = ao.AlignOracle(o).run(distinct, o.tally(distinct), 1, ad.TILE_CUT, band)
    tiled = tiled_want(want, index, ad.TILE_COPIES)
    assert int(tiled["passes"].sum()) >= 4 * WAVES          # four listed reads a wave at the least
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    assert reads.info.uniform_len == 0
    a = check(mf, ks, reads, o, seqs, tiled, band, ad.TILE_CUT, getattr(mf, keep))
    assert int(a.align_records["gapped"].sum()) >= 60 * ad.TILE_COPIES and int(a.align_records["rejected"].min()) >= 10 * ad.TILE_COPIES
    reads.close(); ks.close()


def test_tiled_uniform_reads_match_oracle(mf, ol):
    """reads of one length: max_len is the set's uniform_len, not the length kernel's"""
    text, parts = inputs()[:2]
    distinct = ad.uniform_distinct(parts)
    seqs, index = ad.tiled_reads(distinct, ad.UNIFORM_COPIES, seed=6)
    o = placement(31)[0]
    want = ao.AlignOracle(o).run(distinct, o.tally(distinct), 1, ad.TILE_CUT, 8)
    tiled = tiled_want(want, index, ad.UNIFORM_COPIES)
    assert int(tiled["passes"].sum()) >= 4 * WAVES
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, seqs)
    assert reads.info.uniform_len == ad.UNIFORM_LEN
    check(mf, ks, reads, o, seqs, tiled, 8, ad.TILE_CUT, mf.KEEP_ACCEPTED)
    reads.close(); ks.close()


# a band is narrower than k: 30 is the widest at k = 31; the widest there is, 31 (63 lanes), takes k = 41
@pytest.mark.parametrize("k,band", [(31, 8), (31, 30), (41, 31)])
def test_capped_launch_matches_oracle(mf, ol, k, band):
    """The longest read bounds the work memory of every wave: with 29 999 bases 372 waves fit, each aligns five reads and more, and the
    slice that held the long read's direction words and entries serves reads of 40 to 300 bases afterwards (and held some before)"""
    text, parts = inputs()[:2]
    seqs, at = ad.capped_reads(parts)
    o = placement(k)[0]
    want = ao.AlignOracle(o).run(seqs, o.tally(seqs), 1, 50, band)
    assert int(want["passes"].sum()) > 5 * 372
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    a = check(mf, ks, reads, o, seqs, want, band, 50, mf.KEEP_ACCEPTED)
    assert [int(a.place[f][at]) for f in ("record", "strand", "start", "end")] == [0, 0, -13496, 16503]
    assert [int(a.align[f][at]) for f in ("compared", "mismatches", "insertions", "deletions", "ref_begin", "ref_end")] == [2996, 0, 3, 4, -13500, 16500]
    assert bool(want["accepted"][at]) and (int(a.keep_bits[at >> 5]) >> (at & 31)) & 1
    lo = len(seqs) - 1                                              # the 2 000-base read of the ragged set, behind it
    assert len(seqs[lo]) == 2000 and int(a.align["deletions"][lo]) == 5
    reads.close(); ks.close()
