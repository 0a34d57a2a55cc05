"""The read sets of test_gpu_align_waves.py and test_gpu_align_files.py (tests/align_data.py: distinct_reads, tiled_reads, long_read,
capped_reads, align_mates) held to their conditions from the oracles alone, with no device: the GPU tests cannot pass on a degenerate set."""
import functools
import os
import re

import numpy as np

from tests import align_data as ad
from tests import align_oracle as ao
from tests import place_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES_ASSUMED = 32 * 256          # launch_align's waves on an MI355X: 32 on each of 256 CUs


@functools.lru_cache(maxsize=None)
def bait():
    return ad.align_bait()


@functools.lru_cache(maxsize=None)
def oracle(k):
    return po.PlaceOracle(bait()[0], k)


def run(seqs, k, band, cut):
    o = oracle(k)
    return ao.AlignOracle(o).run(seqs, o.tally(seqs), 1, cut, band)


def wave_bound(max_len):
    """the rule of mf_align.hip's header and mf_align_launch.h: the work memory's bytes over a wave's -- eight bytes a word, 64 words for
    every 32 rows begun and one word a base"""
    src = open(os.path.join(ROOT, "mitoflex_amd", "csrc", "mf_align.hip")).read()
    m = re.search(r"ALIGN_WORK_BYTES\s*=\s*(\d+)ull\s*<<\s*(\d+)", src)
    assert m and int(m.group(1)) << int(m.group(2)) == 256 << 20
    return (256 << 20) // (8 * (64 * ((max_len + 31) // 32) + max_len))


def test_present_builders_give_what_they_gave():
    """the new builders stand beside the old ones: the sets of test_gpu_align.py are the same reads (sizes, and a checksum of the text)"""
    import hashlib
    _, parts = bait()
    seqs, groups = ad.ragged_reads(parts)
    assert len(seqs) == 2007 and groups["long"] == (2006, 2007) and len(seqs[2006]) == 2000
    h = lambda reads: hashlib.md5("\n".join(reads).encode()).hexdigest()
    assert h(seqs) == RAGGED_MD5 and h(ad.uniform_reads(parts, 100, 300, seed=200)) == UNIFORM_MD5


RAGGED_MD5 = "faced1dfd2bb734104164ecc2bcea812"
UNIFORM_MD5 = "84a5e1de82eb903e1ee142f6ad953db3"


def test_distinct_reads_hold_every_kind():
    _, parts = bait()
    seqs, groups = ad.distinct_reads(parts)
    assert 380 <= len(seqs) <= 420 and len(set(seqs)) == len(seqs)
    assert all(40 <= len(s) <= 300 for s in seqs[:-1]) and len(seqs[-1]) < 21
    assert set(groups) == {"plain", "indel", "over", "ns", "repeat", "far", "tie", "random"}
    lo, hi = groups["ns"]
    assert all("N" in s for s in seqs[lo:hi - 6])
    w = run(seqs, 31, 8, 40)
    rows, al = w["rows"], w["aligns"]
    placed = rows[:, 0] < po.AMBIGUOUS
    for j, ln in enumerate(oracle(31).lens):
        on = placed & (rows[:, 0] == j)
        assert (on & w["accepted"]).sum() >= 10 and (on & ~w["accepted"]).sum() >= 10, j          # accepted and rejected reads on every record
        assert (on & (rows[:, 1] == 0)).sum() >= 10 and (on & (rows[:, 1] == 1)).sum() >= 10, j   # both strands
        assert (on & w["accepted"] & (al[:, 4] < 0)).any() and (on & w["accepted"] & (al[:, 5] > ln)).any(), j          # over both ends
    assert (al[:, 2] > 0).sum() >= 30 and (al[:, 3] > 0).sum() >= 30
    assert (w["accepted"] & (al[:, 2] > 0)).sum() >= 30 and (w["accepted"] & (al[:, 3] > 0)).sum() >= 30
    assert (w["passes"] & ~placed).sum() >= 10 and (~w["passes"]).sum() >= 10
    lo, hi = groups["tie"]
    assert (w["passes"][lo:hi] & ~placed[lo:hi]).sum() >= 10
    lo, hi = groups["random"]
    assert not w["passes"][lo:hi].any()
    lo, hi = groups["far"]
    assert (placed[lo:hi] & ~w["accepted"][lo:hi]).sum() >= 25
    lo, hi = groups["repeat"]
    assert placed[lo:hi].sum() >= 15 and (w["indels"][:, 0] > 0).any() and (w["indels"][:, 1] > 0).any()
    # the second configuration of the tiled test tells its keep modes apart as well
    v = run(seqs, 21, 4, 40)
    assert (v["accepted"]).sum() >= 150 and ((v["rows"][:, 0] < po.AMBIGUOUS) & ~v["accepted"]).sum() >= 50 and (v["passes"] & (v["rows"][:, 0] >= po.AMBIGUOUS)).sum() >= 10


def test_tiled_reads_are_every_read_copies_times_shuffled():
    distinct = ["r%d" % i for i in range(57)]
    reads, index = ad.tiled_reads(distinct, 9, seed=3)
    assert len(reads) == len(index) == 57 * 9 and np.array_equal(np.bincount(index), np.full(57, 9))
    assert reads == [distinct[i] for i in index]
    again = ad.tiled_reads(distinct, 9, seed=3)
    assert again[0] == reads and np.array_equal(again[1], index) and not np.array_equal(ad.tiled_reads(distinct, 9, seed=4)[1], index)
    # shuffled: hardly any read stands beside a copy of itself or of its neighbour in `distinct`
    assert (np.abs(np.diff(index)) <= 1).mean() < 0.1


def test_tiles_list_four_reads_a_wave_and_reach_no_clamp():
    """what test_gpu_align_waves.py's tiled sets stand on: the passing reads number 4 x 8 192 at least, and no counter comes near its clamp
    (the largest is the tile's copies times the distinct set's)"""
    _, parts = bait()
    seqs, _ = ad.distinct_reads(parts)
    for k, band in ((31, 8), (21, 4)):
        w = run(seqs, k, band, ad.TILE_CUT)
        assert int(w["passes"].sum()) * ad.TILE_COPIES >= 4 * WAVES_ASSUMED
        assert max(int(w["depth"].max()), int(w["counts"].max()), int(w["align_rec"].max()), int(w["place_rec"].max())) * ad.TILE_COPIES < 1 << 24
    useqs = ad.uniform_distinct(parts)
    assert {len(s) for s in useqs} == {100} and useqs[:ad.UNIFORM_DISTINCT] == ad.uniform_reads(parts, 100, ad.UNIFORM_DISTINCT, seed=ad.UNIFORM_SEED)
    w = run(useqs, 31, 8, ad.TILE_CUT)
    assert int(w["passes"].sum()) * ad.UNIFORM_COPIES >= 4 * WAVES_ASSUMED
    assert (w["aligns"][:, 2] > 0).sum() >= 20 and (w["aligns"][:, 3] > 0).sum() >= 20 and 0 < w["accepted"].sum() < (w["rows"][:, 0] < po.AMBIGUOUS).sum()
    assert set(w["rows"][w["accepted"], 0].tolist()) == {0, 1, 2}
    # paths that end off the winning diagonal (ref_end is not the placement's end), beside the many that end on it
    off = w["accepted"] & (w["aligns"][:, 5] != w["rows"][:, 3])
    assert off.sum() >= 20 and (w["accepted"] & ~off).sum() >= 150
    assert max(int(w["depth"].max()), int(w["counts"].max()), int(w["align_rec"].max())) * ad.UNIFORM_COPIES < 1 << 24


def test_long_read_is_what_the_cap_test_expects():
    _, parts = bait()
    s = ad.long_read(parts)
    assert len(s) == 29999
    # (a band is narrower than k: 30 is the widest at k = 31, and 31, the widest there is, needs k = 41)
    for k, band in ((21, 8), (31, 8), (31, 30), (41, 31)):
        w = run([s], k, band, 50)
        assert w["rows"][0, :4].tolist() == [0, 0, -13496, 16503]
        assert w["aligns"][0].tolist() == [2996, 0, 3, 4, -13500, 16500] and w["accepted"].tolist() == [True]


def test_the_cap_binds_on_the_set_with_the_long_read():
    """256 MiB over eight times (64 words for every 32 rows and a word a base): 372 waves for the 29 999-base read, fewer than a fifth of
    the reads the set lists, and fewer than the waves an uncapped launch would start"""
    assert wave_bound(29999) == 372 and wave_bound(300) > WAVES_ASSUMED
    seqs, at = ad.capped_reads(bait()[1])
    assert len(seqs[at]) == 29999 and len(seqs) // 3 < at < 2 * len(seqs) // 3
    assert max(len(s) for i, s in enumerate(seqs) if i != at) == 2000
    o = oracle(31)
    listed = int(o.place(o.tally(seqs), 1)[0].sum())
    assert 372 * 5 < listed and 372 < min(WAVES_ASSUMED, len(seqs))
    assert 40 <= min(len(s) for s in seqs) and sorted(len(s) for s in seqs)[len(seqs) // 2] <= 300


def pair_rule(bits, both):
    return (bits[0] & bits[1]) if both else (bits[0] | bits[1])


def test_mates_of_the_file_tests():
    """two mates of about 960 reads: the indel reads lie in every batch of 300, the 2 000-base read in a batch behind the first, the
    oracle tells the three keep modes apart under both pair rules, and every record takes accepted and rejected reads"""
    m1, m2, at = ad.align_mates(bait()[1])
    assert len(m1) == len(m2) and 940 <= len(m1) <= 980
    assert len(m1[at]) == 2000 and at >= 2 * ad.FILE_BATCH and max(len(s) for i, s in enumerate(m1) if i != at) <= 300 and max(map(len, m2)) <= 300
    want = [run(m, 31, ad.FILE_BAND, ad.FILE_CUT) for m in (m1, m2)]
    for w in want:
        gapped = (w["aligns"][:, 2] + w["aligns"][:, 3] > 0) & w["accepted"]
        for b in range(0, len(m1), ad.FILE_BATCH):
            assert gapped[b:b + ad.FILE_BATCH].sum() >= 20, b
        assert (w["align_rec"][:, 0] > 0).all() and (w["align_rec"][:, 1] > 0).all()
    assert want[0]["aligns"][at, 3] == 5 and want[0]["accepted"][at]
    bits = {keep: [ao.keep_bits(w, keep) for w in want] for keep in (0, 1, 2)}
    for both in (False, True):
        n = [int(pair_rule(bits[keep], both).sum()) for keep in (0, 1, 2)]
        assert n[0] > n[1] > n[2] > 0, n
    for keep in (0, 1, 2):
        assert int((bits[keep][0] ^ bits[keep][1]).sum()) > 0          # a pair written through one mate only
