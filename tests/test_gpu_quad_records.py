"""GPU parity of the quad records ("Quad records"): a threshold-1 pass of a stride-16 set behind the plain LDS-table screen
records one ScreenRec per FOUR lanes -- a record row is sixteen consecutive samples, 256 bases -- and the finish kernels' quad variant
settles them.  Ten chunks of 131 072 bases: several workgroups, both rows of a chunk, quads, lane and quad borders, a chunk border.

Every case builds its stream on the host, asserts FROM THE STREAM that the situation it is about is really there (the true stage-1
positives are the stream-aligned words that are bait 16-mers; the screen adds false positives, never drops one), and then compares
ALL pass bits of every read with the C oracle.  The host side (build_* below) runs without a GPU.

PARITY UNPINNED BY THE REFERENCE (SURVEY.md 8a group B): the oracle is this repository's own.  Bar: bit-exact.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from mitoflex_amd.utility.synth_bait import bait_records
from tests import lone_data as ld
from tests.util_data import bits_to_bool

pytestmark = pytest.mark.gpu

CHUNKS = 10
CHUNK = ld.CHUNK_BASES            # 131 072 bases: two rows (u = 0, 1) of 65 536, a row of 1024 lane pieces of 64 bases
ROW = ld.BORDER
LANE, QUAD, S, STRIDE = 64, 256, 16, 16
SEED = 20261020
KS = (31, 32, 33, 41, 63)


def n_adj(k):
    """samples of a run: the fewest neighbouring samples that span k bases (finish_kernel)"""
    return (k - S + STRIDE - 1) // STRIDE + 1


# ------------------------------------------------------------------------------------------------------------- host side
def _lut():
    lut = np.full(256, 4, dtype=np.uint8)
    lut[list(b"ACGT")] = range(4)
    lut[list(b"acgt")] = range(4)
    return lut


@functools.lru_cache(maxsize=2)
def bait_smers(bait_text):
    """every 16-mer of the bait, both strands, as it would lie in a stream word (base j in bits 2j)"""
    out = []
    sh = 2 * np.arange(S, dtype=np.uint64)
    for rec in bait_records(bait_text):
        c = _lut()[np.frombuffer(rec.encode(), dtype=np.uint8)]
        for codes in (c, np.where(c < 4, 3 - c, 4)[::-1]):
            if codes.size < S:
                continue
            w = np.lib.stride_tricks.sliding_window_view(codes, S)
            ok = (w < 4).all(axis=1)
            out.append(((w[ok].astype(np.uint64) << sh).sum(axis=1)).astype(np.uint32))
    return np.unique(np.concatenate(out))


def unpack_codes(words, total):
    return ((words[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).ravel()[:total].copy()


def bait_piece(rec, rng, n):
    """n bait bases of either strand"""
    b = int(rng.integers(1, rec.size - n - 1))
    return rec[b:b + n] if rng.integers(0, 2) == 0 else (3 - rec[b:b + n])[::-1]


def finish_set(bait_text, k, codes, offsets, npos, **extra):
    """pack, ask the oracle (threshold 1 and 2, hit counts), find the true positives and the read each lies in (-1: in none)"""
    from oracle import oracle_lib as ol
    codes[npos] = 0
    total = int(offsets[-1])
    s = SimpleNamespace(k=k, n_reads=offsets.size - 1, total=total, words=ld.pack_codes(codes), offsets=offsets.astype(np.uint64),
                        npos=np.sort(npos).astype(np.uint64), **extra)
    oreads = ol.OracleReads.from_arrays(s.words, s.offsets, s.npos)
    t = ol.OracleTable(bait_text, k)
    s.obits, s.ohits = ol.filter_reads(t, oreads, 1, threads=4)
    s.obits2, _ = ol.filter_reads(t, oreads, 2, threads=4)
    s.passes = bits_to_bool(s.obits, s.n_reads)
    pos = np.nonzero(np.isin(s.words[:total // S], bait_smers(bait_text)))[0].astype(np.int64) * S          # first base of every true positive
    r = np.searchsorted(offsets, pos, side="right") - 1
    s.pos_g = pos
    s.pos_read = np.where(pos + S <= offsets[np.minimum(r + 1, s.n_reads)], r, -1)
    for a in (s.words, s.offsets, s.npos, s.obits, s.ohits, s.obits2):
        a.flags.writeable = False
    return s


def run_starts(s):
    """first base of the first and of the last sample of every run of n_adj(k) neighbouring true positives inside one read"""
    have = np.zeros(s.total // S + 8, dtype=bool)
    have[s.pos_g[s.pos_read >= 0] // S] = True
    n = n_adj(s.k)
    i = s.pos_g[s.pos_read >= 0] // S
    ok = np.ones(i.size, dtype=bool)
    for j in range(1, n):
        ok &= have[i + j]
    g = i[ok] * S
    last = g + (n - 1) * STRIDE
    same_read = np.searchsorted(s.offsets.astype(np.int64), g, side="right") == np.searchsorted(s.offsets.astype(np.int64), last + S - 1, side="right")
    return g[same_read], last[same_read]


def assert_runs_cross_borders(s):
    """some run crosses a lane border inside a quad, some run crosses a quad border (its samples lie in two records)"""
    g, last = run_starts(s)
    assert g.size
    lane_x = (g // LANE != last // LANE) & (g // QUAD == last // QUAD)
    quad_x = g // QUAD != last // QUAD
    assert lane_x.any(), "no run crosses a lane border inside a quad"
    assert quad_x.any(), "no run crosses a quad border"
    return int(lane_x.sum()), int(quad_x.sum())


def assert_rows_of_many_reads(s, least=3):
    """some record row holds true positives of >= `least` reads, of which one passes and one does not"""
    inr = s.pos_read >= 0
    row, rd = s.pos_g[inr] // QUAD, s.pos_read[inr]
    pairs = np.unique(np.stack((row, rd), axis=1), axis=0)
    rows, first, count = np.unique(pairs[:, 0], return_index=True, return_counts=True)
    good = 0
    for f, c in zip(first[count >= least], count[count >= least]):
        p = s.passes[pairs[f:f + c, 1]]
        good += bool(p.any() and not p.all())
    assert good, "no record row holds positives of %d reads of which one passes and one does not" % least
    return good


def row_plan(offsets, lens, taken, k, B):
    """(read, sample, window start) for every free read that can hold k bases around one of its samples in the 256-base row at B"""
    plan = []
    r0, r1 = np.searchsorted(offsets, [B, B + QUAD - 1], side="right") - 1
    for r in range(int(r0), int(r1) + 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        p = max(B, -(-lo // S) * S)                                      # the read's first sample in the row
        w = min(max(p - 7, lo), hi - k)
        if lens[r] >= k and not taken[r] and p + S <= min(hi, B + QUAD) and w <= p and p + S <= w + k:
            plan.append((r, p, w))
    return plan


def plant_dense_rows(codes, offsets, k, rec, rng, taken):
    """In both rows u of four chunks, one 256-base row in which three or more reads each get a window of k bait bases around one sample of the
    row -- whole in every second read (it passes), with one base outside the sample changed in the others (a positive whose read holds no
    bait k-mer); which of the two comes first alternates from row to row."""
    lens = np.diff(offsets)
    n_rows = 0
    for c in (0, 1, CHUNKS // 2, CHUNKS - 1):
        for u in (0, 1):
            for B in c * CHUNK + u * ROW + QUAD * rng.permutation(ROW // QUAD):
                plan = row_plan(offsets, lens, taken, k, int(B))
                if len(plan) < 3:
                    continue
                for i, (r, p, w) in enumerate(plan):
                    codes[w:w + k] = bait_piece(rec, rng, k)
                    if (i + n_rows) & 1:
                        x = w + k - 1 if w + k - 1 >= p + S else w
                        codes[x] = (codes[x] + 1 + rng.integers(0, 3)) & 3
                    taken[r] = True
                n_rows += 1
                break
    assert n_rows == 8


@functools.lru_cache(maxsize=32)
def build_bait_reads(bait_text, k, L):
    """Bait reads at every offset: uniform reads of L bases, a bait read starting at every base offset against a quad border that a
    read of L bases can start at (L = 151: all 256; L = 150: the 128 even ones), once in each row u; one more across a chunk border."""
    rng = np.random.default_rng([SEED, k, L, 1])
    rec = ld.first_record_codes(bait_text)
    n = -(-(CHUNKS * CHUNK + 4096) // L)
    offsets = np.arange(n + 1, dtype=np.int64) * L
    codes = rng.integers(0, 4, size=n * L, dtype=np.uint8)
    start = offsets[:-1]
    u_of = (start % CHUNK) // ROW
    whole = (start % ROW) + L <= ROW                                      # the read lies in one row of one chunk
    chosen, seen = [], set()
    for r in rng.permutation(n):
        key = (int(u_of[r]), int(start[r] % QUAD))
        if whole[r] and key not in seen:
            seen.add(key)
            chosen.append(int(r))
    step = int(np.gcd(L, QUAD))
    assert seen == {(u, o) for u in (0, 1) for o in range(0, QUAD, step)}, "an offset against the quad border is missing"
    straddler = int(np.searchsorted(offsets, 3 * CHUNK, side="right") - 1)
    assert offsets[straddler] < 3 * CHUNK < offsets[straddler + 1] - S, "no read lies across the chunk border"
    chosen.append(straddler)
    for r in chosen:
        codes[offsets[r]:offsets[r + 1]] = bait_piece(rec, rng, L)
    s = finish_set(bait_text, k, codes, offsets, np.zeros(0, dtype=np.int64), L=L, bait_reads=np.array(chosen))
    assert s.passes[s.bait_reads].all()
    s.crossings = assert_runs_cross_borders(s)
    return s


def _lone_base(bait_text, k, lens, seed):
    lone = ld.lone_set(bait_text, k, lens, seed)
    offsets = lone.offsets.astype(np.int64)
    codes = unpack_codes(lone.words, lone.total)
    taken = np.zeros(lens.size, dtype=bool)
    taken[lone.read] = True
    taken[np.minimum(lone.read + 1, lens.size - 1)] = True              # (a straddling window runs into the next read)
    return lone, offsets, codes, taken


@functools.lru_cache(maxsize=32)
def build_many_reads(bait_text, k, L):
    """Several reads in one record: lone-k-mer reads (lone_data.lone_set: plain, substituted, with an N, cut by a read border) beside reads
    with no hit, and rows in which every read holds a window of k bait bases, whole or with one base changed."""
    rng = np.random.default_rng([SEED, k, L, 2])
    lens = ld.uniform_lens(L, CHUNKS)
    lone, offsets, codes, taken = _lone_base(bait_text, k, lens, SEED)
    plant_dense_rows(codes, offsets, k, ld.first_record_codes(bait_text), rng, taken)
    s = finish_set(bait_text, k, codes, offsets, lone.npos.astype(np.int64), L=L)
    assert (~s.passes).sum() > s.n_reads // 2, "reads with no hit are most of the stream"
    s.rows = assert_rows_of_many_reads(s, least=3)
    return s


@functools.lru_cache(maxsize=8)
def build_ragged(bait_text, k):
    """Ragged reads of 60 .. 150 bases: lone-k-mer reads, rows of many reads, and one read in twenty a bait read"""
    rng = np.random.default_rng([SEED, k, 3])
    lens = rng.integers(60, 151, size=int((CHUNKS * CHUNK + 4096) / 105 * 1.02) + 8).astype(np.int64)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), CHUNKS * CHUNK + 4096)) + 1]
    lens[0] = lens[-1] = 150
    lone, offsets, codes, taken = _lone_base(bait_text, k, lens, SEED + 1)
    rec = ld.first_record_codes(bait_text)
    plant_dense_rows(codes, offsets, k, rec, rng, taken)
    whole = np.nonzero(~taken & (rng.random(lens.size) < 0.05))[0]
    for r in whole:
        codes[offsets[r]:offsets[r + 1]] = bait_piece(rec, rng, int(lens[r]))
    s = finish_set(bait_text, k, codes, offsets, lone.npos.astype(np.int64), L=0, bait_reads=whole)
    assert np.unique(lens).size > 80 and s.passes[whole].all()
    s.crossings = assert_runs_cross_borders(s)
    s.rows = assert_rows_of_many_reads(s, least=3)
    return s


@functools.lru_cache(maxsize=8)
def build_n_bases(bait_text, k):
    """Invalid bases.  (a) bait reads with an N inside a run: one N near the middle, in the place of an A -- an N is stored as an A, so the
    stream's words, the positives and the run are those of the whole bait read and only the has-N path knows (the read still passes through
    the windows beside it) -- or one every k - 1 bases (no window is whole: positives, no pass).  (b) bait reads in which ONE window of k bases is whole -- an N right
    before it and right behind it, more of them every k - 1 bases outside -- and that window starts 1 .. 15 bases before a lane border inside
    a quad: the sample that owns it is the first one of the NEXT lane of the same quad."""
    rng = np.random.default_rng([SEED, k, 4])
    rec = ld.first_record_codes(bait_text)
    L = 150
    n = -(-(CHUNKS * CHUNK + 4096) // L)
    offsets = np.arange(n + 1, dtype=np.int64) * L
    codes = rng.integers(0, 4, size=n * L, dtype=np.uint8)
    npos, kinds, reads, owners, mids = [], [], [], [], []
    free = list(rng.permutation(np.arange(1, n - 1)))
    for i in range(64):                                                   # (a)
        r = int(free.pop())
        lo = int(offsets[r])
        codes[lo:lo + L] = bait_piece(rec, rng, L)
        a = lo + 40 + int(np.nonzero(codes[lo + 40:lo + L - 40] == 0)[0][0])
        npos += [a] if i & 1 else list(range(lo + k - 1, lo + L, k - 1))
        mids += [a] if i & 1 else []
        kinds.append("mid" if i & 1 else "every")
        reads.append(r)
    for d in range(1, 16):                                                # (b)
        for _ in range(4):
            while True:
                r = int(free.pop())
                lo = int(offsets[r])
                border = [b for b in range(-(-lo // LANE) * LANE, lo + L, LANE) if b % QUAD and b - d - 1 >= lo and b - d + k + 1 <= lo + L]
                if border:
                    break
            b = int(border[int(rng.integers(0, len(border)))])
            w = b - d
            codes[lo:lo + L] = bait_piece(rec, rng, L)
            npos += list(range(w - 1, lo - 1, -(k - 1))) + list(range(w + k, lo + L, k - 1))
            kinds.append("one")
            reads.append(r)
            owners.append((w, b))
    npos = np.array(sorted(set(npos)), dtype=np.int64)
    s = finish_set(bait_text, k, codes, offsets, npos, L=L, n_reads_planted=np.array(reads), kinds=np.array(kinds))
    # (a): the N lies between two true positives of its read that a run would join
    g, last = run_starts(s)
    mid = s.n_reads_planted[s.kinds == "mid"]
    n_mid = np.array(mids)
    j = np.searchsorted(g, n_mid, side="right") - 1
    assert ((g[j] <= n_mid) & (n_mid < last[j] + S)).all(), "an N in the place of an A lies outside every run"
    assert s.passes[mid].all() and not s.passes[s.n_reads_planted[s.kinds == "every"]].any()
    # (b): exactly one whole window, and the first sample at or behind its start lies in the next lane of the same quad
    isn = np.zeros(s.total + 1, dtype=np.int64)
    isn[npos] = 1
    cum = np.concatenate(([0], np.cumsum(isn)))
    for r, (w, b) in zip(s.n_reads_planted[s.kinds == "one"], owners):
        lo = int(offsets[r])
        starts = np.arange(lo, lo + L - k + 1)
        whole = starts[cum[starts + k] - cum[starts] == 0]
        assert whole.tolist() == [w], (r, w, whole)
        own = -(-w // S) * S
        assert own == b and own // LANE == w // LANE + 1 and own // QUAD == w // QUAD
        assert (s.pos_g == own).any(), "the owner of the whole window is not a positive"
    assert s.passes[s.n_reads_planted[s.kinds == "one"]].all()
    return s


# -------------------------------------------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def mf(built_lib):
    from mitoflex_amd import mitofilter
    if mitofilter.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return mitofilter


@pytest.fixture()
def opened(mf, bait_text):
    """opened(s) -> (k-mer set, resident reads) of a set whose default threshold-1 pass uses quad records; closed afterwards"""
    held = []

    def open_(s):
        ks = mf.KmerSet.from_text(bait_text, s.k)
        reads = mf.Reads.from_packed(s.words, s.offsets, s.npos)
        held.extend((reads, ks))
        assert ks.info.screen_stride == STRIDE and ks.info.screen_s == S and ks.info.front_mode == 0, "not a set that records by quads"
        assert int(reads.info.uniform_len) == s.L
        return ks, reads
    yield open_
    for x in held:
        x.close()


def check_default_pass(mf, s, ks, reads):
    bits, _, st = mf.filter_reads(ks, reads, 1, mf.MODE_SCREENED)
    if not np.array_equal(bits, s.obits):
        got = bits_to_bool(bits, s.n_reads)
        lost, spurious = np.nonzero(s.passes & ~got)[0], np.nonzero(got & ~s.passes)[0]
        pytest.fail("pass bits differ from the oracle's (k = %d, L = %d): lost %d %s, spurious %d %s; stream offsets of the first lost reads against "
                    "their quad %s" % (s.k, s.L, lost.size, lost[:8].tolist(), spurious.size, spurious[:8].tolist(),
                                       (s.offsets[lost[:8]].astype(np.int64) % QUAD).tolist()))
    assert st.n_pass == int(s.passes.sum())
    return bits


@pytest.mark.parametrize("L", (150, 151))
@pytest.mark.parametrize("k", KS)
def test_bait_reads_at_every_offset(mf, opened, bait_text, k, L):
    s = build_bait_reads(bait_text, k, L)
    check_default_pass(mf, s, *opened(s))


@pytest.mark.parametrize("L", (31, 36, 75, 150))
def test_several_reads_in_one_record(mf, opened, bait_text, L):
    s = build_many_reads(bait_text, 31, L)
    check_default_pass(mf, s, *opened(s))


@pytest.mark.parametrize("k", (31, 41))
def test_ragged_reads(mf, opened, bait_text, k):
    s = build_ragged(bait_text, k)
    check_default_pass(mf, s, *opened(s))


@pytest.mark.parametrize("k", (31, 41))
def test_n_bases(mf, opened, bait_text, k):
    s = build_n_bases(bait_text, k)
    check_default_pass(mf, s, *opened(s))


@pytest.mark.parametrize("k", (31, 41))
def test_pipelined_passes(mf, opened, bait_text, k):
    """seven passes in flight over two (k = 41: three) buffer sets: every pass's count is the popcount of the single-pass bits, which
    are the oracle's"""
    for s in (build_bait_reads(bait_text, k, 150), build_ragged(bait_text, k)):
        ks, reads = opened(s)
        bits = check_default_pass(mf, s, ks, reads)
        want = int(bits_to_bool(bits, s.n_reads).sum())
        per, _ = mf.filter_resident_passes(ks, reads, 1, mf.MODE_SCREENED, 7)
        assert [int(x) for x in per] == [want] * 7
        check_default_pass(mf, s, ks, reads)


@pytest.mark.parametrize("k", (31, 41))
def test_other_pass_kinds_keep_lane_records(mf, opened, bait_text, k):
    """threshold 2 and hit counts go through mark_kernel and the exact kernel, which read per-lane records: on the same inputs, between
    two default passes, they still equal the oracle"""
    for s in (build_bait_reads(bait_text, k, 150), build_n_bases(bait_text, k), build_ragged(bait_text, k)):
        ks, reads = opened(s)
        check_default_pass(mf, s, ks, reads)
        bits2, _, st2 = mf.filter_reads(ks, reads, 2, mf.MODE_SCREENED)
        assert np.array_equal(bits2, s.obits2) and st2.n_pass == int(bits_to_bool(s.obits2, s.n_reads).sum())
        bits, hits, _ = mf.filter_reads(ks, reads, 1, mf.MODE_SCREENED, want_hits=True)
        assert np.array_equal(hits, s.ohits) and np.array_equal(bits, s.obits)
        check_default_pass(mf, s, ks, reads)
