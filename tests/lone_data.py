"""Reads with ONE bait k-mer: a dense stream of random bases with single bait windows planted into it, at every alignment and at the
borders of the screen's units of work ("Lone-k-mer reads").  A bait-derived read has ~120 hits and eight or nine stage-1
positives, so whatever one of them drops another one catches; here a read passes through one window only, and a dropped owner
window, a missing table bit or an ownership range off by one at a border clears its bit.

Pure numpy, no loop over bases or reads.  The GPU side never sees the kinds: they are the diagnosis of a mismatch."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from mitoflex_amd.utility.synth_bait import bait_records

PLAIN, N_OUTSIDE, N_INSIDE, SUBSTITUTED, STRADDLE = range(5)
KINDS = ("plain", "n_outside", "n_inside", "substituted", "straddle")
# hits of the planted read in the oracle (straddle: of the read the window starts in and of the next one)
KIND_HITS = (1, 1, 0, 0, 0)
_KIND_EDGES = np.array([0.70, 0.80, 0.90, 0.95])

BORDER = 65536                    # bases between a lane's two 16-byte pieces (16 KiB of packed words); every second one ends a 32 KiB chunk
CHUNK_BASES = 2 * BORDER
MIN_CHUNKS = 526                  # more than twice the largest screen grid (256 workgroups): some workgroups take three chunks
UNIFORM_READS, UNIFORM_LEN = 460_000, 150
LAYOUTS = ("uniform", "ragged")
# the length axis: a third layout, ("uniform", L), of LENGTH_CHUNKS chunks.  The read arithmetic of the kernels (the division by L, the
# straddle test, the run start handed to the lane on the left) depends on a chunk's first base, not on how many chunks a workgroup takes,
# and the MIN_CHUNKS streams at L = 150 hold that other axis.
LENGTH_CHUNKS = 40
LENGTHS = (36, 64, 75, 100, 101, 125, 151, 250, 4095, 4096, 4097)
LENGTH_KS = (19, 21, 27, 28, 31, 32, 33, 41, 48, 63)      # the stride-8 geometries, the 32 | 33 key-word switch, 47 | 48 (the exact kernel behind finish)
LONG_READ = 70001                 # longer than a lane piece

# how a window came to its place
AT_RANDOM, AT_START, AT_END, AT_BORDER, AT_STREAM_START, AT_STREAM_END = range(6)


def first_record_codes(bait_text: str) -> np.ndarray:
    """the first bait record as codes 0..3 (it holds nothing but A, C, G, T)"""
    rec = bait_records(bait_text)[0].upper().encode()
    lut = np.full(256, 4, dtype=np.uint8)
    lut[list(b"ACGT")] = range(4)
    codes = lut[np.frombuffer(rec, dtype=np.uint8)]
    assert codes.size and codes.max() < 4, "the first bait record holds an invalid base"
    return codes


def layout_lens(layout: str, k: int, seed: int) -> np.ndarray:
    """read lengths of a layout, at least MIN_CHUNKS chunks in all; the first and the last read hold a window"""
    if layout == "uniform":
        lens = np.full(UNIFORM_READS, UNIFORM_LEN, dtype=np.int64)
    elif layout == "ragged":
        choice = np.array([0, k - 1, k, k + 1, 37, 100, 150, 150, 151, 250], dtype=np.int64)
        need = MIN_CHUNKS * CHUNK_BASES + 4096
        rng = np.random.default_rng([seed, k, 1])
        lens = choice[rng.integers(0, choice.size, size=int(need / choice.mean() * 1.03) + 64)]
        lens[0] = 150
        n = int(np.searchsorted(np.cumsum(lens), need)) + 1
        assert n < lens.size
        lens = lens[:n].copy()
        lens[-1] = 150
    else:
        raise ValueError(layout)
    assert int(lens.sum()) >= MIN_CHUNKS * CHUNK_BASES
    return lens


def uniform_lens(L: int, chunks: int = LENGTH_CHUNKS) -> np.ndarray:
    """read lengths of the layout ("uniform", L): the fewest reads of L bases that fill `chunks` chunks and 4096 bases more"""
    return np.full(-(-(chunks * CHUNK_BASES + 4096) // L), L, dtype=np.int64)


def lengths_for(k: int) -> list:
    """the uniform lengths run at k: both ends of "a read holds one window", lengths of every gcd with 16 and 64, the real ones (PE100,
    125, 151, 250), both sides of the 4096 limit of the 32-bit division, and for two k a read longer than a lane piece"""
    return sorted({L for L in (k, k + 1) + LENGTHS if L >= k}) + ([LONG_READ] if k in (31, 63) else [])


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """codes 0..3 -> u32 words of sixteen bases, base g in bits 2 (g & 15) of word g >> 4, plus eight zero words of slack"""
    n_words = (codes.size + 15) // 16
    padded = np.zeros((n_words + 8) * 16, dtype=np.uint8)
    padded[:codes.size] = codes
    q = padded.reshape(-1, 4)
    b = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
    return np.ascontiguousarray(b).view("<u4").astype(np.uint32, copy=False)


def lone_set(bait_text: str, k: int, lens, seed: int, share: float = 0.25) -> SimpleNamespace:
    """A stream of len(lens) reads of random bases with one window of k bait bases planted into about one read in four (`share` of them).

    -> words, offsets, npos (as Reads.from_packed / OracleReads.from_arrays take them) and, one entry a planted window in stream order:
    read (index of the read the window starts in), g0 (its first base in the stream), strand (0 the bait's, 1 its reverse complement), kind (PLAIN ..
    STRADDLE), how (AT_RANDOM .. AT_STREAM_END), border (the multiple of BORDER an AT_BORDER window was laid across, else -1)."""
    rng = np.random.default_rng([seed, k, 2])
    rec = first_record_codes(bait_text)
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    total = int(offsets[-1])
    assert n >= 2 and lens[0] >= k and lens[-1] >= k and rec.size > k + 2
    codes = rng.integers(0, 4, size=total, dtype=np.uint8)

    # ---- which reads, which kind, where in the read
    chosen = np.nonzero((rng.random(n) < share) & (lens >= k))[0]
    m = chosen.size
    kind = np.searchsorted(_KIND_EDGES, rng.random(m), side="right").astype(np.int8)
    L = lens[chosen]
    where = rng.integers(0, 6, size=m)
    pos = rng.integers(0, L - k + 1)
    pos = np.where(where == 0, 0, np.where(where == 1, L - k, pos))
    how = np.where(where == 0, AT_START, np.where(where == 1, AT_END, AT_RANDOM)).astype(np.int8)
    strad = kind == STRADDLE
    pos = np.where(strad, L - rng.integers(1, k, size=m), pos)          # starts 1..k-1 bases before the end of its read
    how[strad] = AT_RANDOM
    g0 = offsets[chosen] + pos

    # ---- the windows with a place of their own: across every border, at both ends of the stream
    B = np.arange(BORDER, total, BORDER, dtype=np.int64)
    j = B // BORDER
    rb = np.searchsorted(offsets, B, side="right") - 1                  # the read holding base B (zero-length reads hold none)
    d = (j // 2) % k                                                    # the odd and the even borders each go through 0..k-1
    gb = np.clip(B - d, offsets[rb], offsets[rb + 1] - k)
    fits = (lens[rb] >= k) & (rb > 0) & (rb < n - 1) & (gb + 4 * k + 8 < total - k)
    f_read = np.concatenate(([0], rb[fits], [n - 1]))
    f_g0 = np.concatenate(([0], gb[fits], [total - k]))
    f_how = np.concatenate(([AT_STREAM_START], np.full(int(fits.sum()), AT_BORDER), [AT_STREAM_END])).astype(np.int8)
    f_border = np.concatenate(([-1], B[fits], [-1]))

    keep = ~np.isin(chosen, f_read)
    read = np.concatenate((chosen[keep], f_read))
    g0 = np.concatenate((g0[keep], f_g0))
    kind = np.concatenate((kind[keep], np.full(f_read.size, PLAIN, dtype=np.int8)))
    how = np.concatenate((how[keep], f_how))
    border = np.concatenate((np.full(int(keep.sum()), -1, dtype=np.int64), f_border))
    forced = np.concatenate((np.zeros(int(keep.sum()), dtype=bool), np.ones(f_read.size, dtype=bool)))
    order = np.argsort(g0, kind="stable")
    read, g0, kind, how, border, forced = (a[order] for a in (read, g0, kind, how, border, forced))

    # ---- apart: a window that was placed at random goes when its neighbour is near (starts more than 3k + 4 apart: more than 2k + 4 bases between)
    apart = 3 * k + 4
    gap = np.diff(g0)
    near_prev = np.concatenate(([False], gap <= apart))
    fg = g0[forced]                                                     # (the last one is the stream's last window: every window has a next one)
    near_forced_next = fg[np.minimum(np.searchsorted(fg, g0, side="right"), fg.size - 1)] - g0 <= apart
    stay = forced | ~(near_prev | near_forced_next)
    read, g0, kind, how, border = (a[stay] for a in (read, g0, kind, how, border))
    # a straddling window leaves the reads it runs into unplanted: it goes when the next window starts in one of them
    runs_into = np.searchsorted(offsets, g0 + k - 1, side="right") - 1
    stay = ~((kind == STRADDLE) & (np.concatenate((read[1:], [n])) <= runs_into))
    read, g0, kind, how, border = (a[stay] for a in (read, g0, kind, how, border))
    m = read.size
    assert np.all(np.diff(g0) > apart) and g0[0] == 0 and g0[-1] == total - k
    pos = g0 - offsets[read]
    L = lens[read]

    # ---- the bait's k bases, the flanks chosen to differ from the bait's own
    b = rng.integers(1, rec.size - k, size=m)                           # (a neighbour on both sides)
    strand = rng.integers(0, 2, size=m).astype(np.int8)
    ar = np.arange(k)
    fwd = rec[b[:, None] + ar]
    rev = 3 - rec[b[:, None] + (k - 1 - ar)]
    win = np.where(strand[:, None] == 0, fwd, rev).astype(np.uint8)
    before = np.where(strand == 0, rec[b - 1], 3 - rec[b + k])
    after = np.where(strand == 0, rec[b + k], 3 - rec[b - 1])
    codes[g0[:, None] + ar] = win
    has_b, has_a = g0 > 0, g0 + k < total
    codes[g0[has_b] - 1] = (before[has_b] + rng.integers(1, 4, size=m)[has_b]) & 3
    codes[g0[has_a] + k] = (after[has_a] + rng.integers(1, 4, size=m)[has_a]) & 3

    sub = np.nonzero(kind == SUBSTITUTED)[0]
    mid = g0[sub] + k // 2
    codes[mid] = (codes[mid] + rng.integers(1, 4, size=sub.size)) & 3

    # ---- invalid bases: inside the window, or in the same read outside the window and its flanks (a read with no such place stays plain)
    lo, hi = np.maximum(pos - 1, 0), np.minimum(pos + k, L - 1)
    free = L - (hi - lo + 1)
    kind[(kind == N_OUTSIDE) & (free <= 0)] = PLAIN
    out = np.nonzero(kind == N_OUTSIDE)[0]
    q = rng.integers(0, free[out])
    q = np.where(q >= lo[out], q + (hi - lo + 1)[out], q)
    ins = np.nonzero(kind == N_INSIDE)[0]
    npos = np.sort(np.concatenate((offsets[read[out]] + q, g0[ins] + rng.integers(0, k, size=ins.size))))
    codes[npos] = 0

    return SimpleNamespace(k=k, n_reads=n, total=total, words=pack_codes(codes), offsets=offsets.astype(np.uint64), npos=npos.astype(np.uint64),
                           read=read, g0=g0, strand=strand, kind=kind, how=how, border=border, pos=pos, read_len=L)


def border_distance(g0: np.ndarray, k: int) -> np.ndarray:
    """signed distance of a window to the nearest multiple of BORDER: 0 when the window holds it, else the bases between (negative: the
    window ends before it)"""
    nxt = (g0 + BORDER - 1) // BORDER * BORDER                             # the first multiple at or after g0
    inside = nxt < g0 + k
    before = -(nxt - (g0 + k - 1))
    after = g0 - (nxt - BORDER)
    return np.where(inside, 0, np.where(-before <= after, before, after))


# one seed for every set.  (k = 19: 6e7 random windows against 3.5e4 bait keys of 4**19 leave about six chance hits in a stream, where
# tests/test_lone_data.py allows five unplanted reads with a hit; this seed holds that for both layouts -- should another one not, the
# seed changes, not the allowance.)
SEED = 20261019


# (k, L) of the length axis whose set under SEED breaks a condition of tests/test_lone_data.py -> the seed it takes instead
LENGTH_SEEDS = {}


def _with_oracle(k: int, layout, lens, seed: int, bait_text: str, share: float = 0.25) -> SimpleNamespace:
    from oracle import oracle_lib as ol
    s = lone_set(bait_text, k, lens, seed, share)
    s.layout = layout
    s.oreads = ol.OracleReads.from_arrays(s.words, s.offsets, s.npos)
    t = ol.OracleTable(bait_text, k)
    s.obits, s.ohits = ol.filter_reads(t, s.oreads, 1, threads=4)
    s.obits2, _ = ol.filter_reads(t, s.oreads, 2, threads=4)
    for a in (s.words, s.offsets, s.npos, s.obits, s.ohits, s.obits2, s.read, s.g0, s.strand, s.kind):
        a.flags.writeable = False
    return s


@functools.lru_cache(maxsize=16)
def _cached_layout(k: int, layout: str, bait_text: str) -> SimpleNamespace:
    return _with_oracle(k, layout, layout_lens(layout, k, SEED), SEED, bait_text)


@functools.lru_cache(maxsize=16)
def _cached_length(k: int, L: int, bait_text: str) -> SimpleNamespace:           # (a cache of their own: these small sets push no large one out)
    # 4095 .. 4097: 1281 reads in all.  One in four planted leaves some thirty plain windows at a read's first base, too few to start on all
    # sixteen places of a stream word, so every read of these sets is drawn
    share = 1.0 if 250 < L < LONG_READ else 0.25
    return _with_oracle(k, ("uniform", L), uniform_lens(L), LENGTH_SEEDS.get((k, L), SEED), bait_text, share)


@functools.lru_cache(maxsize=4)
def paired_set(k: int, layout: str, bait_text: str) -> SimpleNamespace:
    """The stream of cached_set(k, layout) with every two neighbouring reads taken as ONE read (every second offset; words and npos are the
    set's own), and the oracle's bits at threshold 2.  A lone set's own threshold-2 bitmap is all but empty -- empty for k >= 48, where no
    bait k-mer occurs twice -- so a threshold-2 pass on it can only show a bit that should not be there.  Here a read passes when both its
    halves hold a window: two hits, one from each, and a pass that loses either clears the bit.  -> n_reads, offsets, obits2."""
    from oracle import oracle_lib as ol
    s = cached_set(k, layout, bait_text)
    offsets = np.ascontiguousarray(np.concatenate((s.offsets[:-1:2], s.offsets[-1:])))
    obits2, _ = ol.filter_reads(ol.OracleTable(bait_text, k), ol.OracleReads.from_arrays(s.words, offsets, s.npos), 2, threads=4)
    for a in (offsets, obits2):
        a.flags.writeable = False
    return SimpleNamespace(k=k, layout=layout, n_reads=offsets.size - 1, offsets=offsets, obits2=obits2)


def cached_set(k: int, layout, bait_text: str) -> SimpleNamespace:
    """the set of (k, layout) with the oracle's answers: obits / ohits at threshold 1, obits2 at threshold 2 (one generation and two
    oracle runs a set, shared by every test of a module that asks for it; nothing writes to it).  layout: "uniform", "ragged", or
    ("uniform", L) for the LENGTH_CHUNKS stream of reads of L bases."""
    if isinstance(layout, tuple):
        assert layout[0] == "uniform" and len(layout) == 2
        return _cached_length(k, int(layout[1]), bait_text)
    return _cached_layout(k, layout, bait_text)
