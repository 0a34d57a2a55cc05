"""The lone-k-mer generator (tests/lone_data.py) against the C oracle alone: every kind of planted read has the hit count it was built
for, the unplanted reads have none, and the windows fall on every alignment and across every kind of border.  Conditions on the INPUT
of tests/test_gpu_lone.py, not on the kernels: no GPU."""
import numpy as np
import pytest

from tests import lone_data as ld

KS = [19, 23, 28, 31, 33, 48, 63]
MIN_KIND_SHARE = 0.995          # (the remainder: bait k-mers that occur twice, e.g. inside the poly-T and poly-A runs)
MAX_STRAY_READS = 5             # unplanted reads with a hit (chance: ~6e7 windows against ~3.5e4 keys of 4**k)


@pytest.fixture(scope="module")
def ol():
    from oracle import oracle_lib
    oracle_lib.lib()
    return oracle_lib


@pytest.fixture(scope="module")
def lone(ol, bait_text):
    return lambda k, layout: ld.cached_set(k, layout, bait_text)


def _coverage(s):
    """what the planted positions cover, as (name, got, want at least) rows"""
    k = s.k
    plain = s.kind == ld.PLAIN
    rows = [("(g0 mod 64, strand) among plain windows", np.unique((s.g0[plain] % 64) * 2 + s.strand[plain]).size, 128)]
    want16 = 16 if s.layout == "ragged" else 8
    rows.append(("g0 mod 16 at in-read position 0", np.unique(s.g0[plain & (s.pos == 0)] % 16).size, want16))
    rows.append(("g0 mod 16 at in-read position len - k", np.unique(s.g0[plain & (s.pos == s.read_len - k)] % 16).size, want16))
    at = s.how == ld.AT_BORDER
    d = s.border[at] - s.g0[at]
    odd = (s.border[at] // ld.BORDER) % 2 == 1
    assert np.all((d >= 0) & (d < k))
    rows.append(("d at odd multiples of 65 536 (lane-piece border)", np.unique(d[odd]).size, k))
    rows.append(("d at multiples of 131 072 (chunk border)", np.unique(d[~odd]).size, k))
    return rows, {"d_odd_missing": sorted(set(range(k)) - set(d[odd].tolist())), "d_even_missing": sorted(set(range(k)) - set(d[~odd].tolist())),
                  "borders": int(at.sum()), "of": (s.total - 1) // ld.BORDER}


@pytest.mark.parametrize("layout", ld.LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_layout_reaches_the_third_chunk_of_a_workgroup(lone, k, layout):
    s = lone(k, layout)
    assert s.total >= ld.MIN_CHUNKS * ld.CHUNK_BASES
    assert s.words.size == (s.total + 15) // 16 + 8 and not s.words[-8:].any()
    assert s.offsets[0] == 0 and s.offsets[-1] == s.total and s.offsets.size == s.n_reads + 1
    assert np.all(np.diff(s.npos.astype(np.int64)) > 0)
    w = s.words[(s.npos >> np.uint64(4)).astype(np.int64)] >> (2 * (s.npos & np.uint64(15))).astype(np.uint32)
    assert not (w & 3).any(), "an invalid base is stored as 0"
    if layout == "uniform":
        assert s.n_reads == 460_000 and np.all(np.diff(s.offsets.astype(np.int64)) == 150)
    else:
        lens = np.diff(s.offsets.astype(np.int64))
        assert set(np.unique(lens).tolist()) == {0, k - 1, k, k + 1, 37, 100, 150, 151, 250}
        assert 600_000 < s.n_reads < 800_000
    assert 0.08 * s.n_reads < s.read.size < 0.25 * s.n_reads          # one read in four is drawn; reads shorter than k and near neighbours go
    assert np.all(np.diff(s.g0) > 2 * k + 4 + k)


@pytest.mark.parametrize("layout", ld.LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_every_kind_has_its_hit_count(lone, k, layout):
    s = lone(k, layout)
    hits = s.ohits.astype(np.int64)
    shares = {}
    for kind, name in enumerate(ld.KINDS):
        sel = s.kind == kind
        assert sel.sum() > 0.02 * s.read.size, (k, layout, name, int(sel.sum()))
        ok = hits[s.read[sel]] == ld.KIND_HITS[kind]
        if kind == ld.STRADDLE:
            ok &= hits[s.read[sel] + 1] == 0
        shares[name] = (float(ok.mean()), int(sel.sum()))
    print(k, layout, {n: "%.4f of %d" % v for n, v in shares.items()})
    for name, (share, _) in shares.items():
        assert share >= MIN_KIND_SHARE, (k, layout, name, shares)
    # the windows that hold a place of their own (borders, stream ends) are plain and must ALL be single hits or known repeats
    planted = np.zeros(s.n_reads, dtype=bool)
    planted[s.read] = True
    planted[s.read[s.kind == ld.STRADDLE] + 1] = True                 # (the read a straddling window runs into has 0 hits: counted above)
    stray = int((hits[~planted] > 0).sum())
    assert stray <= MAX_STRAY_READS, (k, layout, stray)
    # threshold 2: nearly all clear
    from tests.util_data import bits_to_bool
    assert np.array_equal(bits_to_bool(s.obits, s.n_reads), hits >= 1)
    assert np.array_equal(bits_to_bool(s.obits2, s.n_reads), hits >= 2)
    assert (hits >= 2).sum() <= 0.005 * s.read.size


@pytest.mark.parametrize("layout", ld.LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_windows_cover_every_alignment_and_border(lone, k, layout):
    s = lone(k, layout)
    rows, detail = _coverage(s)
    table = "\n".join("%-55s %4d (want >= %d)" % r for r in rows)
    assert all(got >= want for _, got, want in rows), "coverage of (k=%d, %s):\n%s\n%s" % (k, layout, table, detail)
    assert s.g0[0] == 0 and s.kind[0] == ld.PLAIN and s.read[0] == 0
    assert s.g0[-1] + k == s.total and s.kind[-1] == ld.PLAIN and s.read[-1] == s.n_reads - 1


RESIDENT_BITS_KS = [21, 31, 41, 48, 63]          # the sets whose every pipelined pass tests/test_gpu_resident_bits.py reads


@pytest.mark.parametrize("layout", ld.LAYOUTS)
@pytest.mark.parametrize("k", RESIDENT_BITS_KS)
def test_expected_bitmaps_show_a_moved_or_stale_bit(lone, bait_text, k, layout):
    """What the per-pass bit comparisons rest on: some reads pass and not all; some read r has bit r set and bit r ^ 1 clear, so that a pass
    bit moved to the neighbouring read (every count stays right) changes the bitmap; and the two thresholds, which run on one handle, differ
    in their bits.  The threshold-1 bitmap holds all of it at every k.  The set's own threshold-2 bitmap does NOT for k >= 48: no bait
    k-mer occurs twice, no read has two hits, the bitmap is empty (measured when this test was written: 0 reads at k = 48 and 63, both
    layouts) -- a threshold-2 pass on the set itself shows only the bits of the threshold-1 passes before it that were not cleared.  So the
    threshold-2 passes are also run on the stream with two neighbouring reads taken as one (lone_data.paired_set), whose bitmap holds
    every condition at every k."""
    from tests.sequence_data import moved_bit_shows
    from tests.util_data import bits_to_bool
    s, p = lone(k, layout), ld.paired_set(k, layout, bait_text)
    n1, n2, np2 = (int(bits_to_bool(b, n).sum()) for b, n in ((s.obits, s.n_reads), (s.obits2, s.n_reads), (p.obits2, p.n_reads)))
    print(k, layout, "pass at threshold 1:", n1, "at threshold 2:", n2, "at threshold 2, reads paired:", np2, "of", p.n_reads)
    assert 0 < n1 < s.n_reads and moved_bit_shows(s.obits, s.n_reads), (k, layout, n1)
    assert not np.array_equal(s.obits, s.obits2)
    assert (n2 == 0) == (k >= 48) and (n2 == 0 or moved_bit_shows(s.obits2, s.n_reads)), (k, layout, n2)
    assert p.n_reads == (s.n_reads + 1) // 2 and p.offsets[0] == 0 and p.offsets[-1] == s.total and np.array_equal(p.offsets[:-1], s.offsets[:-1:2])
    assert 0.002 * p.n_reads < np2 < 0.1 * p.n_reads and moved_bit_shows(p.obits2, p.n_reads), (k, layout, np2)


# --------------------------------------------------------------------------- the length axis: ("uniform", L), LENGTH_CHUNKS chunks
MAX_STRAY_READS_SHORT = 3       # (the stream is 13 times shorter than the one MAX_STRAY_READS was set for)
KL = [(k, L) for k in ld.LENGTH_KS for L in ld.lengths_for(k)]


def reachable_alignments(k, L):
    """How many (g0 mod 64, strand) a window inside a read of L bases can take.  A read starts at a multiple of g = gcd(L, 64) and the
    window at one of the L - k + 1 places in it, so g0 mod g takes min(g, L - k + 1) values and g0 mod 64 takes 64 / g times as many.
    All 128 for most (k, L); measured and explained at (21, 64): every read starts at g0 mod 64 = 0, the window at 0 .. 43 in it, which is
    44 residues on two strands = 88.  ((31, 32): reads start at 0 or 32 and the window at 0 or 1: 4 residues, 8.)"""
    g = int(np.gcd(L, 64))
    return 2 * (64 // g) * min(g, L - k + 1)


def test_reachable_alignments():
    assert reachable_alignments(21, 64) == 88 and reachable_alignments(31, 32) == 8 and reachable_alignments(63, 64) == 4
    assert all(reachable_alignments(31, L) == 128 for L in (31, 36, 75, 100, 101, 125, 151, 250))
    assert reachable_alignments(19, 20) == 64 and reachable_alignments(48, 48) == 8 and reachable_alignments(33, 36) == 128


@pytest.mark.parametrize("k,L", KL)
def test_uniform_length_set(lone, k, L):
    """the conditions of a ("uniform", L) set: the layout, the hit counts of the kinds, the alignments and the borders the windows reach"""
    s = lone(k, ("uniform", L))
    n = -(-(ld.LENGTH_CHUNKS * ld.CHUNK_BASES + 4096) // L)
    assert s.n_reads == n and s.total == n * L and s.total >= ld.LENGTH_CHUNKS * ld.CHUNK_BASES + 4096
    assert s.offsets[0] == 0 and s.offsets.size == n + 1 and np.all(np.diff(s.offsets.astype(np.int64)) == L)
    assert s.words.size == (s.total + 15) // 16 + 8 and not s.words[-8:].any()
    assert np.all(np.diff(s.npos.astype(np.int64)) > 0)
    w = s.words[(s.npos >> np.uint64(4)).astype(np.int64)] >> (2 * (s.npos & np.uint64(15))).astype(np.uint32)
    assert not (w & 3).any(), "an invalid base is stored as 0"
    assert np.all(np.diff(s.g0) > 2 * k + 4 + k)
    assert s.g0[0] == 0 and s.kind[0] == ld.PLAIN and s.read[0] == 0
    assert s.g0[-1] + k == s.total and s.kind[-1] == ld.PLAIN and s.read[-1] == n - 1
    at = s.how == ld.AT_BORDER
    d = s.border[at] - s.g0[at]
    assert np.all((d >= 0) & (d < k)) and np.all(s.kind[at] == ld.PLAIN)
    assert (s.total - 1) // ld.BORDER == 2 * ld.LENGTH_CHUNKS
    if L == ld.LONG_READ:
        # several forced border windows fall in one read: the hit counts of the kinds do not apply
        assert n == 75 and int(at.sum()) >= 78, (k, L, int(at.sum()))
        return
    assert int(at.sum()) >= 2 * ld.LENGTH_CHUNKS - 1, (k, L, int(at.sum()))          # (L = 4096: the last border is the last read's first base)

    if L <= 250:
        assert s.read.size >= 0.08 * n, (k, L, s.read.size, n)
    else:
        assert s.read.size >= 250, (k, L, s.read.size)
    hits = s.ohits.astype(np.int64)
    good = 0
    shares = {}
    for kind, name in enumerate(ld.KINDS):
        sel = s.kind == kind
        ok = hits[s.read[sel]] == ld.KIND_HITS[kind]
        if kind == ld.STRADDLE:
            ok &= hits[s.read[sel] + 1] == 0
        good += int(ok.sum())
        shares[name] = (float(ok.mean()) if sel.any() else 1.0, int(sel.sum()))       # (n_outside: none when the window and its flanks fill the read)
    print(k, L, {name: "%.4f of %d" % v for name, v in shares.items()})
    for name, (share, count) in shares.items():
        if count >= 400:
            assert share >= MIN_KIND_SHARE, (k, L, name, shares)
    assert good >= 0.99 * s.read.size, (k, L, shares)
    planted = np.zeros(n, dtype=bool)
    planted[s.read] = True
    planted[s.read[s.kind == ld.STRADDLE] + 1] = True
    stray = int((hits[~planted] > 0).sum())
    assert stray <= MAX_STRAY_READS_SHORT, (k, L, stray)                               # (should a set break this: its seed changes, lone_data.LENGTH_SEEDS)
    from tests.util_data import bits_to_bool
    assert np.array_equal(bits_to_bool(s.obits, n), hits >= 1)
    assert np.array_equal(bits_to_bool(s.obits2, n), hits >= 2)

    plain = s.kind == ld.PLAIN
    if L <= 250:
        got = np.unique((s.g0[plain] % 64) * 2 + s.strand[plain]).size
        assert got == reachable_alignments(k, L), (k, L, got)
    # a read's first and last window on every place of a stream word that reads of L bases start on: 16 // gcd(L, 16) of them.  The reads that
    # hold a multiple of 65 536 carry their window across it, not at an end; at L = 4095 and 4097 these are the reads 16 j and 16 j + 15, all
    # the reads of one place, which leaves 15 of 16 at one end of the read (measured, every k: L = 4095 16 at the start -- the stream's first
    # window is the sixteenth -- and 15 at the end; L = 4097 15 at the start and 16 at the end, with the stream's last window).  Required:
    # every place that a read without a border starts on.
    starts = s.offsets.astype(np.int64)[:-1]
    free = np.ones(n, dtype=bool)
    free[np.arange(ld.BORDER, s.total, ld.BORDER) // L] = False
    free[[0, n - 1]] = False                                                           # (the stream's first and last window: `own` below)
    for name, at_pos, shift, own in (("first", 0, 0, 0), ("last", L - k, L - k, s.total - k)):
        got = set((s.g0[plain & (s.pos == at_pos)] % 16).tolist())
        want = set(((starts[free] + shift) % 16).tolist()) | {own % 16}
        assert want <= got and len(got) <= 16 // int(np.gcd(L, 16)), (k, L, name, sorted(want - got))
        if L <= 250:
            assert len(got) == 16 // int(np.gcd(L, 16)), (k, L, name, sorted(got))


def test_existing_layouts_are_what_they_were(bait_text):
    """the length axis left the two MIN_CHUNKS layouts byte for byte as they were (md5 of words, offsets, npos at k = 31)"""
    import hashlib
    want = {"uniform": ("b9f5974ccdd17a8ccebf780895713845", "de215e6ec3883f26368546e76d601053", "9e93ea9d2e4135adb4029c680c562100"),
            "ragged": ("b50538feacdb8b418a4c47bf0ef804a1", "6c2f5bbb092d115fa0f65824a24f52fa", "1d131aec448ba6bc2609ba228b874788")}
    for layout in ld.LAYOUTS:
        s = ld.lone_set(bait_text, 31, ld.layout_lens(layout, 31, ld.SEED), ld.SEED)
        assert tuple(hashlib.md5(a.tobytes()).hexdigest() for a in (s.words, s.offsets, s.npos)) == want[layout], layout


def test_border_distance():
    g0 = np.array([0, 1, 65536 - 31, 65536 - 30, 65536, 65537, 131072 - 100, 65536 + 40000], dtype=np.int64)
    assert ld.border_distance(g0, 31).tolist() == [0, 1, -1, 0, 0, 1, -70, -(65536 - 40000 - 30)]
