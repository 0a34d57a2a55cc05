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


def test_border_distance():
    g0 = np.array([0, 1, 65536 - 31, 65536 - 30, 65536, 65537, 131072 - 100, 65536 + 40000], dtype=np.int64)
    assert ld.border_distance(g0, 31).tolist() == [0, 1, -1, 0, 0, 1, -70, -(65536 - 40000 - 30)]
