"""Data for the places where the pair kernels (mf_pairs.hip) change their code path (test_pair_edge_data.py, test_gpu_pair_edges.py):
rescue targets around the longest read a wave stages (994 bases), uniform-length target sets that hold Ns, bait Ns under the rescue
candidates, baits on either side of the pair counters' LDS limit (170 records), and more pairs than one turn of pair_list_kernel's
grid.  Every builder returns (text, seqs1, seqs2, what); `what` names how each pair was drawn.  Seeded, pure Python; what the sets
hold is checked in test_pair_edge_data.py with the oracle alone.

The long bait (long_bait).  `ends` (3100 bases): a diverged stretch of 1300, 500 own bases, a diverged stretch of 1300 -- the targets
that hang over a record's begin or end lie there.  `long` (2300): 400 own bases, the diverged stretch D of 1500, 400 own bases.
`other` (500): unrelated.  The sample is the bait with another letter every 20 bases along the diverged stretches (no 21-mer in
common) and 200 bases of flank around every record.  Inside D, at ECHO_AT, the bait repeats k + 4 of `long`'s first bases and the
sample keeps them (the positions on either side differ): a target over that echo holds bait k-mers, none of them an anchor, so it
passes and is ambiguous; with an N in the echo's middle no k-window of it is left and the target does not pass."""
import random

import numpy as np

from tests import pair_data as pd
from tests import scale_data as sd
from tests.report_data import fasta
from tests.util_data import revcomp

STAGE_MAX = 994                                          # the longest read rescue_kernel stages (16 * 64 - 30)
LONG_WINDOW = (1650, 1665)
LONG_LENGTHS = (993, 994, 995, 1200)
FLANK = 200
ECHO_AT, ECHO_FROM = 1200, 20
N_OFFSETS = (0, 31, 32, 63, 64, 95, 96)                  # and L - 1: the edges of the 32-bit words a ballot round fills
N_STRADDLES = ((63, 64), (62, 63, 64), (63, 64, 65))


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(c):
    return "CGTA"["ACGT".index(c)]


def with_n(s, offsets):
    t = list(s)
    for i in offsets:
        t[i] = "N"
    return "".join(t)


def long_bait(k, seed=41):
    """-> (FASTA text, {name: record}, {name: sample record with its flanks}, E) with E = k + 4, the echo's length"""
    rng = random.Random(seed)
    E = k + 4
    ends = _rand(rng, 1300) + _rand(rng, 500) + _rand(rng, 1300)
    long_ = list(_rand(rng, 400) + _rand(rng, 1500) + _rand(rng, 400))
    long_[ECHO_AT:ECHO_AT + E] = long_[ECHO_FROM:ECHO_FROM + E]
    long_ = "".join(long_)
    other = _rand(rng, 500)
    s_ends = pd.substituted(ends[:1300], 20, 7) + ends[1300:1800] + pd.substituted(ends[1800:], 20, 7)
    s_long = list(long_[:400] + pd.substituted(long_[400:1900], 20, 7) + long_[1900:])
    s_long[ECHO_AT:ECHO_AT + E] = long_[ECHO_AT:ECHO_AT + E]
    # no window that reaches beyond the echo is the bait's, there or where the echo comes from
    for p, q in ((ECHO_AT - 1, ECHO_FROM - 1), (ECHO_AT + E, ECHO_FROM + E)):
        s_long[p] = next(c for c in "ACGT" if c not in (long_[p], long_[q]))
    recs = {"ends": ends, "long": long_, "other": other}
    sample = {"ends": s_ends, "long": "".join(s_long), "other": other}
    sample = {n: _rand(rng, FLANK) + s + _rand(rng, FLANK) for n, s in sample.items()}
    return fasta([(n, recs[n]) for n in ("ends", "long", "other")]), recs, sample, E


def _cut(sample, name, begin, end):
    """bases [begin, end) of the record's coordinates out of its sample"""
    assert -FLANK <= begin < end <= len(sample[name]) - FLANK
    return sample[name][FLANK + begin:FLANK + end]


class _Ragged:
    """pairs added one by one; a target (mate 2) is put behind a filler pair of random reads that brings its first base to the wanted
    place in its word of the packed stream (tests/test_gpu_verify.sweep_reads does the same for single reads)"""

    def __init__(self, rng):
        self.rng, self.seqs1, self.seqs2, self.what, self.b0 = rng, [], [], [], 0

    def add(self, m1, m2, what, bmod=None):
        if bmod is not None:
            fill = 21 + ((bmod - self.b0 - 21) % 16)          # 21 .. 36 random bases: a pair of kind none
            self.add(_rand(self.rng, 150), _rand(self.rng, fill), ("filler",))
            assert self.b0 % 16 == bmod
        self.seqs1.append(m1)
        self.seqs2.append(m2)
        self.what.append(what)
        self.b0 += len(m2)


def _n_form(m2, form, mid):
    """the three forms of a target: 0 without an N, 1 with one N at offset `mid`, 2 with Ns at its first and last base"""
    return m2 if form == 0 else with_n(m2, (mid,)) if form == 1 else with_n(m2, (0, len(m2) - 1))


def _long_pair(rng, sample, E, L, strand, ins):
    """a settled mate of 150 own bases of `long` and a target of L bases wholly inside D, on `strand`, `ins` apart -> (mate 1, target,
    the target's start, the read offset of the echo's middle)"""
    if strand == 1:          # forward settled mate in the first own bases, the target behind it
        a = rng.randint(100, 200)
        end = a + ins
        start = end - L
        m1, fwd = _cut(sample, "long", a, a + 150), _cut(sample, "long", start, end)
    else:                    # reverse settled mate in the last own bases, the target in front of it
        e = rng.randint(2100, 2250)
        start = e - ins
        m1, fwd = revcomp(_cut(sample, "long", e - 150, e)), _cut(sample, "long", start, start + L)
    assert 400 <= start and start + L <= 1900
    mid = ECHO_AT + E // 2 - start
    return m1, (revcomp(fwd) if strand else fwd), start, (L - 1 - mid if strand else mid)


def long_targets(k, seed=7):
    """targets of 993, 994, 995 and 1200 bases around the staging limit: what = ("long", L, strand, form, b0 mod 16, start) for the
    targets inside D, ("hang", L, strand, form, b0 mod 16, start) for those over an end of `ends`, ("filler",) for the pairs between"""
    text, recs, sample, E = long_bait(k)
    rng = random.Random(seed)
    S = _Ragged(rng)
    lo, hi = LONG_WINDOW
    cells = [(L, bm) for L in (994, 995) for bm in range(16)] + [(L, bm) for L in (993, 1200) for bm in (15, 6)]
    for L, bm in cells:
        for strand in (0, 1):
            for form in (0, 1, 2):
                m1, m2, start, mid = _long_pair(rng, sample, E, L, strand, rng.randint(lo, hi))
                assert start <= ECHO_AT and ECHO_AT + E <= start + L
                S.add(m1, _n_form(m2, form, mid), ("long", L, strand, form, bm, start), bmod=bm)
    # over the end of `ends`: a forward settled mate in its own bases, the reverse target `over` bases beyond the record; over its
    # begin: a reverse settled mate, the forward target beginning `over` bases in front of the record
    n_ends = len(recs["ends"])
    bm = 15
    for L in (994, 1200):
        for over in (5, 37):
            for strand in (0, 1):
                for form in (0, 1, 2):
                    ins = rng.randint(lo, hi)
                    if strand == 1:
                        start = n_ends + over - L
                        a = start + L - ins
                        m1, m2 = _cut(sample, "ends", a, a + 150), revcomp(_cut(sample, "ends", start, start + L))
                    else:
                        start = -over
                        e = start + ins
                        m1, m2 = revcomp(_cut(sample, "ends", e - 150, e)), _cut(sample, "ends", start, start + L)
                    assert 1300 <= (a if strand else e - 150) and (a + 150 if strand else e) <= 1800
                    S.add(m1, _n_form(m2, form, L // 2), ("hang", L, strand, form, bm, start), bmod=bm)
                    bm = (bm + 5) % 16
    starts = np.cumsum([0] + [len(s) for s in S.seqs2[:-1]])
    for b0, w in zip(starts, S.what):
        assert w[0] == "filler" or int(b0) % 16 == w[4]
    return text, S.seqs1, S.seqs2, S.what


def uniform_targets(L, k=31, seed=11, n=None):
    """both sets of one length each: mate 1 of 150 bases, mate 2 of L (150: `n` = 120 pairs; beyond that 48).  Targets in D of
    long_bait(k) in both directions; two in three hold Ns, over the set at offsets 0, 31, 32, 63, 64, 95, 96 and L - 1 and, in the
    150 set, two and three in a row across 63 | 64.  what = ("uniform", strand, the N offsets) or ("single",) (a random mate 2) or
    ("none",)"""
    text, recs, sample, E = long_bait(k)
    rng = random.Random(seed + L)
    n = n or (120 if L <= 150 else 48)
    forms = [(o,) for o in N_OFFSETS] + [(L - 1,)] + (list(N_STRADDLES) if L == 150 else [])
    seqs1, seqs2, what = [], [], []
    lo, hi = LONG_WINDOW
    drawn = [0, 0]
    for i in range(n):
        if i % 24 == 23:
            seqs1.append(_rand(rng, 150)); seqs2.append(_rand(rng, L)); what.append(("none",))
            continue
        strand = i % 2
        m1, m2, start, _ = _long_pair(rng, sample, E, L, strand, lo + (i * 7) % (hi - lo + 1))
        if i % 24 == 11:
            seqs1.append(m1); seqs2.append(_rand(rng, L)); what.append(("single",))
            continue
        t = drawn[strand]                                         # every third target of a strand without an N, the others through the forms
        drawn[strand] += 1
        at = () if t % 3 == 2 else forms[(t - t // 3) % len(forms)]
        seqs1.append(m1); seqs2.append(with_n(m2, at)); what.append(("uniform", strand, at))
    return text, seqs1, seqs2, what


# ------------------------------------------------------------------ bait Ns under the candidates
BAIT_N_WINDOW = (400, 463)
BAIT_N_RUNS = ((416, 1), (431, 16), (479, 33))           # (start, positions) inside D of pair_bait's r0; start mod 32 = 0, 15, 31
BAIT_N_EDGE = 15                                         # one more N, this near r0's begin


def bait_n_bait():
    """pair_bait with the N runs planted in r0 -> (FASTA text, records, sample)"""
    text, recs, sample = pd.pair_bait()
    r0 = list(recs[0])
    for at, n in BAIT_N_RUNS + ((BAIT_N_EDGE, 1),):
        r0[at:at + n] = "N" * n
    recs = ["".join(r0), recs[1], recs[2]]
    return fasta([("r0", recs[0]), ("r1", recs[1]), ("r2", recs[2])]), recs, sample


def bait_n_targets(k):
    """targets in D of r0 (the sample differs every 20 bases there) whose true candidate covers a run of bait Ns wholly, partly with
    its left or right end, or not at all; reverse targets behind a forward mate 1 in r0's first bases, forward targets in front of a
    reverse mate 1 that ends in r0's last own bases.  what = ("run", strand, start, L, positions of the run the footprint holds).
    And two forward targets over r0's begin with the true insert the window's smallest, so that no other candidate compares more:
    ("edge", inside, compared) with k inside and k - 1 compared (the N at BAIT_N_EDGE is among them), and k + 1 inside, k compared."""
    assert k > BAIT_N_EDGE + 1
    text, recs, sample = bait_n_bait()
    rng = random.Random(13 + k)
    lo, hi = BAIT_N_WINDOW
    seqs1, seqs2, what = [], [], []

    def add(strand, start, L):
        """the target at [start, start + L) of r0 on `strand`"""
        end = start + L
        assert pd.D[0] <= start and end <= pd.D[1]
        if strand == 1:
            a = rng.randint(max(0, end - hi), min(150, end - lo))
            m1, m2 = sample[0][pd.FLANK + a:pd.FLANK + a + 150], revcomp(sample[0][pd.FLANK + start:pd.FLANK + end])
        else:
            e = rng.randint(max(850, start + lo), min(900, start + hi))
            m1, m2 = revcomp(sample[0][pd.FLANK + e - 150:pd.FLANK + e]), sample[0][pd.FLANK + start:pd.FLANK + end]
        held = sum(max(0, min(end, at + n) - max(start, at)) for at, n in BAIT_N_RUNS)
        seqs1.append(m1); seqs2.append(m2); what.append(("run", strand, start, L, held))

    def feasible(strand, start, L):
        """the window reaches the target from a mate 1 in r0's own bases"""
        return lo <= start + L <= 150 + hi if strand == 1 else 850 - hi <= start <= 900 - lo

    for strand in (0, 1):
        for _ in range(3):
            # one run wholly and nothing of the others: 1, 16 and 33 positions
            add(strand, 340 + rng.randint(0, 5), 80) if strand == 1 else add(strand, 390, 40 - rng.randint(0, 4))
            add(strand, rng.randint(417, 420), 58)
            add(strand, rng.randint(448, 452), 90)
            # no run at all
            add(strand, 447, 32) if strand == 0 else add(strand, 512 + rng.randint(0, 6), 80)
        # a footprint that begins or ends inside a run (whatever else it holds)
        for at, n in BAIT_N_RUNS[1:]:
            for L in (80, 97):
                for start in (at + rng.randint(1, n - 1), at + rng.randint(1, n - 1) - L):
                    if feasible(strand, start, L) and start + L <= pd.D[1]:
                        add(strand, start, L)
    for inside in (k, k + 1):
        over = 150 - inside
        e = lo - over                                                             # the true insert is lo: every other candidate holds fewer bases
        m2 = list(sample[0][pd.FLANK - over:pd.FLANK + inside])
        m2[over + 3] = _other(m2[over + 3])
        seqs1.append(revcomp(sample[0][pd.FLANK + e - 150:pd.FLANK + e])); seqs2.append("".join(m2)); what.append(("edge", inside, inside - 1))
    return text, seqs1, seqs2, what


# ------------------------------------------------------------------ the pair counters' LDS limit
MANY_WINDOW = (100, 199)
MANY_KINDS = ("proper", "far", "same_strand", "cross", "rescued", "single")


def many_record_pairs(n_rec, seed=5):
    """pairs of 40 .. 60-base mates over short_record_bait(n_rec, 260): every record holds one pair of a kind that changes from record
    to record, the last six records three more of every kind, and now and then a `light` pair (mate 2 with two substitutions in 60
    bases: proper at a cut of 1000, single -- placed and rejected, never rescued -- at 30) and a `none` pair.  what = (kind, record)"""
    text, recs = sd.short_record_bait(n_rec, 260, 170 + seed)
    rng = random.Random(seed)
    lo, hi = MANY_WINDOW
    seqs1, seqs2, what = [], [], []

    def add(kind, j):
        r = recs[j]
        L1, L2 = rng.randint(40, 60), 60 if kind == "light" else rng.randint(40, 60)
        flip = rng.random() < 0.5
        ins = rng.randint(205, 250) if kind == "far" else rng.randint(lo + 5, hi - 5)
        a = rng.randint(0, len(r) - ins)
        f, b = r[a:a + (L2 if flip else L1)], r[a + ins - (L1 if flip else L2):a + ins]          # the fragment's first and last bases
        m1, m2 = (b, f) if flip else (f, b)                                       # as the record reads
        if kind == "rescued":
            m2 = pd.substituted(m2, 15, 5)
        elif kind == "light":
            m2 = pd.substituted(pd.substituted(m2, 1000, 2), 1000, 57)
        elif kind == "single":
            m2 = _rand(rng, L2)
        elif kind == "cross":
            r2 = recs[(j + 1) % n_rec]
            c = rng.randint(0, len(r2) - L2)
            m2 = r2[c:c + L2]
        rev1, rev2 = flip, not flip
        if kind == "same_strand":
            rev2 = rev1
        seqs1.append(revcomp(m1) if rev1 else m1); seqs2.append(revcomp(m2) if rev2 else m2); what.append((kind, j))

    for j in range(n_rec):
        add(MANY_KINDS[j % len(MANY_KINDS)], j)
        if j % 9 == 4:
            add("light", j)
        if j % 5 == 2:
            seqs1.append(_rand(rng, rng.randint(40, 60))); seqs2.append(_rand(rng, rng.randint(40, 60))); what.append(("none", -1))
    for j in range(n_rec - 6, n_rec):
        for kind in MANY_KINDS:
            for _ in range(3):
                add(kind, j)
    return text, seqs1, seqs2, what


# ------------------------------------------------------------------ more pairs than one turn of the list grid
TURN_WINDOW = (92, 107)


def turn_pool(seed=8, per_kind=16):
    """a pool of distinct 40-base pairs of every kind on pair_bait for k = 21 and TURN_WINDOW: what = the kind each was drawn as"""
    text, recs, sample = pd.pair_bait()
    rng = random.Random(seed)
    lo, hi = TURN_WINDOW
    r0, r2 = recs[0], recs[2]
    seqs1, seqs2, what = [], [], []
    for _ in range(per_kind):
        for kind in ("proper", "far", "same_strand", "cross", "rescued_2", "rescued_1", "single", "none"):
            a, ins = rng.randint(0, 150), rng.randint(lo, hi)
            if kind == "far":
                ins = rng.randint(hi + 5, 140)
            f, b = r0[a:a + 40], r0[a + ins - 40:a + ins]
            if kind == "cross":
                c = rng.randint(0, 250)
                b = r2[c:c + 40]
            elif kind == "single":
                b = _rand(rng, 40)
            elif kind == "none":
                f, b = _rand(rng, 40), _rand(rng, 40)
            elif kind == "rescued_2":
                b = pd.substituted(b, 15, 5)
            elif kind == "rescued_1":
                f = pd.substituted(f, 15, 5)
            m1, m2 = f, (b if kind == "same_strand" else revcomp(b))
            if rng.random() < 0.5 and kind not in ("rescued_1", "rescued_2"):          # the reverse mate first
                m1, m2 = m2, m1
            seqs1.append(m1); seqs2.append(m2); what.append(kind)
    assert len(set(zip(seqs1, seqs2))) == len(seqs1)
    return text, seqs1, seqs2, what


def copies(pool1, pool2, n, seed):
    """-> int64[n]: which pair of the pool pair i of the set is, drawn at random; the last 1100 go through the whole pool in turn, so
    that every kind lies behind any turn that ends before them"""
    assert len(pool1) == len(pool2) and n >= 1100
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, len(pool1), size=n).astype(np.int64)
    idx[n - 1100:] = np.arange(1100) % len(pool1)
    return idx
