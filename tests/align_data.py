"""Baits and reads of the banded-alignment tests (test_align_oracle.py, test_align_model.py, test_gpu_align.py and, with the builders at
the end, test_align_data.py, test_gpu_align_waves.py, test_gpu_align_files.py): a three-record bait
with Ns, a poly-A stretch and a (TA)n stretch, and reads that carry one simulated indel each at about a third of their length (never in
the middle: equal votes on both sides of an indel make a read ambiguous by placement's rule), beside plain, overhanging, N-bearing and
stacked ones.  Everything is drawn from seeded generators: the same inputs on every run."""
import random

import numpy as np

from tests.report_data import fasta, mutate
from tests.util_data import revcomp

POLY_A, TA_N = "A" * 14, "TA" * 12


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def align_bait():
    """-> (FASTA text, {name: sequence}): g 3000 random positions; rep 1200 with a poly-A stretch at 300, a (TA)n stretch at 514 and
    three Ns at 700; short 400"""
    rng = random.Random(4242)
    rep = _rand(rng, 300) + POLY_A + _rand(rng, 200) + TA_N + _rand(rng, 162) + "NNN" + _rand(rng, 497)
    parts = {"g": _rand(rng, 3000), "rep": rep, "short": _rand(rng, 400)}
    assert len(rep) == 1200 and rep[300:314] == POLY_A and rep[514:538] == TA_N and rep[700:703] == "NNN"
    return fasta(list(parts.items())), parts


def with_indel(rng, s, at, g, insert):
    """s with g bases inserted (random ones) or deleted at offset `at`"""
    return s[:at] + _rand(rng, g) + s[at:] if insert else s[:at] + s[at + g:]


def _strand(rng, s):
    return s if rng.random() < 0.5 else revcomp(s)


def indel_reads(parts, n, seed, lo=100, hi=250, max_g=8, names=("g", "short")):
    """n reads that are a bait stretch with one indel of 1 .. max_g bases at about a third of the read and no other difference, from
    both strands -> (reads, their g)"""
    rng = random.Random(seed)
    out, gs = [], []
    for _ in range(n):
        rec = parts[rng.choice(names)]
        L = rng.randint(lo, min(hi, len(rec) - 20))
        a = rng.randrange(0, len(rec) - L - 10)
        g = rng.randint(1, max_g)
        at = L // 3 + rng.randint(-5, 5) if rng.random() < 0.5 else L - L // 3 + rng.randint(-5, 5)
        s = with_indel(rng, rec[a:a + L + 10], at, g, rng.random() < 0.5)[:L]
        out.append(_strand(rng, s))
        gs.append(g)
    return out, gs


def ragged_reads(parts, seed=7):
    """The ragged read set of the parity tests -> (reads, {group: (first, last + 1)})"""
    rng = random.Random(seed)
    seqs, groups = [], {}

    def group(name, reads):
        groups[name] = (len(seqs), len(seqs) + len(reads))
        seqs.extend(reads)

    plain = []
    for i in range(700):                                            # lengths 40 .. 300, 1 % substitutions
        rec = parts[rng.choice(("g", "g", "rep", "short"))]
        L = rng.randint(40, 300)
        a = rng.randrange(0, len(rec) - L + 1)
        plain.append(_strand(rng, mutate(rec[a:a + L], 0.01, 1000 + i)))
    group("plain", plain)
    group("indel", indel_reads(parts, 500, seed + 1)[0])
    over = []
    for name in ("g", "rep", "short"):                              # over the begin and the end of every record, the first and last included
        rec = parts[name]
        for _ in range(10):
            junk, L = rng.randint(5, 40), rng.randint(90, 160)
            over.append(_strand(rng, _rand(rng, junk) + rec[:L - junk]))
            over.append(_strand(rng, rec[len(rec) - (L - junk):] + _rand(rng, junk)))
            # ... and with a deletion near the record's end, which the band can turn into an overhang
            over.append(_strand(rng, with_indel(rng, rec[:L], 12, 3, False)))
            over.append(_strand(rng, with_indel(rng, rec[len(rec) - L:], L - 15, 3, True)))
    group("over", over)
    ns = []
    for i in range(60):                                             # reads with Ns, half of them with an indel too
        rec = parts["g"]
        L = rng.randint(80, 200)
        a = rng.randrange(0, len(rec) - L - 10)
        s = list(with_indel(rng, rec[a:a + L + 10], L // 3, rng.randint(1, 6), rng.random() < 0.5)[:L] if i % 2 else rec[a:a + L])
        for p in rng.sample(range(L), rng.randint(1, 3)):
            s[p] = "N"
        ns.append(_strand(rng, "".join(s)))
    for a in (640, 660, 690):                                       # ... and over the bait's own Ns
        ns.append(parts["rep"][a:a + 120])
        ns.append(revcomp(with_indel(rng, parts["rep"][a:a + 130], 40 if a < 680 else 25, 2, False)[:120]))
    group("ns", ns)
    rep, reps = parts["rep"], []
    for _ in range(20):                                             # one A, one TA, more or fewer, with the repeat at a third of the read
        L = rng.randint(120, 200)
        for at, unit in ((300, "A"), (514, "TA")):
            a = at - L // 3
            s = rep[a:a + L + 4]
            for more in (False, True):
                t = s[:at - a] + unit + s[at - a:] if more else s[:at - a] + s[at - a + len(unit):]
                reps.append(_strand(rng, t[:L]))
    group("repeat", reps)
    ends = []
    for _ in range(40):                                             # an indel a few bases from either end of the read
        rec = parts["g"]
        L = rng.randint(100, 180)
        a = rng.randrange(0, len(rec) - L - 10)
        near = rng.randint(2, 9)
        ends.append(_strand(rng, with_indel(rng, rec[a:a + L + 10], near if rng.random() < 0.5 else L - near, rng.randint(1, 4), rng.random() < 0.5)[:L]))
    group("ends", ends)
    group("stack", [with_indel(rng, parts["g"][1000:1160], 50, 3, False)] * 500)
    group("long", [with_indel(rng, parts["g"][400:2410], 650, 5, False)[:2000]])
    return seqs, groups


def uniform_reads(parts, L, n, seed):
    """n reads of exactly L bases: two plain ones to every one with an indel (of at most L // 12 bases, where L allows one)"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        rec = parts[rng.choice(("g", "rep", "short"))]
        a = rng.randrange(0, len(rec) - L - 10)
        g = min(rng.randint(1, 8), L // 12)
        if i % 3 == 2 and g:
            s = with_indel(rng, rec[a:a + L + 10], L // 3, g, rng.random() < 0.5)[:L]
        else:
            s = mutate(rec[a:a + L], 0.01, seed + i)
        out.append(_strand(rng, s))
    return out


# ------------------------------------------------------------------ several reads a wave, the capped launch, the files
# (tests/test_align_data.py holds what these give to their conditions, from the oracle alone)
def distinct_reads(parts, seed=11):
    """About 400 different reads of 40 .. 300 bases (and one shorter than any k) from all three records and both strands: every kind of
    ragged_reads but the stack and the long one, reads of a copy that differs at 6 % (the cut rejects them), reads of two equal halves
    from two places (they pass, and placement leaves them ambiguous), random reads -> (reads, {group: (first, last + 1)})"""
    rng = random.Random(seed)
    seqs, groups = [], {}

    def group(name, reads):
        groups[name] = (len(seqs), len(seqs) + len(reads))
        seqs.extend(reads)

    names = ("g", "rep", "short")
    plain = []
    for i in range(120):
        rec = parts[names[i % 3]]
        L = rng.randint(40, 300)
        a = rng.randrange(0, len(rec) - L + 1)
        plain.append(_strand(rng, mutate(rec[a:a + L], 0.01, 5000 + i)))
    group("plain", plain)
    group("indel", indel_reads(parts, 100, seed + 1)[0] + indel_reads(parts, 20, seed + 2, names=("rep",))[0])
    over = []
    for name in names:
        rec = parts[name]
        for _ in range(3):
            junk, L = rng.randint(5, 40), rng.randint(90, 160)
            over.append(_strand(rng, _rand(rng, junk) + rec[:L - junk]))
            over.append(_strand(rng, rec[len(rec) - (L - junk):] + _rand(rng, junk)))
            over.append(_strand(rng, with_indel(rng, rec[:L], 12, 3, False)))
            over.append(_strand(rng, with_indel(rng, rec[len(rec) - L:], L - 15, 3, True)))
    group("over", over)
    ns = []
    for i in range(20):
        rec = parts["g"]
        L = rng.randint(80, 200)
        a = rng.randrange(0, len(rec) - L - 10)
        s = list(with_indel(rng, rec[a:a + L + 10], L // 3, rng.randint(1, 6), rng.random() < 0.5)[:L] if i % 2 else rec[a:a + L])
        for p in rng.sample(range(L), rng.randint(1, 3)):
            s[p] = "N"
        ns.append(_strand(rng, "".join(s)))
    for a in (640, 660, 690):
        ns.append(parts["rep"][a:a + 120])
        ns.append(revcomp(with_indel(rng, parts["rep"][a:a + 130], 40 if a < 680 else 25, 2, False)[:120]))
    group("ns", ns)
    rep, reps = parts["rep"], []
    for _ in range(5):
        L = rng.randint(120, 200)
        for at, unit in ((300, "A"), (514, "TA")):
            a = at - L // 3
            s = rep[a:a + L + 4]
            for more in (False, True):
                t = s[:at - a] + unit + s[at - a:] if more else s[:at - a] + s[at - a + len(unit):]
                reps.append(_strand(rng, t[:L]))
    group("repeat", reps)
    far = []
    for i in range(36):                                             # 6 % substitutions: placed by a clean window or two, and far above any cut in use
        rec = parts[names[i % 3]]
        L = rng.randint(200, 300)
        a = rng.randrange(0, len(rec) - L + 1)
        far.append(_strand(rng, mutate(rec[a:a + L], 0.06, 6000 + i)))
    group("far", far)
    ties = []
    for i in range(16):                                             # two halves of one length from two places: as many votes for either
        h = rng.randint(45, 149)
        r1, r2 = parts[names[i % 3]], parts[names[(i + 1 + i // 3) % 3]]
        a, b = rng.randrange(0, len(r1) - h + 1), rng.randrange(0, len(r2) - h + 1)
        ties.append(_strand(rng, r1[a:a + h] + "N" + (r2[b:b + h] if i % 2 else revcomp(r2[b:b + h]))))
    group("tie", ties)
    group("random", [_rand(rng, rng.randint(40, 300)) for _ in range(14)] + [parts["g"][500:518]])
    return seqs, groups


def tiled_reads(distinct, copies, seed):
    """Every read of `distinct` copies times over in a seeded shuffle -> (reads, index of every read in `distinct`).  The device's list of
    passing reads is not ordered, so no neighbour can be planned: the shuffle gives every wave reads of different kind, length and record"""
    index = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(distinct)), copies))
    return [distinct[i] for i in index], index


def long_read(parts, flank=13500, seed=17):
    """Record g without the four bases from 1000 and with three more at 2200, between random flanks of `flank` bases: with the default
    29 999 bases, almost all of them overhang"""
    rng = random.Random(seed)
    g = parts["g"]
    return _rand(rng, flank) + g[:1000] + g[1004:2200] + _rand(rng, 3) + g[2200:] + _rand(rng, flank)


def capped_reads(parts):
    """ragged_reads with long_read in the middle -> (reads, the long read's index): mf_align.hip's work memory then allows 372 waves"""
    seqs, _ = ragged_reads(parts)
    at = len(seqs) // 2
    return seqs[:at] + [long_read(parts)] + seqs[at:], at


# what test_gpu_align_waves.py tiles: copies of distinct_reads, the cut; length, number, seed and copies of the uniform set
TILE_COPIES, TILE_CUT = 88, 40
UNIFORM_LEN, UNIFORM_DISTINCT, UNIFORM_SEED, UNIFORM_COPIES = 100, 300, 200, 96


def uniform_distinct(parts):
    """The distinct reads of the uniform tile: uniform_reads, whose indels lie at a third of the read -- placement goes by the longer part
    behind it, so every path ends on the winning diagonal with diagonal moves alone --, and 60 reads of the same length with the indel at
    two thirds, whose paths end off it"""
    L = UNIFORM_LEN
    rng = random.Random(UNIFORM_SEED + 1)
    late = []
    for i in range(60):
        rec = parts[("g", "rep", "short")[i % 3]]
        a = rng.randrange(0, len(rec) - L - 10)
        late.append(_strand(rng, with_indel(rng, rec[a:a + L + 10], L - L // 3 + rng.randint(-3, 3), rng.randint(1, 6), i % 2 == 0)[:L]))
    return uniform_reads(parts, L, UNIFORM_DISTINCT, seed=UNIFORM_SEED) + late
# the batch, band and cut of test_gpu_align_files.py
FILE_BATCH, FILE_BAND, FILE_CUT = 300, 8, 30


def align_mates(parts, seed=23):
    """The two mates of the file tests, from the groups of ragged_reads -- every other read of a group to a mate, 170 of the stack --, the
    ambiguous reads of distinct_reads, which the two placing keep modes differ on, and 22 random reads each, shuffled mate by mate, so that
    the indel reads lie all over the file and the reads that are not written meet ones that are; the 2 000-base read stands in mate 1 behind the first two batches -> (mate 1, mate 2, the long read's index)"""
    seqs, groups = ragged_reads(parts)
    others, kinds = distinct_reads(parts)
    ties = others[kinds["tie"][0]:kinds["tie"][1]]
    rng = random.Random(seed)
    mates = []
    for m in (0, 1):
        reads = []
        for name, (lo, hi) in groups.items():
            if name != "long":
                reads += seqs[lo:lo + 340 if name == "stack" else hi][m::2]
        reads += ties[m::2] + [_rand(rng, rng.randint(40, 300)) for _ in range(22)]
        rng.shuffle(reads)
        mates.append(reads)
    at = 2 * FILE_BATCH + 50
    mates[0].insert(at, seqs[groups["long"][0]])
    mates[1].insert(at, seqs[groups["plain"][0] + 1])
    return mates[0], mates[1], at
