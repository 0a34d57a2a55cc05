"""Baits and reads of the banded-alignment tests (test_align_oracle.py, test_align_model.py, test_gpu_align.py): a three-record bait
with Ns, a poly-A stretch and a (TA)n stretch, and reads that carry one simulated indel each at about a third of their length (never in
the middle: equal votes on both sides of an indel make a read ambiguous by placement's rule), beside plain, overhanging, N-bearing and
stacked ones.  Everything is drawn from seeded generators: the same inputs on every run."""
import random

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
