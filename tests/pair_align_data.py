"""What the tests of pairs with a band share (test_pair_align_data.py, test_gpu_pair_align.py): a bait of three records and a paired
sample drawn so that every class of rescued mate the aligning rescue treats differently, every pair kind, every way a rescue is refused
and the pairs that only the aligned cut settles occur -- by construction and, checked in test_pair_align_data.py with the oracle alone,
in fact (a planted substitution can turn a neighbouring copy's k-mers into anchors: what a read claims is what the oracle says of it).

The bait.  r0 (900 bases) and r1 (650) are their own random bases; r2 (820) holds a 30-base unit twice in a row at UNIT_AT.  The sample
is the bait with FLANK random bases on either side of every record.  A pair is a fragment [a, a + ins) of one sample record: the forward
mate is its first bases, the reverse mate the reverse complement of its last.  One mate, the ANCHOR, is 150 clean bases of the record;
the other, the TARGET, is what the class says.  A diverged target differs from the sample every 20 bases: it shares no 21-mer with the
bait, the vote cannot place it and only the rescue finds it.

WINDOW is the insert window, RESCUE_PERMILLE the rescue's cut: 250 lets a 3-base indel 25 .. 30 bases from the end of a diverged
150-base mate through -- the 120 bases on the seed's diagonal carry about 6 mismatches, the 30 shifted ones about 22."""
import random

from tests.pair_data import _rand, substituted
from tests.report_data import fasta
from tests.util_data import revcomp

WINDOW = (270, 333)
RESCUE_PERMILLE = 250
FLANK = 200
UNIT_AT, UNIT = 300, 30
RESCUED = ("ins", "del", "over_begin", "over_end", "n")
CLASSES = RESCUED + ("proper", "far", "cross", "none", "cut", "tie", "short", "indel_placed")


def bait(seed=41):
    """-> (FASTA text, the three records, the three sample records with their flanks)"""
    rng = random.Random(seed)
    unit = _rand(rng, UNIT)
    recs = [_rand(rng, 900), _rand(rng, 650), _rand(rng, 300) + unit + unit + _rand(rng, 460)]
    sample = [_rand(rng, FLANK) + r + _rand(rng, FLANK) for r in recs]
    return fasta([("r0", recs[0]), ("r1", recs[1]), ("r2", recs[2])]), recs, sample


def inserted(s, at, rng, n=3):
    """n bases more behind offset `at`; the mate keeps its length and its first base"""
    return (s[:at] + _rand(rng, n) + s[at:])[:len(s)]


def pair_set(seed=5, per_combo=7, mixed=False):
    """-> (seqs1, seqs2, what): what[i] = (class, target set 1 or 2, target strand 0 or 1).  Every class is drawn per_combo times for each of
    the four (target set, target strand) combinations.  mixed=False: the anchor is always mate 1 (a uniform set of 150-base reads, and a
    ragged set); `what` still says which set the target WOULD be in, so both forms hold the same pairs in the same order."""
    text, recs, sample = bait()
    rng = random.Random(seed)
    lo, hi = WINDOW
    seqs1, seqs2, what = [], [], []

    def frag(j, b, e):
        assert -FLANK <= b <= e <= len(recs[j]) + FLANK
        return sample[j][FLANK + b:FLANK + e]

    def put(name, tset, fwd, anchor, target):
        a, t = (anchor, target) if (tset == 2 or not mixed) else (target, anchor)
        seqs1.append(a); seqs2.append(t); what.append((name, tset, 0 if fwd else 1))

    def add(name, tset, fwd, j, a, ins, L, change=None, L_anchor=150):
        """the pair of fragment [a, a + ins) of record j whose target of L bases is the forward mate (fwd) or the reverse one"""
        if fwd:
            t, anchor = frag(j, a, a + L), revcomp(frag(j, a + ins - L_anchor, a + ins))
        else:
            t, anchor = frag(j, a + ins - L, a + ins), frag(j, a, a + L_anchor)
        t = change(t) if change else t
        put(name, tset, fwd, anchor, t if fwd else revcomp(t))

    def diverged(s):
        return substituted(s, 20, rng.randrange(20))

    def near_end(L):
        return rng.randint(25, 30) if rng.random() < 0.5 else L - rng.randint(25, 30)

    for tset in (1, 2):
        for fwd in (True, False):
            for _ in range(per_combo):
                L = rng.randint(120, 151)
                j = rng.randrange(3)
                n = len(recs[j])
                a = rng.randint(20, n - 360) if j < 2 else rng.randint(440, n - 350)          # (r2: clear of the unit)
                ins = rng.randint(lo + 8, hi - 8)
                at = near_end(L)
                add("ins", tset, fwd, j, a, ins, L, lambda s: diverged(inserted(s, at, rng)))
                add("del", tset, fwd, j, a, ins, L, lambda s: diverged(s[:at] + s[at + 2:]))
                add("n", tset, fwd, j, a, ins, L, lambda s: (lambda t: t[:at] + "N" + t[at + 1:])(diverged(s)))
                add("proper", tset, fwd, j, a, ins, L)
                add("far", tset, fwd, j, a, hi + rng.randint(5, 20), L)
                add("cut", tset, fwd, j, a, ins, L, lambda s: substituted(s, 3, 1))
                add("indel_placed", tset, fwd, j, a, ins, 150, lambda s: s[:50] + s[53:] if rng.random() < 0.5 else inserted(s, 100, rng, 2))
                # the target hangs over the record's begin (a forward one) or end (a reverse one) by 5 .. 45 bases; on the other strand it
                # can only do so when it is longer than the insert
                over = rng.randint(5, 45)
                jj = rng.randrange(2)
                nn = len(recs[jj])
                if fwd:
                    add("over_begin", tset, True, jj, -over, ins, L, diverged)
                    b = nn - ins - rng.randint(0, 20)
                    add("over_end", tset, True, jj, b, ins, nn + over - b, diverged)
                else:
                    b = rng.randint(0, 20)
                    add("over_begin", tset, False, jj, b, ins, ins + over + b, diverged)
                    add("over_end", tset, False, jj, nn + over - ins, ins, L, diverged)
                # the anchor at the record's end and the target in the flank beyond it: no candidate compares k bases
                if fwd:
                    e, d = rng.randint(150, 185), rng.randint(lo, hi)
                    add("short", tset, True, jj, e - d, d, 100, diverged)
                else:
                    add("short", tset, False, jj, nn - 150 - rng.randint(0, 10), hi - rng.randint(0, 10), 100, diverged)
                # the target inside the first copy of r2's unit: the candidates UNIT apart tie
                Lt = rng.randint(22, UNIT - 2)
                x = rng.randint(0, UNIT - Lt)
                if fwd:
                    add("tie", tset, True, 2, UNIT_AT + x, rng.randint(lo + UNIT + 2, hi - 2), Lt)
                else:
                    d = rng.randint(lo + 2, hi - UNIT - 2)
                    add("tie", tset, False, 2, UNIT_AT + x + Lt - d, d, Lt)
                put("cross", tset, fwd, frag(0, 30, 180), revcomp(frag(1, 300, 300 + L)))
                put("none", tset, fwd, _rand(rng, 150), _rand(rng, L))
    return seqs1, seqs2, what
