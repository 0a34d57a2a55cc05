"""What the tests of pair-aware placement share (test_pair_data.py, test_gpu_pairs.py): a bait of three records and a paired sample drawn
so that every pair kind and every way a rescue is refused occurs, by construction and -- checked in test_pair_data.py with the oracle
alone -- in fact.

The bait.  r0 (900 bases): 300 of its own, the 300-base stretch D, a 200-base stretch it shares letter for letter with r1, 100 of its
own.  r1 (650): 150 of its own, the shared stretch, 300 of its own.  r2 (820): 300 of its own, a 60-base unit twice in a row -- the first
copy with its first base substituted --, 400 of its own.  Reads inside the shared stretch or inside the unit have no anchor window.
The sample is the bait with 200 bases of flank on either side of every record and, along D, another letter every 20 bases: a read
there shares no 21-mer with the bait.
Mate 1 is always 150 bases; mate 2 has 40 .. 151 bases and now and then an N (every b0 mod 16, the offsets path).  The insert window the
tests use is WINDOW."""
import random

from tests.report_data import fasta
from tests.util_data import revcomp

WINDOW = (250, 350)
FLANK = 200
D = (300, 600)
UNIT_AT, UNIT = 300, 60


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def substituted(s, every, first):
    t = list(s)
    for i in range(first, len(t), every):
        t[i] = "CGTA"["ACGT".index(t[i])]
    return "".join(t)


def pair_bait(seed=20):
    """-> (FASTA text, the three records, the three sample records with their flanks)"""
    rng = random.Random(seed)
    shared, unit = _rand(rng, 200), _rand(rng, UNIT)
    r0 = _rand(rng, 300) + _rand(rng, 300) + shared + _rand(rng, 100)
    r1 = _rand(rng, 150) + shared + _rand(rng, 300)
    r2 = _rand(rng, 300) + substituted(unit, 1000, 0) + unit + _rand(rng, 400)
    recs = [r0, r1, r2]
    s0 = r0[:D[0]] + substituted(r0[D[0]:D[1]], 20, 7) + r0[D[1]:]
    sample = [_rand(rng, FLANK) + s + _rand(rng, FLANK) for s in (s0, r1, r2)]
    return fasta([("r0", r0), ("r1", r1), ("r2", r2)]), recs, sample


def _fragment(sample, j, begin, end):
    """bases [begin, end) of record j's coordinates out of its sample (the flanks give what lies outside the record)"""
    return sample[j][FLANK + begin:FLANK + end]


def pair_set(seed=3, per_kind=26):
    """-> (seqs1, seqs2, what): `what` names how each pair was drawn.  A pair is a fragment [a, a + ins) of one sample record: the
    forward mate is its first bases, the reverse mate the reverse complement of its last; `flip` says mate 1 is the reverse one."""
    text, recs, sample = pair_bait()
    rng = random.Random(seed)
    seqs1, seqs2, what = [], [], []
    lo, hi = WINDOW

    def len2(most=151, least=40):
        return rng.randint(least, most)

    def add(name, j, a, ins, flip, L2, change2=None, same_strand=False, change1=None):
        L1 = 150
        if not flip:
            m1 = _fragment(sample, j, a, a + L1)
            m2 = _fragment(sample, j, a + ins - L2, a + ins)
            m2 = change2(m2) if change2 else m2
            m2 = m2 if same_strand else revcomp(m2)
        else:
            m1 = _fragment(sample, j, a + ins - L1, a + ins)
            m1 = revcomp(change1(m1) if change1 else m1)
            m2 = _fragment(sample, j, a, a + L2)
            m2 = change2(m2) if change2 else m2
            m2 = revcomp(m2) if same_strand else m2
        if rng.random() < 0.15 and L2 > 45:
            i = rng.randrange(L2)
            m2 = m2[:i] + "N" + m2[i + 1:]
        seqs1.append(m1)
        seqs2.append(m2)
        what.append(name)

    for _ in range(per_kind):
        # both mates in their record's own bases
        add("proper", 1, rng.randint(350, 360), rng.randint(lo + 10, 290), False, len2())
        add("proper", 2, rng.randint(440, 470), rng.randint(lo + 10, hi - 10), True, len2())
        add("far", 2, rng.randint(420, 430), rng.randint(hi + 10, 390), rng.random() < 0.5, len2())
        add("same_strand", 2, rng.randint(430, 450), rng.randint(lo + 10, hi - 10), False, len2(), same_strand=True)
        # mates from different records
        seqs1.append(_fragment(sample, 0, 20, 170)); seqs2.append(revcomp(_fragment(sample, 1, 400, 400 + len2()))); what.append("cross")
        seqs1.append(_rand(rng, 150)); seqs2.append(_rand(rng, len2())); what.append("none")
        # one mate in the diverged stretch: mate 2 behind a forward mate 1, mate 1 (reverse) behind a forward mate 2
        add("diverged_2", 0, rng.randint(135, 150), rng.randint(325, 340), False, len2())
        add("diverged_1", 0, rng.randint(100, 140), rng.randint(335, 345), True, len2())
        # a mate that differs every 8 bases: beyond a cut of 100
        add("heavy", 0, rng.randint(135, 150), rng.randint(325, 340), False, len2(), change2=lambda s: substituted(s, 8, 3))
        add("heavy_1", 0, rng.randint(100, 140), rng.randint(335, 345), True, len2(), change1=lambda s: substituted(s, 8, 3))
        # a mate that differs every 28 bases: placed by the vote at k = 21 and rejected at 30 permille (never rescued), a target above
        add("light", 2, rng.randint(440, 470), rng.randint(lo + 10, hi - 10), False, len2(most=151, least=120), change2=lambda s: substituted(s, 28, 5))
        # mate 1 inside the stretch r0 shares with r1 (it passes and is ambiguous); mate 2 in r0's last bases says which copy
        a = rng.randint(605, 640)
        add("shared", 0, a, 900 - a - rng.randint(0, 5), False, len2(most=95))
        # mate 2 inside the unit's two copies: the candidates 60 apart tie -- except from the first copy's first base on, where the bait's
        # substitution and one of the mate's own in its second base leave the second copy the better one
        L2 = len2(most=50)
        x = rng.randint(1, UNIT - L2)
        ins = 270 - rng.randint(0, 15)
        add("tandem", 2, UNIT_AT + x + L2 - ins, ins, False, L2)
        seqs1.append(seqs1[-1])
        seqs2.append(revcomp(substituted(recs[2][UNIT_AT + UNIT:UNIT_AT + UNIT + L2], 1000, 1)))
        what.append("tandem_first_base")
        # mate 1 hangs over r1's end, mate 2 lies in the flank: no candidate compares a base
        a = 650 - rng.randint(60, 100)
        add("beyond", 1, a, rng.randint(lo + 10, 650 + FLANK - a), False, len2())
        # a diverged mate 2 that hangs over r1's end / over r0's begin
        over = rng.randint(5, 45)
        ins = rng.randint(lo + 10, hi - 50)
        add("over_end", 1, 650 + over - ins, ins, False, len2(most=151, least=100), change2=lambda s: substituted(s, 20, 9))
        add("over_begin", 0, -over, rng.randint(lo + 10, 290), True, len2(most=151, least=100), change2=lambda s: substituted(s, 20, 9))
    return seqs1, seqs2, what


def neighbour_pairs(k):
    """mates that lie across the border of r0 and r1 in global positions, each behind a forward mate 1 on r0.  Mate 2 differs from the
    bait often enough (once in the middle of a short stretch inside r0, else every 20 bases) that the vote places it on neither record; `inside` of its 150 bases lie in r0: k - 1 (no candidate
    is admissible), k, k + 9 and 100 (rescued, clipped at r0's end).  -> (seqs1, seqs2, inside)"""
    text, recs, sample = pair_bait()
    r0, r1 = recs[0], recs[1]
    seqs1, seqs2, inside = [], [], []
    for n_in in (k - 1, k, k + 9, 100):
        own = r0[900 - n_in:]
        m2 = (substituted(own, 1000, n_in // 2) if n_in < 60 else substituted(own, 20, 10)) + substituted(r1[:150 - n_in], 20, 5)
        end = 900 + (150 - n_in)
        a = min(740, end - 260)
        seqs1.append(r0[a:a + 150])
        seqs2.append(revcomp(m2))
        inside.append(n_in)
    return seqs1, seqs2, inside
