"""Plain-Python oracle of the gapped consensus (mf_align_gapped), written from the rule in include/mitofilter.h: the insertion pile from
the steps of tests/align_oracle.AlignOracle.align_row, and the call from that oracle's unclamped depth, indel table and counts and from
PileupOracle.call's consensus.  Nothing here is shared with the product."""
import numpy as np

from tests import align_oracle as ao
from tests import pileup_oracle as pio

LETTERS = "ACGT"
_IDX = {c: i for i, c in enumerate(LETTERS)}


def pile_steps(pile, x, steps, s0, ln, span):
    """What one accepted read adds to pile (int64[positions, span, 4]): the t-th base of a maximal run of insertion steps at column c, t
    from 0 in the order of the oriented read x, at [s0 + c - 1, t, letter] when 0 <= c - 1 < ln; an N takes its offset and adds nowhere"""
    prev, t = None, 0
    for mv, bi, c in steps:
        if mv != ao.INS:
            prev = None
            continue
        t = t + 1 if prev == c else 0
        prev = c
        assert t < span, "a run of insertions is never longer than 2 * band"
        if 0 <= c - 1 < ln and x[bi] != "N":
            pile[s0 + c - 1, t, _IDX[x[bi]]] += 1


def call(starts, depth, dels, consensus, pile, min_depth):
    """The call from unclamped sums: depth int[positions], dels int[positions], consensus bytes[positions], pile int[positions, span, 4].
    -> (gapped bytes, gapped_starts [R + 1], records [R][length, deleted, insertions, inserted_bases])"""
    assert min_depth >= 1
    span = pile.shape[1]
    out, gstarts, recs = bytearray(), [], []
    for j in range(len(starts) - 1):
        gstarts.append(len(out))
        deleted = insertions = inserted = 0
        for p in range(int(starts[j]), int(starts[j + 1])):
            D = int(depth[p])
            deep = D >= min_depth
            if span and deep and 2 * int(dels[p]) > D:
                deleted += 1
            else:
                out.append(consensus[p])
            cols = 0
            for q in range(span):
                row = [int(v) for v in pile[p, q]]
                if not (deep and 2 * sum(row) > D):
                    break
                m = max(row)
                out.append(ord(LETTERS[row.index(m)]) if row.count(m) == 1 else ord("N"))
                cols += 1
            insertions += cols > 0
            inserted += cols
        recs.append([len(out) - gstarts[j], deleted, insertions, inserted])
    gstarts.append(len(out))
    return bytes(out), gstarts, recs


class GappedOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.A = ao.AlignOracle(place_oracle)
        self.P = pio.PileupOracle(place_oracle)

    def pile(self, seqs, want, W):
        """-> the insertion pile int64[positions, 2 W, 4] of the reads that AlignOracle.run accepted (want: what it gave)"""
        o = self.o
        pile = np.zeros((int(o.starts[-1]), 2 * W, 4), np.int64)
        for seq, row, ok in zip(seqs, want["rows"], want["accepted"]):
            if not ok:
                continue
            j = int(row[0])
            a = self.A.align_row(seq, row, W)
            pile_steps(pile, self.A.oriented(seq, int(row[1])), a["steps"], int(o.starts[j]), o.lens[j], 2 * W)
        return pile

    def call(self, want, pile, min_depth):
        """the call from the sums of one or more runs: want holds depth, indels, counts (AlignOracle.run's, or their sums)"""
        cons, _ = self.P.call(want["counts"], min_depth)
        return call([int(s) for s in self.o.starts], want["depth"], want["indels"][:, 0], bytes(cons), pile, min_depth)

    def run(self, seqs, tallies, thr, max_permille, W, min_depth):
        """AlignOracle.run plus ins_pile int64[positions, 2 W, 4], gapped bytes, gapped_starts and gapped_records"""
        want = self.A.run(seqs, tallies, thr, max_permille, W)
        want["ins_pile"] = self.pile(seqs, want, W)
        want["gapped"], want["gapped_starts"], want["gapped_records"] = self.call(want, want["ins_pile"], min_depth)
        return want


def clamped(pile):
    return np.minimum(pile, pio.CLAMP)
