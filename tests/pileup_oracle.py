"""Plain-Python oracle of the pile-up (mf_pileup), written from the semantics in include/mitofilter.h over strings: every base of a
placed read goes to the record coordinate its placement gives it, complemented on strand 1, unless it is an N or hangs over an end of
the record; a position is called when at least min_depth bases lie there and one letter has strictly the most.  Placements come from
tests/place_oracle.PlaceOracle (its place rows); nothing here is shared with the product."""
import numpy as np

from oracle import kmer_bait_ref as kb
from tests import place_oracle as po

CLAMP = 0xFFFFFFFE
LETTERS = "ACGT"
_IDX = {c: i for i, c in enumerate(LETTERS)}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


class PileupOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.bait = "".join(place_oracle.recs)          # one letter per position: A C G T, N for an invalid one
        self.starts = [int(s) for s in place_oracle.starts]

    def pile(self, seqs, rows):
        """-> counts int64[positions, 4] (unclamped, columns A C G T) of the reads seqs placed as rows (PlaceOracle.place()[1])"""
        counts = np.zeros((self.starts[-1], 4), np.int64)
        for seq, row in zip(seqs, rows):
            j = int(row[0])
            if j >= po.AMBIGUOUS:
                continue
            strand, start = int(row[1]), int(row[2])
            s = kb._norm(seq)
            L, len_j = len(s), self.o.lens[j]
            for i, ch in enumerate(s):
                if ch == "N":
                    continue
                c = start + i if strand == 0 else start + (L - 1 - i)
                if not 0 <= c < len_j:
                    continue
                counts[self.starts[j] + c, _IDX[ch if strand == 0 else _COMP[ch]]] += 1
        return counts

    def call(self, counts, min_depth):
        """-> (consensus u8[positions], records u64[R, 6]: bases, matches, mismatches, called, ambiguous, variants)"""
        assert min_depth >= 1
        cons = bytearray(len(self.bait))
        rec = np.zeros((len(self.o.recs), 6), np.int64)
        for j in range(len(self.o.recs)):
            for p in range(self.starts[j], self.starts[j + 1]):
                row = [int(v) for v in counts[p]]
                d, m, ref = sum(row), max(row), self.bait[p]
                rec[j, 0] += d
                if ref != "N":
                    rec[j, 1] += row[_IDX[ref]]
                    rec[j, 2] += d - row[_IDX[ref]]
                if d < min_depth:
                    cons[p] = ord(ref.lower())
                elif row.count(m) == 1:
                    call = LETTERS[row.index(m)]
                    cons[p] = ord(call)
                    rec[j, 3] += 1
                    rec[j, 5] += ref != "N" and ref != call
                else:
                    cons[p] = ord("N")
                    rec[j, 4] += 1
        return np.frombuffer(bytes(cons), np.uint8), rec.astype(np.uint64)

    def call_fast(self, counts, min_depth):
        """call() restated over whole arrays, for baits of a million positions (tests/test_pileup_oracle.py holds it to call()): the same
        results, the records' sums by np.add.reduceat over the starts of the records that are not empty"""
        assert min_depth >= 1
        counts = np.asarray(counts, np.int64)
        n, R = len(self.bait), len(self.o.recs)
        ref = np.frombuffer(self.bait.encode(), np.uint8)
        ref_idx = np.full(n, -1, np.int64)
        for i, c in enumerate(LETTERS):
            ref_idx[ref == ord(c)] = i
        valid = ref_idx >= 0
        d, m = counts.sum(axis=1), counts.max(axis=1)
        best = counts.argmax(axis=1)                                     # the first letter that holds the maximum: row.index(m)
        alone = (counts == m[:, None]).sum(axis=1) == 1
        own = np.where(valid, counts[np.arange(n), np.maximum(ref_idx, 0)], 0)
        deep = d >= min_depth
        called, tied = deep & alone, deep & ~alone
        cons = np.where(called, np.frombuffer(LETTERS.encode(), np.uint8)[best], np.where(tied, ord("N"), ref | 0x20)).astype(np.uint8)
        cols = (d, own, np.where(valid, d - own, 0), called, tied, called & valid & (best != ref_idx))
        starts = np.asarray(self.starts, np.int64)
        full = starts[1:] > starts[:-1]
        rec = np.zeros((R, 6), np.int64)
        if full.any():
            for c, col in enumerate(cols):
                rec[full, c] = np.add.reduceat(col.astype(np.int64), starts[:-1][full])
        return cons, rec.astype(np.uint64)

    def variants(self, counts, consensus):
        """-> [(record, 0-based position inside the record, ref, alt, depth, alt count)]"""
        out = []
        for j in range(len(self.o.recs)):
            for p in range(self.starts[j], self.starts[j + 1]):
                alt, ref = chr(consensus[p]), self.bait[p]
                if alt in LETTERS and ref != "N" and alt != ref:
                    out.append((j, p - self.starts[j], ref, alt, int(counts[p].sum()), int(counts[p, _IDX[alt]])))
        return out


def clamped(counts):
    return np.minimum(counts, CLAMP)
