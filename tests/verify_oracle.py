"""Plain-Python oracle of the verification of placed reads (mf_verify), written from the semantics in include/mitofilter.h over strings:
every base of a placed read that lies inside its record, is a valid letter and lies on a valid bait letter is compared with that letter
(complemented on strand 1); the read is accepted iff mismatches * 1000 <= max_permille * compared; a rejected read counts nowhere but
in its record's `rejected` and in the histogram.  Placements come from tests/place_oracle.PlaceOracle (its place rows), the pile-up and
the calls from tests/pileup_oracle.PileupOracle; nothing here is shared with the product."""
import numpy as np

from oracle import kmer_bait_ref as kb
from tests import pileup_oracle as pio
from tests import place_oracle as po

BINS = 32
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def accepts(compared, mismatches, max_permille):
    return mismatches * 1000 <= max_permille * compared


class VerifyOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.P = pio.PileupOracle(place_oracle)

    def score(self, seq, row):
        """-> (compared, mismatches) of one read placed as row (a PlaceOracle place row); (0, 0) when it is not placed"""
        j = int(row[0])
        if j >= po.AMBIGUOUS:
            return 0, 0
        strand, start = int(row[1]), int(row[2])
        s, rec = kb._norm(seq), self.o.recs[j]
        L = len(s)
        compared = mismatches = 0
        for i, ch in enumerate(s):
            c = start + i if strand == 0 else start + (L - 1 - i)
            if ch == "N" or not 0 <= c < len(rec) or rec[c] == "N":
                continue
            compared += 1
            mismatches += (ch if strand == 0 else _COMP[ch]) != rec[c]
        return compared, mismatches

    def verify(self, seqs, tallies, thr, max_permille):
        """-> dict: passes bool[n], rows int64[n, 6] (every placed read keeps its row), scores int64[n, 2], accepted bool[n], depth
        int64[positions] unclamped, place_rec u64[R, 6], score_rec u64[R, 4 + BINS], unplaced [2], counts int64[positions, 4]"""
        assert 0 <= max_permille <= 1000
        o = self.o
        passes, rows, _, _, unplaced = o.place(tallies, thr)
        n, R = len(seqs), len(o.recs)
        scores = np.zeros((n, 2), np.int64)
        accepted = np.zeros(n, bool)
        srec = np.zeros((R, 4 + BINS), np.int64)
        prec = np.zeros((R, 6), np.int64)
        depth = np.zeros(int(o.starts[-1]), np.int64)
        for i, (seq, row) in enumerate(zip(seqs, rows)):
            j = int(row[0])
            if j >= po.AMBIGUOUS:
                continue
            c, m = self.score(seq, row)
            assert c >= o.k and m <= c - o.k
            scores[i] = (c, m)
            srec[j, 4 + min(m, BINS - 1)] += 1
            if not accepts(c, m, max_permille):
                srec[j, 1] += 1
                continue
            accepted[i] = True
            srec[j, 0] += 1
            srec[j, 2] += c
            srec[j, 3] += m
            strand, start, end = int(row[1]), int(row[2]), int(row[3])
            a, b = max(start, 0), min(end, o.lens[j])
            depth[int(o.starts[j]) + a:int(o.starts[j]) + b] += 1
            prec[j, strand] += 1
            prec[j, 2] += start < 0
            prec[j, 3] += end > o.lens[j]
        for j in range(R):
            d = depth[int(o.starts[j]):int(o.starts[j + 1])]
            prec[j, 4], prec[j, 5] = int((d > 0).sum()), int(d.sum())
        kept_rows = rows.copy()
        kept_rows[~accepted, 0] = po.NONE          # (for the pile-up oracle only: a rejected read piles nothing)
        counts = self.P.pile(seqs, kept_rows)
        return {"passes": passes, "rows": rows, "scores": scores, "accepted": accepted, "depth": depth, "place_rec": prec.astype(np.uint64),
                "score_rec": srec.astype(np.uint64), "unplaced": unplaced, "counts": counts}
