"""Plain-Python oracle of pair-aware placement (mf_place_pairs), written from the "pairs" section of include/mitofilter.h over
tests/verify_oracle.VerifyOracle and strings: each mate set verified on its own, the insert and the kind of every pair, the rescue of a
mate that is not placed from the candidates its settled mate implies -- one per insert d, scored by VerifyOracle.score, admissible when
compared >= k and mismatches * 1000 <= rescue_permille * compared, rescued when exactly one admissible candidate has the fewest
mismatches -- and every report over both sets with the rescued mates counted as accepted placed reads.  Nothing here is shared with the
product."""
import numpy as np

from tests import place_oracle as po
from tests import verify_oracle as vo

NONE, PROPER, DISCORDANT, RESCUED_1, RESCUED_2, SINGLE_1, SINGLE_2 = range(7)
RESCUE_MAX = 4096


def candidate_start(s, a, e, L, d):
    """leftmost record coordinate of the candidate for insert d of a mate of L bases whose settled mate lies on strand s at [a, e)"""
    return a + d - L if s == 0 else e - d


def insert_of(a, b):
    """insert of two settled mates' place rows: `end` of the strand-1 mate minus `start` of the strand-0 mate when they lie on one
    record and on opposite strands and that is above 0, else -1"""
    if a[0] != b[0] or a[1] == b[1]:
        return -1
    f, r = (a, b) if a[1] == 0 else (b, a)
    s = int(r[3]) - int(f[2])
    return s if s > 0 else -1


class PairOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.V = vo.VerifyOracle(place_oracle)
        self.scored = {}

    def rescue(self, seq, A, min_insert, max_insert, rescue_permille):
        """the mate `seq` of the settled mate with place row A -> ((start, d, compared, mismatches), None) when it is rescued, else
        (None, why): "tie" when several admissible candidates share the fewest mismatches, "cut" when some candidate compares k bases
        or more and none is admissible, "short" when no candidate compares k bases"""
        j, s, a, e = int(A[0]), int(A[1]), int(A[2]), int(A[3])
        L = len(seq)
        best, reached = [], False
        key = (seq, j, s, a, e, min_insert, max_insert)
        if key not in self.scored:          # (the candidates' scores do not depend on the cut: a test asks with several)
            starts = [candidate_start(s, a, e, L, d) for d in range(min_insert, max_insert + 1)]
            self.scored[key] = [(start,) + tuple(self.V.score(seq, (j, 1 - s, start, start + L, 0, 0))) for start in starts]
        for d, (start, c, m) in zip(range(min_insert, max_insert + 1), self.scored[key]):
            if c < self.o.k:
                continue
            reached = True
            if m * 1000 > rescue_permille * c:
                continue
            if not best or m < best[0][3]:
                best = [(start, d, c, m)]
            elif m == best[0][3]:
                best.append((start, d, c, m))
        if len(best) == 1:
            return best[0], None
        return None, "tie" if best else "cut" if reached else "short"

    def account(self, seqs, rows, scores, accepted):
        """the reports of a verifying call over reads with these place rows and scores, the accepted ones counted (a rescued mate is
        one of them) -> depth, place_rec, score_rec, unplaced, counts as VerifyOracle.verify names them"""
        o = self.o
        R = len(o.recs)
        srec = np.zeros((R, 4 + vo.BINS), np.int64)
        prec = np.zeros((R, 6), np.int64)
        depth = np.zeros(int(o.starts[-1]), np.int64)
        unplaced = [0, 0]
        for i, row in enumerate(rows):
            j = int(row[0])
            if j >= po.AMBIGUOUS:
                unplaced[0 if j == po.AMBIGUOUS else 1] += 1
                continue
            c, m = int(scores[i][0]), int(scores[i][1])
            srec[j, 4 + min(m, vo.BINS - 1)] += 1
            if not accepted[i]:
                srec[j, 1] += 1
                continue
            srec[j, 0] += 1
            srec[j, 2] += c
            srec[j, 3] += m
            strand, start, end = int(row[1]), int(row[2]), int(row[3])
            a, b = max(start, 0), min(end, o.lens[j])
            assert a < b
            depth[int(o.starts[j]) + a:int(o.starts[j]) + b] += 1
            prec[j, strand] += 1
            prec[j, 2] += start < 0
            prec[j, 3] += end > o.lens[j]
        for j in range(R):
            d = depth[int(o.starts[j]):int(o.starts[j + 1])]
            prec[j, 4], prec[j, 5] = int((d > 0).sum()), int(d.sum())
        kept = np.array(rows, np.int64).reshape(-1, 6).copy()
        kept[~np.asarray(accepted, bool), 0] = po.NONE
        return {"depth": depth, "place_rec": prec.astype(np.uint64), "score_rec": srec.astype(np.uint64), "unplaced": unplaced,
                "counts": self.V.P.pile(seqs, kept)}

    def pairs(self, seqs1, seqs2, tallies1, tallies2, thr, max_permille, min_insert, max_insert, rescue, rescue_permille):
        """-> dict: passes1 / passes2, rows1 / rows2, scores1 / scores2 (rescues applied), pairs int64[n, 2] (kind, insert), pair_rec
        u64[R, 6], none, why (per pair: None, or why a rescue target was refused), and the reports of `account` over both sets"""
        assert len(seqs1) == len(seqs2) and 1 <= min_insert <= max_insert and max_insert - min_insert + 1 <= RESCUE_MAX
        assert 0 <= rescue_permille <= 1000 and rescue in (0, 1)
        n, R = len(seqs1), len(self.o.recs)
        v = [self.V.verify(seqs1, tallies1, thr, max_permille), self.V.verify(seqs2, tallies2, thr, max_permille)]
        seqs = [seqs1, seqs2]
        rows = [v[0]["rows"].copy(), v[1]["rows"].copy()]
        scores = [v[0]["scores"].copy(), v[1]["scores"].copy()]
        accepted = [v[0]["accepted"].copy(), v[1]["accepted"].copy()]
        settled = [v[0]["accepted"], v[1]["accepted"]]
        pairs = np.zeros((n, 2), np.int64)
        prec = np.zeros((R, 6), np.int64)
        none, why = 0, [None] * n
        for i in range(n):
            a, b = v[0]["rows"][i], v[1]["rows"][i]
            if settled[0][i] and settled[1][i]:
                ins = insert_of(a, b)
                j = int(a[0])
                if a[0] != b[0]:
                    pairs[i] = (DISCORDANT, -1)
                    prec[j, 2] += 1
                elif min_insert <= ins <= max_insert:
                    pairs[i] = (PROPER, ins)
                    prec[j, 0] += 1
                    prec[j, 5] += ins
                else:
                    pairs[i] = (DISCORDANT, ins)
                    prec[j, 1] += 1
            elif settled[0][i] or settled[1][i]:
                m = 0 if settled[0][i] else 1          # the settled mate's set; 1 - m is looked for
                A, B = v[m]["rows"][i], v[1 - m]["rows"][i]
                j = int(A[0])
                won = None
                if rescue and int(B[0]) >= po.AMBIGUOUS:
                    won, why[i] = self.rescue(seqs[1 - m][i], A, min_insert, max_insert, rescue_permille)
                if won is None:
                    pairs[i] = (SINGLE_1 if m == 0 else SINGLE_2, -1)
                    prec[j, 4] += 1
                    continue
                start, d, c, mm = won
                L = len(seqs[1 - m][i])
                rows[1 - m][i] = (j, 1 - int(A[1]), start, start + L, 0, int(B[5]))
                scores[1 - m][i] = (c, mm)
                accepted[1 - m][i] = True
                pairs[i] = (RESCUED_2 if m == 0 else RESCUED_1, d)
                prec[j, 3] += 1
                prec[j, 5] += d
            else:
                pairs[i] = (NONE, -1)
                none += 1
        out = self.account(list(seqs1) + list(seqs2), np.concatenate(rows), np.concatenate(scores), np.concatenate(accepted))
        out.update({"passes1": v[0]["passes"], "passes2": v[1]["passes"], "rows1": rows[0], "rows2": rows[1], "scores1": scores[0], "scores2": scores[1],
                    "pairs": pairs, "pair_rec": prec.astype(np.uint64), "none": none, "why": why, "single": v})
        return out
