"""Plain-Python oracle of pairs with a band (mf_align_pairs), written from the "pairs with a band" section of include/mitofilter.h over
tests/pair_oracle.PairOracle, tests/align_oracle.AlignOracle, tests/gapped_oracle and tests/extend_oracle: each mate set aligned on its
own, settled by the aligned cut; insert, kind and the rescue's candidates by the place rows exactly as PairOracle has them (the seed is
ungapped: PairOracle.rescue unchanged); the rescued mate aligned inside the band around the winning candidate's start and counted as an
accepted aligned read; every report over both sets by AlignOracle.run's accounting.  Nothing here is shared with the product."""
import numpy as np

from tests import align_oracle as ao
from tests import extend_oracle as xo
from tests import gapped_oracle as go
from tests import pair_oracle as pa
from tests import place_oracle as po

NONE, PROPER, DISCORDANT, RESCUED_1, RESCUED_2, SINGLE_1, SINGLE_2 = range(7)


class PairAlignOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.P = pa.PairOracle(place_oracle)
        self.X = xo.ExtendOracle(place_oracle)
        self.G = self.X.G
        self.A = self.X.A

    def account(self, seqs, rows, accepted, W):
        """AlignOracle.run's accounting over reads with these place rows, the accepted ones counted (a rescued mate is one of them, aligned
        around its row's start as any placed read is) -> aligns, depth, place_rec, align_rec, counts, indels, footprints"""
        o = self.o
        n, R, P = len(seqs), len(o.recs), int(o.starts[-1])
        aligns = np.zeros((n, 6), np.int64)
        arec = np.zeros((R, 7 + ao.BINS), np.int64)
        prec = np.zeros((R, 6), np.int64)
        depth = np.zeros(P, np.int64)
        counts = np.zeros((P, 4), np.int64)
        indels = np.zeros((P, 3), np.int64)
        foot = np.zeros(R, np.int64)
        for r, (seq, row) in enumerate(zip(seqs, rows)):
            a = self.A.align_row(seq, row, W)
            if a is None:
                continue
            j, strand = int(row[0]), int(row[1])
            s0, ln = int(o.starts[j]), o.lens[j]
            c, m, ni, nd = a["compared"], a["mismatches"], a["insertions"], a["deletions"]
            aligns[r] = (c, m, ni, nd, a["ref_begin"], a["ref_end"])
            arec[j, 7 + min(m + ni + nd, ao.BINS - 1)] += 1
            if not accepted[r]:
                arec[j, 1] += 1
                continue
            arec[j, 0] += 1
            arec[j, 2:7] += (c, m, ni, nd, int(ni + nd > 0))
            lo, hi = max(a["ref_begin"], 0), min(a["ref_end"], ln)
            assert lo < hi, "an accepted read's clipped footprint is not empty"
            depth[s0 + lo:s0 + hi] += 1
            foot[j] += hi - lo
            prec[j, strand] += 1
            prec[j, 2] += a["ref_begin"] < 0
            prec[j, 3] += a["ref_end"] > ln
            x = self.A.oriented(seq, strand)
            for mv, bi, bc in a["steps"]:
                if mv == ao.DIAG and x[bi] != "N" and 0 <= bc < ln:
                    counts[s0 + bc, "ACGT".index(x[bi])] += 1
                elif mv == ao.DEL and 0 <= bc < ln:
                    indels[s0 + bc, 0] += 1
            for bc, cnt in ao.insertion_runs(a["steps"]):
                if 0 <= bc - 1 < ln:
                    indels[s0 + bc - 1, 1] += 1
                    indels[s0 + bc - 1, 2] += cnt
        for j in range(R):
            d = depth[int(o.starts[j]):int(o.starts[j + 1])]
            prec[j, 4], prec[j, 5] = int((d > 0).sum()), int(d.sum())
        return {"aligns": aligns, "depth": depth, "place_rec": prec.astype(np.uint64), "align_rec": arec.astype(np.uint64), "counts": counts,
                "indels": indels, "footprints": foot}

    def pairs(self, seqs1, seqs2, tallies1, tallies2, thr, max_permille, W, min_insert, max_insert, rescue, rescue_permille, min_depth=1, E=0):
        """-> dict: passes1 / passes2, rows1 / rows2, aligns1 / aligns2 (rescues applied), pairs int64[n, 2], pair_rec u64[R, 6], none, why,
        single (the two AlignOracle.run results), the reports of `account` over both sets, rows / accepted over both sets (set 1 first),
        unplaced, ins_pile, gapped, gapped_starts, gapped_records and, with E > 0, ext_pile, extended, extended_starts, extend_records"""
        assert len(seqs1) == len(seqs2) and 1 <= min_insert <= max_insert and max_insert - min_insert + 1 <= pa.RESCUE_MAX
        assert 0 <= rescue_permille <= 1000 and rescue in (0, 1)
        n, R = len(seqs1), len(self.o.recs)
        v = [self.A.run(seqs1, tallies1, thr, max_permille, W), self.A.run(seqs2, tallies2, thr, max_permille, W)]
        seqs = [list(seqs1), list(seqs2)]
        rows = [v[0]["rows"].copy(), v[1]["rows"].copy()]
        accepted = [v[0]["accepted"].copy(), v[1]["accepted"].copy()]
        settled = [v[0]["accepted"], v[1]["accepted"]]
        unplaced = [v[0]["unplaced"][0] + v[1]["unplaced"][0], v[0]["unplaced"][1] + v[1]["unplaced"][1]]
        pairs = np.zeros((n, 2), np.int64)
        prec = np.zeros((R, 6), np.int64)
        none, why = 0, [None] * n
        for i in range(n):
            a, b = v[0]["rows"][i], v[1]["rows"][i]
            if settled[0][i] and settled[1][i]:
                ins = pa.insert_of(a, b)
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
                m = 0 if settled[0][i] else 1
                A, B = v[m]["rows"][i], v[1 - m]["rows"][i]
                j = int(A[0])
                won = None
                if rescue and int(B[0]) >= po.AMBIGUOUS:
                    won, why[i] = self.P.rescue(seqs[1 - m][i], A, min_insert, max_insert, rescue_permille)
                if won is None:
                    pairs[i] = (SINGLE_1 if m == 0 else SINGLE_2, -1)
                    prec[j, 4] += 1
                    continue
                start, d, _, _ = won
                L = len(seqs[1 - m][i])
                rows[1 - m][i] = (j, 1 - int(A[1]), start, start + L, 0, int(B[5]))
                accepted[1 - m][i] = True
                unplaced[0 if int(B[0]) == po.AMBIGUOUS else 1] -= 1
                pairs[i] = (RESCUED_2 if m == 0 else RESCUED_1, d)
                prec[j, 3] += 1
                prec[j, 5] += d
            else:
                pairs[i] = (NONE, -1)
                none += 1
        both = seqs[0] + seqs[1]
        out = self.account(both, np.concatenate(rows), np.concatenate(accepted), W)
        out.update({"passes1": v[0]["passes"], "passes2": v[1]["passes"], "rows1": rows[0], "rows2": rows[1], "aligns1": out["aligns"][:n],
                    "aligns2": out["aligns"][n:], "rows": np.concatenate(rows), "accepted": np.concatenate(accepted), "unplaced": unplaced,
                    "pairs": pairs, "pair_rec": prec.astype(np.uint64), "none": none, "why": why, "single": v})
        out["ins_pile"] = self.G.pile(both, out, W)
        out["gapped"], out["gapped_starts"], out["gapped_records"] = self.G.call(out, out["ins_pile"], min_depth)
        if E:
            out["ext_pile"] = self.X.pile(both, out, W, E)
            out["extended"], out["extended_starts"], out["extend_records"] = xo.call(out["gapped"], out["gapped_starts"], out["ext_pile"], min_depth)
        return out
