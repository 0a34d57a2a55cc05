"""Plain-Python oracle of the banded alignment of placed reads (mf_align), written from the rule in include/mitofilter.h over strings:
a full table of the band's cells, the end cell by (least D, least distance from the placement's diagonal, smaller c), the traceback by
the first move that reproduces a cell in the order diagonal, deletion, insertion, and what an accepted read adds to base depth, the
records, the pile-up and the indel table.  Placements come from tests/place_oracle.PlaceOracle (its place rows), the call of the
pile-up from tests/pileup_oracle.PileupOracle; nothing here is shared with the product."""
import numpy as np

from oracle import kmer_bait_ref as kb
from tests import pileup_oracle as pio
from tests import place_oracle as po

BINS = 32
INF = 1 << 60
DIAG, DEL, INS = "M", "D", "I"
_IDX = {c: i for i, c in enumerate("ACGT")}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def accepts(compared, mismatches, insertions, deletions, max_permille):
    return (mismatches + insertions + deletions) * 1000 <= max_permille * (compared + insertions + deletions)


def sub(x, i, rec, c):
    """-> (cost, compared) of read base x[i] on record coordinate c"""
    if not 0 <= c < len(rec) or x[i] == "N" or rec[c] == "N":
        return 0, False
    return int(x[i] != rec[c]), True


def align(x, rec, start, W):
    """The alignment of the oriented read x placed at start on the record rec inside the band W.
    -> dict: compared, mismatches, insertions, deletions, ref_begin, ref_end, steps: [(move, i, c)] in path order, where a diagonal step
    puts read base i on c, a deletion step deletes bait position c (in row i) and an insertion step puts read base i between c-1 and c"""
    L = len(x)
    D = [dict() for _ in range(L + 1)]
    for c in range(start - W, start + W + 1):
        D[0][c] = 0
    for i in range(1, L + 1):
        for c in range(start + i - W, start + i + W + 1):          # ascending: the deletion reads the cell to the left
            D[i][c] = min(D[i - 1].get(c - 1, INF) + sub(x, i - 1, rec, c - 1)[0], D[i - 1].get(c, INF) + 1, D[i].get(c - 1, INF) + 1)
    end = min(D[L], key=lambda c: (D[L][c], abs(c - (start + L)), c))
    i, c, steps = L, end, []
    while i > 0:
        v = D[i][c]
        if v == D[i - 1].get(c - 1, INF) + sub(x, i - 1, rec, c - 1)[0]:
            steps.append((DIAG, i - 1, c - 1))
            i, c = i - 1, c - 1
        elif v == D[i].get(c - 1, INF) + 1:
            steps.append((DEL, i, c - 1))
            c -= 1
        else:
            assert v == D[i - 1].get(c, INF) + 1
            steps.append((INS, i - 1, c))
            i -= 1
    steps.reverse()
    out = {"compared": 0, "mismatches": 0, "insertions": 0, "deletions": 0, "ref_begin": c, "ref_end": end, "steps": steps, "D": D[L][end]}
    for mv, bi, bc in steps:
        if mv == DIAG:
            s, cmpd = sub(x, bi, rec, bc)
            out["compared"] += cmpd
            out["mismatches"] += s
        else:
            out["insertions" if mv == INS else "deletions"] += 1
    assert out["mismatches"] + out["insertions"] + out["deletions"] == out["D"]
    return out


_CODE = np.full(256, -1, np.int64)
_CODE[list(b"ACGT")] = range(4)


def align_fast(x, rec, start, W):
    """align() restated a row at a time over arrays, for read sets of thousands (tests/test_align_oracle.py holds it to align()): the
    deletions inside a row are a running minimum, D[d] = d + min over e <= d of (t[e] - e); the traceback reads the stored rows by the
    same preference"""
    L, n = len(x), 2 * W + 1
    xs = _CODE[np.frombuffer(x.encode(), np.uint8)]
    lo = start - W - 1                                             # the record coordinate of ref[0]
    cs = np.arange(lo, start + L + W + 1)
    inside = (cs >= 0) & (cs < len(rec))
    ref = np.full(len(cs), -1, np.int64)
    if inside.any():
        ref[inside] = _CODE[np.frombuffer(rec[cs[inside][0]:cs[inside][-1] + 1].encode(), np.uint8)]
    ar = np.arange(n)
    windows = np.lib.stride_tricks.sliding_window_view(ref, n)[1:L + 1]          # row i: the bait letters at c - 1 of its cells, ref[i:i + n]
    S = ((windows != xs[:, None]) & (windows >= 0) & (xs[:, None] >= 0)).astype(np.int64)
    Dm = np.zeros((L + 1, n + 1), np.int64)
    Dm[:, n] = INF                                                  # (the cell above the band's last diagonal)
    for i in range(1, L + 1):
        t = np.minimum(Dm[i - 1, :n] + S[i - 1], Dm[i - 1, 1:] + 1)
        Dm[i, :n] = np.minimum.accumulate(t - ar) + ar
    ends = [(int(Dm[L, d]), abs(d - W), d) for d in range(n)]
    _, _, d = min(ends)
    end = start + L + d - W
    i, steps = L, []
    while i > 0:
        c = start + i + d - W
        v = Dm[i, d]
        if v == Dm[i - 1, d] + sub(x, i - 1, rec, c - 1)[0]:
            steps.append((DIAG, i - 1, c - 1))
            i -= 1
        elif d > 0 and v == Dm[i, d - 1] + 1:
            steps.append((DEL, i, c - 1))
            d -= 1
        else:
            assert d < n - 1 and v == Dm[i - 1, d + 1] + 1
            steps.append((INS, i - 1, c))
            i, d = i - 1, d + 1
    steps.reverse()
    out = {"compared": 0, "mismatches": 0, "insertions": 0, "deletions": 0, "ref_begin": start + d - W, "ref_end": end, "steps": steps,
           "D": int(Dm[L, end - start - L + W])}
    for mv, bi, bc in steps:
        if mv == DIAG:
            sc, cmpd = sub(x, bi, rec, bc)
            out["compared"] += cmpd
            out["mismatches"] += sc
        else:
            out["insertions" if mv == INS else "deletions"] += 1
    assert out["mismatches"] + out["insertions"] + out["deletions"] == out["D"]
    return out


def insertion_runs(steps):
    """-> [(c, n)]: the maximal runs of n consecutive insertion steps at column c"""
    runs = []
    prev = None
    for mv, _, c in steps:
        if mv == INS and prev == (INS, c):
            runs[-1][1] += 1
        elif mv == INS:
            runs.append([c, 1])
        prev = (mv, c) if mv == INS else None
    return [(c, n) for c, n in runs]


class AlignOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.P = pio.PileupOracle(place_oracle)
        self.memo = {}

    def oriented(self, seq, strand):
        s = kb._norm(seq)
        return s if strand == 0 else "".join(_COMP[ch] for ch in reversed(s))

    def align_row(self, seq, row, W):
        """-> the alignment of one read placed as row (a PlaceOracle place row), or None when it is not placed"""
        j = int(row[0])
        if j >= po.AMBIGUOUS:
            return None
        key = (self.oriented(seq, int(row[1])), j, int(row[2]), W)          # (stacked reads: one alignment)
        if key not in self.memo:
            self.memo[key] = align_fast(key[0], self.o.recs[j], key[2], W)
        return self.memo[key]

    def run(self, seqs, tallies, thr, max_permille, W):
        """-> dict: passes bool[n], rows int64[n, 6] (placement's), aligns int64[n, 6] (compared, mismatches, insertions, deletions,
        ref_begin, ref_end; zeros when not placed), accepted bool[n], depth int64[positions] unclamped, place_rec u64[R, 6], align_rec
        u64[R, 7 + BINS], unplaced [2], counts int64[positions, 4], indels int64[positions, 3] (del, ins, ins_bases), footprints: the sum
        of the clipped footprints of every record's accepted reads"""
        assert 0 <= max_permille <= 1000 and 0 <= W <= 31 and W < self.o.k
        o = self.o
        passes, rows, _, _, unplaced = o.place(tallies, thr)
        n, R, P = len(seqs), len(o.recs), int(o.starts[-1])
        aligns = np.zeros((n, 6), np.int64)
        accepted = np.zeros(n, bool)
        arec = np.zeros((R, 7 + BINS), np.int64)
        prec = np.zeros((R, 6), np.int64)
        depth = np.zeros(P, np.int64)
        counts = np.zeros((P, 4), np.int64)
        indels = np.zeros((P, 3), np.int64)
        foot = np.zeros(R, np.int64)
        for r, (seq, row) in enumerate(zip(seqs, rows)):
            a = self.align_row(seq, row, W)
            if a is None:
                continue
            j, strand, s0, ln = int(row[0]), int(row[1]), int(o.starts[int(row[0])]), o.lens[int(row[0])]
            c, m, ni, nd = a["compared"], a["mismatches"], a["insertions"], a["deletions"]
            aligns[r] = (c, m, ni, nd, a["ref_begin"], a["ref_end"])
            arec[j, 7 + min(m + ni + nd, BINS - 1)] += 1
            if not accepts(c, m, ni, nd, max_permille):
                arec[j, 1] += 1
                continue
            accepted[r] = True
            arec[j, 0] += 1
            arec[j, 2:7] += (c, m, ni, nd, int(ni + nd > 0))
            lo, hi = max(a["ref_begin"], 0), min(a["ref_end"], ln)
            assert lo < hi
            depth[s0 + lo:s0 + hi] += 1
            foot[j] += hi - lo
            prec[j, strand] += 1
            prec[j, 2] += a["ref_begin"] < 0
            prec[j, 3] += a["ref_end"] > ln
            x = self.oriented(seq, strand)
            for mv, bi, bc in a["steps"]:
                if mv == DIAG and x[bi] != "N" and 0 <= bc < ln:
                    counts[s0 + bc, _IDX[x[bi]]] += 1
                elif mv == DEL and 0 <= bc < ln:
                    indels[s0 + bc, 0] += 1
            for bc, cnt in insertion_runs(a["steps"]):
                if 0 <= bc - 1 < ln:
                    indels[s0 + bc - 1, 1] += 1
                    indels[s0 + bc - 1, 2] += cnt
        for j in range(R):
            d = depth[int(o.starts[j]):int(o.starts[j + 1])]
            prec[j, 4], prec[j, 5] = int((d > 0).sum()), int(d.sum())
        return {"passes": passes, "rows": rows, "aligns": aligns, "accepted": accepted, "depth": depth, "place_rec": prec.astype(np.uint64),
                "align_rec": arec.astype(np.uint64), "unplaced": unplaced, "counts": counts, "indels": indels, "footprints": foot}


def keep_bits(want, keep):
    """the keep bits of every read from what AlignOracle.run gave: 0 the passing reads, 1 (accepted) without the placed reads the cut
    rejects, 2 (placed) the accepted reads alone"""
    placed = want["rows"][:, 0] < po.AMBIGUOUS
    if keep == 1:
        return want["passes"] & ~(placed & ~want["accepted"])
    if keep == 2:
        return want["passes"] & placed & want["accepted"]
    return want["passes"].copy()
