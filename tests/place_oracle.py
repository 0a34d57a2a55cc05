"""Plain-Python oracle of read placement (mf_place), written from the semantics in include/mitofilter.h over strings: anchors are the
canonical k-mers that exactly one valid bait window holds (and that are not their own reverse complement); every anchor window of a
passing read votes for (record, strand, start); the strict winner places the read; base depth counts the placed reads over every
position.  Strand needs no canonical form: it is 0 when the read's window reads as the bait's text and 1 when its reverse complement
does."""
from collections import Counter

import numpy as np

from oracle import kmer_bait_ref as kb

AMBIGUOUS, NONE, CLAMP = 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFE
MAX_INSERT = 100000
_COMP = str.maketrans("ACGT", "TGCA")


def rc(w):
    return w.translate(_COMP)[::-1]


def canon(w):
    r = rc(w)
    return w if w < r else r


class PlaceOracle:
    def __init__(self, text, k):
        self.k = k
        self.recs = [kb._norm(r) for r in kb.read_fasta_records(text)]
        self.lens = [len(r) for r in self.recs]
        self.starts = np.cumsum([0] + self.lens).astype(np.uint64)
        held = Counter()
        where = {}
        for j, s in enumerate(self.recs):
            for p in range(len(s) - k + 1):
                w = s[p:p + k]
                if "N" in w:
                    continue
                c = canon(w)
                held[c] += 1
                where[c] = (j, p, w)
        self.bait = set(held)
        self.anchors = {c: where[c] for c, n in held.items() if n == 1 and where[c][2] != rc(where[c][2])}

    def votes(self, seq):
        """-> (hits, Counter of (record, strand, start)) of one read"""
        s, k = kb._norm(seq), self.k
        L = len(s)
        hits, v = 0, Counter()
        for o in range(L - k + 1):
            w = s[o:o + k]
            if "N" in w:
                continue
            c = canon(w)
            hits += c in self.bait
            a = self.anchors.get(c)
            if a is not None:
                j, p, text = a
                strand = 0 if w == text else 1
                v[(j, strand, p - o if strand == 0 else p - (L - k - o))] += 1
        return hits, v

    def tally(self, seqs):
        return [self.votes(s) + (len(s),) for s in seqs]

    def place(self, tallies, thr):
        """-> (passes bool[n], place rows int64[n, 6], base depth int64[positions] unclamped, records u64[R, 6], unplaced [2])"""
        n, R = len(tallies), len(self.recs)
        passes = np.zeros(n, bool)
        rows = np.zeros((n, 6), np.int64)
        depth = np.zeros(int(self.starts[-1]), np.int64)
        rec = np.zeros((R, 6), np.int64)
        unplaced = [0, 0]
        for i, (hits, v, L) in enumerate(tallies):
            if hits < thr:
                rows[i, 0] = NONE
                unplaced[1] += 1
                continue
            passes[i] = True
            windows = sum(v.values())
            top = v.most_common(2)
            if not top or (len(top) == 2 and top[0][1] == top[1][1]):
                rows[i] = (AMBIGUOUS, 0, 0, 0, 0, windows)
                unplaced[0] += 1
                continue
            (j, strand, start), n_votes = top[0]
            end = start + L
            rows[i] = (j, strand, start, end, n_votes, windows)
            a, b = max(start, 0), min(end, self.lens[j])
            assert a < b
            depth[int(self.starts[j]) + a:int(self.starts[j]) + b] += 1
            rec[j, strand] += 1
            rec[j, 2] += start < 0
            rec[j, 3] += end > self.lens[j]
        for j in range(R):
            d = depth[int(self.starts[j]):int(self.starts[j + 1])]
            rec[j, 4], rec[j, 5] = int((d > 0).sum()), int(d.sum())
        return passes, rows, depth, rec.astype(np.uint64), unplaced


def inserts(rows1, rows2):
    """insert size per pair from two place-row arrays; -1 where there is none"""
    out = []
    for a, b in zip(rows1, rows2):
        size = -1
        if a[0] < AMBIGUOUS and a[0] == b[0] and a[1] != b[1]:
            f, r = (a, b) if a[1] == 0 else (b, a)
            s = int(r[3]) - int(f[2])
            if 0 < s <= MAX_INSERT:
                size = s
        out.append(size)
    return np.array(out, np.int64)
