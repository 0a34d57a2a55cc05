"""Plain-Python oracle of the extended records (mf_align_extended), written from the rule in include/mitofilter.h: the extension pile from
the steps of tests/align_oracle.AlignOracle.align_row -- a diagonal step that puts a read base on a record coordinate outside [0, len) --
and the call per record and end from the unclamped sums, around the gapped consensus of tests/gapped_oracle.  Nothing here is shared
with the product."""
import numpy as np

from tests import align_oracle as ao
from tests import gapped_oracle as go
from tests import pileup_oracle as pio

LETTERS = "ACGT"
_IDX = {c: i for i, c in enumerate(LETTERS)}
BEGIN, END = 0, 1


def pile_steps(ext, x, steps, j, ln, E):
    """What one accepted read of record j adds to ext (int64[R, 2, E, 4]): a diagonal step of read base x[i] on coordinate c < 0 at
    [j, BEGIN, -1 - c], on c >= ln at [j, END, c - ln], where that offset is below E and x[i] is a letter.  An N adds nowhere and shifts
    no column; insertion and deletion steps add nowhere."""
    for mv, bi, c in steps:
        if mv != ao.DIAG or 0 <= c < ln:
            continue
        side, e = (BEGIN, -1 - c) if c < 0 else (END, c - ln)
        if e < E and x[bi] != "N":
            ext[j, side, e, _IDX[x[bi]]] += 1


def call_end(table, min_depth):
    """the emitted letters of one end, by offset from the record: table int[E, 4], unclamped"""
    out = []
    for row in table:
        row = [int(v) for v in row]
        m = max(row)
        if sum(row) < min_depth or row.count(m) != 1:          # a tie emits nothing and stops the end
            break
        out.append(LETTERS[row.index(m)])
    return "".join(out)


def call(gapped, gstarts, ext, min_depth):
    """-> (extended bytes, extended_starts [R + 1], records [R][length, begin_bases, end_bases, begin_piled, end_piled])"""
    assert min_depth >= 1
    out, xstarts, recs = bytearray(), [], []
    for j in range(len(gstarts) - 1):
        xstarts.append(len(out))
        b, e = call_end(ext[j, BEGIN], min_depth), call_end(ext[j, END], min_depth)
        out += b[::-1].encode() + bytes(gapped[gstarts[j]:gstarts[j + 1]]) + e.encode()
        recs.append([len(out) - xstarts[j], len(b), len(e), int(ext[j, BEGIN].sum()), int(ext[j, END].sum())])
    xstarts.append(len(out))
    return bytes(out), xstarts, recs


def overhang_bounds(o, want, E):
    """The invariant's right-hand side, int64[R, 2, E]: for every record and e the number of its accepted reads with -ref_begin > e (begin)
    and with ref_end - len > e (end)"""
    R = len(o.recs)
    bound = np.zeros((R, 2, E), np.int64)
    for row, al, ok in zip(want["rows"], want["aligns"], want["accepted"]):
        if not ok:
            continue
        j = int(row[0])
        over = (-int(al[4]), int(al[5]) - o.lens[j])
        for side in (BEGIN, END):
            if over[side] > 0:
                bound[j, side, :min(over[side], E)] += 1
    return bound


class ExtendOracle:
    def __init__(self, place_oracle):
        self.o = place_oracle
        self.G = go.GappedOracle(place_oracle)
        self.A = self.G.A

    def pile(self, seqs, want, W, E):
        """-> the extension pile int64[R, 2, E, 4] of the reads that AlignOracle.run accepted (want: what it gave)"""
        o = self.o
        ext = np.zeros((len(o.recs), 2, E, 4), np.int64)
        for seq, row, ok in zip(seqs, want["rows"], want["accepted"]):
            if not ok:
                continue
            j = int(row[0])
            a = self.A.align_row(seq, row, W)
            pile_steps(ext, self.A.oriented(seq, int(row[1])), a["steps"], j, o.lens[j], E)
        return ext

    def call(self, want, ins_pile, ext, min_depth):
        """the call from the sums of one or more runs -> (extended, extended_starts, extend_records)"""
        gapped, gstarts, _ = self.G.call(want, ins_pile, min_depth)
        return call(gapped, gstarts, ext, min_depth)

    def run(self, seqs, tallies, thr, max_permille, W, min_depth, E):
        """GappedOracle.run plus ext_pile int64[R, 2, E, 4], extended bytes, extended_starts and extend_records"""
        want = self.G.run(seqs, tallies, thr, max_permille, W, min_depth)
        want["ext_pile"] = self.pile(seqs, want, W, E)
        want["extended"], want["extended_starts"], want["extend_records"] = call(want["gapped"], want["gapped_starts"], want["ext_pile"], min_depth)
        return want


def clamped(ext):
    return np.minimum(ext, pio.CLAMP)
