#!/usr/bin/env python3
"""Cost of the gapped consensus' insertion pile (mf_align_gapped) next to mf_align, and a control that mf_align itself costs what the
PARENT commit's does; prints one JSON object.

The two libraries run in ONE process, as in tools/bench_verify.py and tools/bench_align.py: this tree's through mitoflex_amd.mitofilter,
the parent's through the mitofilter.py of a checkout of the parent commit whose library is built (--parent-root DIR).  Each builds its own
k-mer set and its own read set from the same seed.  Every leg takes its two sides alternately, --reps (5) runs a side, ms a pass, on
bench.py's resident set (33.3 M x 150 b, 0.5 % bait reads, k = 31), band 8, cut 1000, the pile-up on, record summaries and unplaced only.

  a   the PARENT library's mf_align against this build's mf_align: the plain launch is unchanged, so the change's median should lie inside
      the parent's own min .. max (`inside_parent_range`); a miss is reported as one.
  b   this build's mf_align against its mf_align_gapped asked for the gapped record summaries alone -- the insertion pile, the emitted
      bytes and their counts stay on the device: what zeroing and reading 4 * span words a position, one atomic an inserted base and the
      call kernel cost.  Stated as measured, no bar.
`headline`: the 16.5 kbp one-record bait; `eight`: the 8-record, ~132 kbp bait of tools/bench_assign.py.

    python tools/bench_gapped.py --parent-root DIR [--reads N] [--reps 5] [--band 8] [--only headline,eight] [--load-first parent|change]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_verify import alternately, compared, load_parent, timed  # noqa: E402

SUMS = ("accepted", "rejected", "compared", "mismatches", "insertions", "deletions", "gapped")


def legs(mf, ks, reads, pf, pks, preads, reps, band, min_depth=3):
    """mf, ks, reads: this tree's; pf, pks, preads: the parent's"""
    L, PL = mf.load(), pf.load()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    precs, urecs, arecs, grecs = (np.zeros(max(R, 1), d) for d in (mf.PLACE_RECORD, mf.PILEUP_RECORD, mf.ALIGN_RECORD, mf.GAPPED_RECORD))
    pprecs, purecs, parecs = (np.zeros(max(R, 1), d) for d in (pf.PLACE_RECORD, pf.PILEUP_RECORD, pf.ALIGN_RECORD))
    unplaced, punplaced = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    align = lambda: mf._chk(L.mf_align(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, mf.KEEP_PASSING, band, None, None, None, None, None,
                                       precs.ctypes.data, None, None, urecs.ctypes.data, None, arecs.ctypes.data, unplaced.ctypes.data, None))
    palign = lambda: pf._chk(PL.mf_align(pks._h, preads._h, 1, pf.MODE_SCREENED, min_depth, 1000, pf.KEEP_PASSING, band, None, None, None, None, None,
                                         pprecs.ctypes.data, None, None, purecs.ctypes.data, None, parecs.ctypes.data, punplaced.ctypes.data, None))
    gapped = lambda: mf._chk(L.mf_align_gapped(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, mf.KEEP_PASSING, band, None, None, None, None, None,
                                               precs.ctypes.data, None, None, urecs.ctypes.data, None, arecs.ctypes.data, None, None, None, grecs.ctypes.data,
                                               unplaced.ctypes.data, None))
    out = {"records": R, "positions": P, "band": band, "min_depth": min_depth, "insertion_pile_bytes": 4 * 2 * band * P * 8,
           "tables_ms_with_first_call": round(timed(align) * 1e3, 2)}
    tp, ta = alternately(palign, align, reps)
    out["a_align_vs_parent_align_ms"] = compared(tp, ta)
    out["same_align_records_as_parent"] = bool(all(np.array_equal(arecs[f], parecs[f]) for f in pf.ALIGN_RECORD.names))
    plain = {f: int(arecs[f].sum()) for f in SUMS}
    ta, tg = alternately(align, gapped, reps)
    leg = compared(ta, tg)          # ("parent" is mf_align of this build here)
    leg.pop("inside_parent_range")
    out["b_gapped_vs_align_ms"] = leg
    out["gapped_same_align_records"] = bool(plain == {f: int(arecs[f].sum()) for f in SUMS})
    out["align"] = plain
    out["gapped_records"] = {f: int(grecs[f].sum()) for f in mf.GAPPED_RECORD.names}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--only", default="headline,eight")
    ap.add_argument("--load-first", choices=("parent", "change"), default="parent",
                    help="which library the process loads first (the second one loaded has measured slower whatever it holds: run both orders)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    from tools.bench_assign import mutated
    if a.load_first == "change":
        mf.load()
    pf = load_parent(a.parent_root)
    bait = make_bait()
    g = bait_records(bait)[0]
    synth = dict(seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
    reads, preads = mf.Reads.synth(a.reads, 150, **synth), pf.Reads.synth(a.reads, 150, **synth)
    out = {"loaded_first": a.load_first}
    if "headline" in only:
        ks, pks = mf.KmerSet.from_text(bait, 31), pf.KmerSet.from_text(bait, 31)
        out["headline"] = legs(mf, ks, reads, pf, pks, preads, a.reps, a.band)
        ks.close(); pks.close()
    if "eight" in only:
        eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
        ks8, pks8 = mf.KmerSet.from_text(eight, 31), pf.KmerSet.from_text(eight, 31)
        out["eight"] = legs(mf, ks8, reads, pf, pks8, preads, a.reps, a.band)
        ks8.close(); pks8.close()
    reads.close(); preads.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
