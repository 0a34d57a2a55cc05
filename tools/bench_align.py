#!/usr/bin/env python3
"""Cost of the banded alignment of the placed reads (mf_align) next to mf_verify, and a control that mf_verify itself costs what the
PARENT commit's does; prints one JSON object.

The two libraries run in ONE process, as in tools/bench_verify.py: this tree's through mitoflex_amd.mitofilter, the parent's through the
mitofilter.py of a checkout of the parent commit whose library is built (--parent-root DIR).  Each builds its own k-mer set and its own
read set from the same seed.  Every leg takes its two sides alternately, --reps (5) runs a side, ms a pass, on bench.py's resident set
(33.3 M x 150 b, 0.5 % bait reads, k = 31), record summaries and unplaced only (no per-read or per-position array is copied back).

  a   the PARENT library's mf_verify against this build's mf_verify (cut 1000, pile-up on): no existing kernel changed, so the change's
      median should lie inside the parent's own min .. max (`inside_parent_range`).
  b   this build's mf_verify against its mf_align at band 0 and at band 8 (the same cut, the pile-up on; the indel table stays on the
      device): ratios of medians, no bar.  About 0.5 % of the reads are placed, so this mostly shows what the other launch and the wider
      counters cost.
`headline`: the 16.5 kbp one-record bait; `eight`: the 8-record, ~132 kbp bait of tools/bench_assign.py.

    python tools/bench_align.py --parent-root DIR [--reads N] [--reps 5] [--only headline,eight] [--load-first parent|change]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_verify import alternately, compared, load_parent, timed  # noqa: E402


def legs(mf, ks, reads, pf, pks, preads, reps, min_depth=3):
    """mf, ks, reads: this tree's; pf, pks, preads: the parent's"""
    L, PL = mf.load(), pf.load()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    precs, urecs, srecs, arecs = (np.zeros(max(R, 1), d) for d in (mf.PLACE_RECORD, mf.PILEUP_RECORD, mf.SCORE_RECORD, mf.ALIGN_RECORD))
    pprecs, purecs, psrecs = (np.zeros(max(R, 1), d) for d in (pf.PLACE_RECORD, pf.PILEUP_RECORD, pf.SCORE_RECORD))
    unplaced, punplaced = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    verify = lambda: mf._chk(L.mf_verify(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, None, None, None, None, precs.ctypes.data, None, None,
                                         urecs.ctypes.data, srecs.ctypes.data, unplaced.ctypes.data, None))
    pverify = lambda: pf._chk(PL.mf_verify(pks._h, preads._h, 1, pf.MODE_SCREENED, min_depth, 1000, None, None, None, None, pprecs.ctypes.data, None, None,
                                           purecs.ctypes.data, psrecs.ctypes.data, punplaced.ctypes.data, None))

    def align(band):
        return lambda: mf._chk(L.mf_align(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, mf.KEEP_PASSING, band, None, None, None, None, None,
                                          precs.ctypes.data, None, None, urecs.ctypes.data, None, arecs.ctypes.data, unplaced.ctypes.data, None))
    out = {"records": R, "positions": P, "min_depth": min_depth, "tables_ms_with_first_call": round(timed(verify) * 1e3, 2)}
    tp, tv = alternately(pverify, verify, reps)
    out["a_verify_vs_parent_verify_ms"] = compared(tp, tv)
    out["same_score_records_as_parent"] = bool(all(np.array_equal(srecs[f], psrecs[f]) for f in pf.SCORE_RECORD.names))
    for band in (0, 8):
        tv, ta = alternately(verify, align(band), reps)
        leg = compared(tv, ta)          # ("parent" is mf_verify of this build here)
        leg.pop("inside_parent_range")
        out["b_align_band_%d_vs_verify_ms" % band] = leg
        out["band_%d" % band] = {f: int(arecs[f].sum()) for f in ("accepted", "rejected", "compared", "mismatches", "insertions", "deletions", "gapped")}
    out["band_0_same_as_verify"] = bool(all(out["band_0"][f] == int(srecs[f].sum()) for f in ("accepted", "rejected", "compared", "mismatches")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--reps", type=int, default=5)
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
        out["headline"] = legs(mf, ks, reads, pf, pks, preads, a.reps)
        ks.close(); pks.close()
    if "eight" in only:
        eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
        ks8, pks8 = mf.KmerSet.from_text(eight, 31), pf.KmerSet.from_text(eight, 31)
        out["eight"] = legs(mf, ks8, reads, pf, pks8, preads, a.reps)
        ks8.close(); pks8.close()
    reads.close(); preads.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
