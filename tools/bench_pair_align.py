#!/usr/bin/env python3
"""Cost of the aligning paired call (mf_align_pairs) next to the PARENT commit's mf_place_pairs and next to this build's own single-set
aligning calls; prints one JSON object.

The two libraries run in ONE process, as in tools/bench_pairs.py: this tree's through mitoflex_amd.mitofilter, the parent's through the
mitofilter.py of a checkout of the parent commit whose library is built (--parent-root DIR).  Each builds its own k-mer set and its own
read sets from the same data.  Every leg takes its two sides alternately, --reps (5) runs a side, ms a call; record summaries, the pair
records and unplaced only, no pile-up.  The data is tools/bench_pairs.py's leg b: --pairs (200 k) pairs of 150-base mates drawn from the
bait's first record, whose sample differs every 20 bases along --diverged-share (10 %) of its length; a window of --window (400) inserts.

  a   the PARENT's mf_place_pairs against this build's mf_place_pairs, rescue = 1: the plain call runs the kernels it ran (the shared
      host body is what changed).  The expectation: the change's median inside the parent's own min .. max; a miss is reported as one.
  b   this build's mf_place_pairs against mf_align_pairs at --band (8), rescue = 1 on both: what the band costs -- both sets through
      align_kernel instead of place_kernel, and the rescued mates aligned.  Stated as measured, no bar.
  c   this build's two mf_align passes (one a set) against mf_align_pairs at rescue = 0: what the pair list costs on top.  No bar.

    python tools/bench_pair_align.py --parent-root DIR [--reps 5] [--pairs N] [--window W] [--band W] [--only a,b,c]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pairs import drawn_pairs, pack, paired_call  # noqa: E402
from tools.bench_verify import alternately, compared, load_parent  # noqa: E402


def aligned_pair_call(mf, ks, r1, r2, lo, hi, band, rescue, bufs):
    L = mf.load()
    precs, arecs, prs, none, unplaced = bufs
    return lambda: mf._chk(L.mf_align_pairs(ks._h, r1._h, r2._h, 1, mf.MODE_SCREENED, 1, 1000, band, 0, lo, hi, rescue, 100, *([None] * 8), precs.ctypes.data,
                                            *([None] * 4), arecs.ctypes.data, *([None] * 8), prs.ctypes.data, none.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            unplaced.ctypes.data, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--diverged-share", type=float, default=0.10)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    pf = load_parent(a.parent_root)
    bait = make_bait()
    ks, pks = mf.KmerSet.from_text(bait, 31), pf.KmerSet.from_text(bait, 31)
    R = max(len(ks.record_starts) - 1, 1)
    shared = [np.zeros(R, mf.PLACE_RECORD), None, np.zeros(R, mf.PAIR_RECORD), np.zeros(1, np.uint64), np.zeros(2, np.uint64)]
    bufs = shared[:1] + [np.zeros(R, mf.SCORE_RECORD)] + shared[2:]
    abufs = shared[:1] + [np.zeros(R, mf.ALIGN_RECORD)] + shared[2:]
    pbufs = [np.zeros(R, pf.PLACE_RECORD), np.zeros(R, pf.SCORE_RECORD), np.zeros(R, pf.PAIR_RECORD), np.zeros(1, np.uint64), np.zeros(2, np.uint64)]
    c1, c2, share = drawn_pairs(bait_records(bait)[0], a.pairs, a.diverged_share, 7)
    r1, r2 = mf.Reads.from_packed(*pack(c1)), mf.Reads.from_packed(*pack(c2))
    p1, p2 = pf.Reads.from_packed(*pack(c1)), pf.Reads.from_packed(*pack(c2))
    lo, hi = 400 - a.window // 2 + 1, 400 + a.window // 2
    out = {"pairs": a.pairs, "window": [lo, hi], "band": a.band, "share_of_pairs_with_a_diverged_mate": round(share, 4)}
    pair_sums = lambda b, m: {f: int(b[2][f].sum()) for f in m.PAIR_RECORD.names}
    if "a" in only:
        parent, change = paired_call(pf, pks, p1, p2, lo, hi, 1, pbufs), paired_call(mf, ks, r1, r2, lo, hi, 1, bufs)
        leg = compared(*alternately(parent, change, a.reps))
        parent(); change()
        leg.update({"same_pair_records_as_parent": pair_sums(pbufs, pf) == pair_sums(bufs, mf) and pbufs[4].tolist() == bufs[4].tolist(), "pair_records": pair_sums(bufs, mf)})
        out["a_parent_place_pairs_vs_place_pairs_ms"] = leg
    if "b" in only:
        plain, banded = paired_call(mf, ks, r1, r2, lo, hi, 1, bufs), aligned_pair_call(mf, ks, r1, r2, lo, hi, a.band, 1, abufs)
        leg = compared(*alternately(plain, banded, a.reps))          # ("parent" is this build's mf_place_pairs here)
        leg.pop("inside_parent_range")
        plain()
        was = pair_sums(bufs, mf)
        banded()
        leg.update({"pair_records_plain": was, "pair_records_banded": pair_sums(abufs, mf), "gapped_reads": int(abufs[1]["gapped"].sum())})
        out["b_place_pairs_vs_align_pairs_ms"] = leg
    if "c" in only:
        L = mf.load()
        precs, arecs, unplaced = np.zeros(R, mf.PLACE_RECORD), np.zeros(R, mf.ALIGN_RECORD), np.zeros(2, np.uint64)

        def two_single():
            for r in (r1, r2):
                mf._chk(L.mf_align(ks._h, r._h, 1, mf.MODE_SCREENED, 1, 1000, 0, a.band, None, None, None, None, None, precs.ctypes.data, None, None, None, None,
                                   arecs.ctypes.data, unplaced.ctypes.data, None))
        leg = compared(*alternately(two_single, aligned_pair_call(mf, ks, r1, r2, lo, hi, a.band, 0, abufs), a.reps))          # ("parent": the two single passes)
        leg.pop("inside_parent_range")
        out["c_two_align_passes_vs_align_pairs_no_rescue_ms"] = leg
    for r in (r1, r2, p1, p2):
        r.close()
    ks.close(); pks.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
