#!/usr/bin/env python3
"""Cost of the paired call (mf_place_pairs) next to two mf_verify passes of the PARENT commit, and of the rescue itself; prints one JSON
object.

The two libraries run in ONE process, as in tools/bench_extend.py: this tree's through mitoflex_amd.mitofilter, the parent's through the
mitofilter.py of a checkout of the parent commit whose library is built (--parent-root DIR).  Each builds its own k-mer set and its own
read sets from the same seeds.  Every leg takes its two sides alternately, --reps (5) runs a side, ms a call; record summaries, the pair
records and unplaced only, no pile-up.

  a   bench.py's resident set (33.3 M x 150 b, 0.5 % bait reads, k = 31) split into two mate sets of half the reads: the PARENT
      library's two mf_verify passes against this build's mf_place_pairs(rescue = 0).  The expectation: the change's median inside the
      parent's own min .. max plus what pair_list_kernel reads (48 bytes a pair, `pair_list_bytes`); a miss is reported as one.
  b   --pairs (200 k) pairs of 150-base mates drawn from the bait's first record, whose sample differs every 20 bases along
      --diverged-share (10 %) of its length: the mates that lie there draw no vote.  This build at rescue = 0 against rescue = 1 with a
      window of --window (400) inserts.  Stated as measured, no bar.

    python tools/bench_pairs.py --parent-root DIR [--reads N] [--reps 5] [--pairs N] [--window W] [--only a,b]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_verify import alternately, compared, load_parent  # noqa: E402


def paired_call(mf, ks, r1, r2, lo, hi, rescue, bufs):
    L = mf.load()
    precs, srecs, prs, none, unplaced = bufs
    return lambda: mf._chk(L.mf_place_pairs(ks._h, r1._h, r2._h, 1, mf.MODE_SCREENED, 1, 1000, lo, hi, rescue, 100, None, None, None, None, None, None, None,
                                            None, precs.ctypes.data, None, None, None, srecs.ctypes.data, prs.ctypes.data, none.ctypes.data_as(C.POINTER(C.c_uint64)), unplaced.ctypes.data, None))


def pack(codes):
    """2-bit codes, one read a row -> (words u32, offsets u64, no invalid positions) as Reads.from_packed takes them"""
    n, L = codes.shape
    flat = codes.reshape(-1).astype(np.uint32)
    pad = (-flat.size) % 16
    flat = np.concatenate([flat, np.zeros(pad, np.uint32)]).reshape(-1, 16)
    words = (flat << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([words, np.zeros(8, np.uint32)]), np.arange(n + 1, dtype=np.uint64) * L, np.zeros(0, np.uint64)


def drawn_pairs(g, n, share, seed):
    """n pairs of 150-base mates out of record text g: inserts 300 .. 500, the sample differing every 20 bases along the last `share` of
    g -> (codes1, codes2, the share of pairs with a mate that lies wholly in that stretch)"""
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(g.encode(), np.uint8)
    code = np.zeros(256, np.uint8)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    sample = code[ref].copy()
    first = int(len(g) * (1.0 - share))
    at = np.arange(first + 7, len(g), 20)
    sample[at] = (sample[at] + 1) & 3
    ins = rng.integers(300, 501, n)
    a = rng.integers(0, len(g) - 500, n)
    idx1 = a[:, None] + np.arange(150)[None, :]
    idx2 = (a + ins)[:, None] - 1 - np.arange(150)[None, :]          # the reverse mate, read from the fragment's far end
    return sample[idx1], 3 - sample[idx2], float(np.mean(a + ins - 150 >= first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--diverged-share", type=float, default=0.10)
    ap.add_argument("--only", default="a,b")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    pf = load_parent(a.parent_root)
    bait = make_bait()
    ks, pks = mf.KmerSet.from_text(bait, 31), pf.KmerSet.from_text(bait, 31)
    R = len(ks.record_starts) - 1
    bufs = [np.zeros(max(R, 1), mf.PLACE_RECORD), np.zeros(max(R, 1), mf.SCORE_RECORD), np.zeros(max(R, 1), mf.PAIR_RECORD), np.zeros(1, np.uint64),
            np.zeros(2, np.uint64)]
    out = {}
    if "a" in only:
        half = a.reads // 2
        synth = dict(bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
        sets = [mf.Reads.synth(half, 150, seed=20261003 + m, **synth) for m in (0, 1)]
        psets = [pf.Reads.synth(half, 150, seed=20261003 + m, **synth) for m in (0, 1)]
        PL = pf.load()
        pprecs, psrecs, punpl = np.zeros(max(R, 1), pf.PLACE_RECORD), np.zeros(max(R, 1), pf.SCORE_RECORD), np.zeros(2, np.uint64)
        sums = {}

        def parent_two():
            tot = np.zeros(2, np.uint64)
            acc = 0
            for r in psets:
                pf._chk(PL.mf_verify(pks._h, r._h, 1, pf.MODE_SCREENED, 1, 1000, None, None, None, None, pprecs.ctypes.data, None, None, None, psrecs.ctypes.data,
                                     punpl.ctypes.data, None))
                tot += punpl
                acc += int(psrecs["accepted"].sum())
            sums["parent"] = (acc, tot.tolist())
        change = paired_call(mf, ks, sets[0], sets[1], 200, 600, 0, bufs)
        tp, tc = alternately(parent_two, change, a.reps)
        leg = compared(tp, tc)
        leg.update({"pairs": half, "pair_list_bytes": 48 * half, "same_accepted_and_unplaced_as_parent": sums["parent"] == (int(bufs[1]["accepted"].sum()), bufs[4].tolist()),
                    "pair_records": {f: int(bufs[2][f].sum()) for f in mf.PAIR_RECORD.names}, "pairs_none": int(bufs[3][0])})
        out["a_two_parent_verify_vs_place_pairs_no_rescue_ms"] = leg
        for r in sets + psets:
            r.close()
    if "b" in only:
        g = bait_records(bait)[0]
        c1, c2, share = drawn_pairs(g, a.pairs, a.diverged_share, 7)
        r1, r2 = mf.Reads.from_packed(*pack(c1)), mf.Reads.from_packed(*pack(c2))
        lo, hi = 400 - a.window // 2 + 1, 400 + a.window // 2
        off, on = paired_call(mf, ks, r1, r2, lo, hi, 0, bufs), paired_call(mf, ks, r1, r2, lo, hi, 1, bufs)
        t0, t1 = alternately(off, on, a.reps)
        leg = compared(t0, t1)          # ("parent" is this build at rescue = 0 here)
        leg.pop("inside_parent_range")
        on()
        leg.update({"pairs": a.pairs, "window": [lo, hi], "share_of_pairs_with_a_diverged_mate": round(share, 4),
                    "pair_records": {f: int(bufs[2][f].sum()) for f in mf.PAIR_RECORD.names}, "pairs_none": int(bufs[3][0])})
        out["b_no_rescue_vs_rescue_ms"] = leg
        r1.close(); r2.close()
    ks.close(); pks.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
