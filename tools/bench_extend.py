#!/usr/bin/env python3
"""Cost of the extension pile (mf_align_extended) next to mf_align_gapped, and a control that the extended entry point at extend == 0
costs what the PARENT commit's mf_align_gapped does; prints one JSON object.

The two libraries run in ONE process, as in tools/bench_gapped.py: this tree's through mitoflex_amd.mitofilter, the parent's through the
mitofilter.py of a checkout of the parent commit whose library is built (--parent-root DIR).  Each builds its own k-mer set and its own
read set from the same seed.  Every leg takes its two sides alternately, --reps (5) runs a side, ms a pass, on bench.py's resident set
(33.3 M x 150 b, 0.5 % bait reads, k = 31), band 8, cut 1000, the pile-up on, record summaries and unplaced only.

  a        the PARENT library's mf_align_gapped against this build's mf_align_extended at extend == 0 (the same kernels): the change's
           median should lie inside the parent's own min .. max (`inside_parent_range`); a miss is reported as one.
  b        this build at extend == 0 against extend = 64 and extend = 4096, asked for the extend record summaries alone -- the pile, the
           clamped table and the emitted bytes stay on the device or in the report: what zeroing 2 * E * 4 words a record, one atomic an
           overhanging base and the call kernel cost.  Stated as measured, no bar.
  stacked  leg b on --stack-reads (2 M) copies of ONE 160-base read of which 64 bases hang over the end of the 16.5 kbp record: every
           wave adds to the same 64 counters.  Stated as measured, no bar.
`headline`: the 16.5 kbp one-record bait; `eight`: the 8-record, ~132 kbp bait of tools/bench_assign.py.

    python tools/bench_extend.py --parent-root DIR [--reads N] [--reps 5] [--band 8] [--only headline,eight,stacked] [--load-first parent|change]
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


def extended_call(mf, ks, reads, band, min_depth, E, bufs):
    """mf_align_extended asked for the record summaries alone: the gapped ones at E == 0, the extend ones otherwise"""
    L = mf.load()
    precs, urecs, arecs, grecs, xrecs, unplaced = bufs
    return lambda: mf._chk(L.mf_align_extended(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, mf.KEEP_PASSING, band, E, None, None, None, None, None,
                                               precs.ctypes.data, None, None, urecs.ctypes.data, None, arecs.ctypes.data, None, None, None, grecs.ctypes.data,
                                               None, None, None, xrecs.ctypes.data if E else None, unplaced.ctypes.data, None))


def buffers(mf, R):
    return [np.zeros(max(R, 1), d) for d in (mf.PLACE_RECORD, mf.PILEUP_RECORD, mf.ALIGN_RECORD, mf.GAPPED_RECORD, mf.EXTEND_RECORD)] + [np.zeros(2, np.uint64)]


def leg_b(mf, ks, reads, reps, band, min_depth):
    R = len(ks.record_starts) - 1
    bufs = buffers(mf, R)
    zero = extended_call(mf, ks, reads, band, min_depth, 0, bufs)
    out = {}
    for E in (64, 4096):
        t0, te = alternately(zero, extended_call(mf, ks, reads, band, min_depth, E, bufs), reps)
        leg = compared(t0, te)          # ("parent" is this build at extend == 0 here)
        leg.pop("inside_parent_range")
        leg["extension_pile_bytes"] = 4 * 2 * E * R * 8
        leg["extend_records"] = {f: int(bufs[4][f].sum()) for f in mf.EXTEND_RECORD.names}
        out["E%d" % E] = leg
    return out


def legs(mf, ks, reads, pf, pks, preads, reps, band, min_depth=3):
    """mf, ks, reads: this tree's; pf, pks, preads: the parent's"""
    PL = pf.load()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    bufs = buffers(mf, R)
    pprecs, purecs, parecs, pgrecs = (np.zeros(max(R, 1), d) for d in (pf.PLACE_RECORD, pf.PILEUP_RECORD, pf.ALIGN_RECORD, pf.GAPPED_RECORD))
    punplaced = np.zeros(2, np.uint64)
    pgapped = lambda: pf._chk(PL.mf_align_gapped(pks._h, preads._h, 1, pf.MODE_SCREENED, min_depth, 1000, pf.KEEP_PASSING, band, None, None, None, None, None,
                                                 pprecs.ctypes.data, None, None, purecs.ctypes.data, None, parecs.ctypes.data, None, None, None, pgrecs.ctypes.data,
                                                 punplaced.ctypes.data, None))
    zero = extended_call(mf, ks, reads, band, min_depth, 0, bufs)
    out = {"records": R, "positions": P, "band": band, "min_depth": min_depth, "tables_ms_with_first_call": round(timed(zero) * 1e3, 2)}
    tp, tc = alternately(pgapped, zero, reps)
    out["a_extended_at_0_vs_parent_gapped_ms"] = compared(tp, tc)
    out["same_records_as_parent"] = bool(all(np.array_equal(bufs[2][f], parecs[f]) for f in pf.ALIGN_RECORD.names)
                                         and all(np.array_equal(bufs[3][f], pgrecs[f]) for f in pf.GAPPED_RECORD.names))
    out["align"] = {f: int(bufs[2][f].sum()) for f in SUMS}
    out["b_extend_vs_extend_0_ms"] = leg_b(mf, ks, reads, reps, band, min_depth)
    return out


def stacked_reads(mf, record, n, seed=20261020):
    """n copies of one 160-base read -- the record's last 96 bases and 64 random ones behind them -- packed sixteen bases a word"""
    rng = np.random.default_rng(seed)
    code = np.full(256, 0, np.uint32)
    code[list(b"ACGT")] = range(4)
    letters = np.concatenate([code[np.frombuffer(record[-96:].encode(), np.uint8)], rng.integers(0, 4, 64).astype(np.uint32)])
    one = (letters.reshape(10, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    return mf.Reads.from_packed(np.tile(one, n), np.arange(n + 1, dtype=np.uint64) * 160, np.zeros(0, np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--stack-reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--only", default="headline,eight,stacked")
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
    out = {"loaded_first": a.load_first}
    if only & {"headline", "eight"}:
        reads, preads = mf.Reads.synth(a.reads, 150, **synth), pf.Reads.synth(a.reads, 150, **synth)
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
    if "stacked" in only:
        ks = mf.KmerSet.from_text(">mito\n%s\n" % g, 31)
        stack = stacked_reads(mf, g, a.stack_reads)
        out["stacked"] = {"reads": a.stack_reads, "b_extend_vs_extend_0_ms": leg_b(mf, ks, stack, a.reps, a.band, 3)}
        stack.close(); ks.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
