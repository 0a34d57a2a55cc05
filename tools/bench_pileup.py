#!/usr/bin/env python3
"""Cost of the pile-up (mf_pileup, mf_filter_fastq_files_pileup) next to read placement; prints one JSON object.

  headline     mf_filter, mf_place and mf_pileup, ms a pass in one process, on bench.py's resident set (33.3 M x 150 b, 0.5 % bait reads,
               k = 31) and its 16.5 kbp one-record bait.  Neither call copies a per-position array back (mf_place: record summaries
               and unplaced; mf_pileup: record summaries and unplaced); they are taken alternately and `pileup_over_place` is the ratio
               of their medians.  mf_pileup is also run with the per-position outputs (17 bytes a position: `ms_pileup_with_outputs`).
               The yardstick is mf_place: the pile-up adds one atomic per base to a pass that already reads the read once.
  eight        the same reads against the 8-record, ~132 kbp bait of tools/bench_assign.py
  stacked      a read set of --stacked reads that all lie on one start and its reverse (amplicon data): every wave adds to the same
               150 x 4 counters
  files        filter_fastq_files against filter_fastq_files_pileup, wall seconds, median of 5 warm calls, on a ~2 M-pair PE set from
               tools/make_fastq.py compressed with tools/pgzip.py
  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (the program after `--`): place_kernel (its
  PILE instance: the second template argument is true), pileup_call_kernel.

    python tools/bench_pileup.py [--reads N] [--pairs N] [--reps 10] [--no-files] [--only headline,eight,stacked]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter(); fn()
    return (time.perf_counter() - t0) * 1e3


def per_pass(fn, reps):
    fn(); fn()
    return statistics.median(timed(fn) for _ in range(reps))


def passes(mf, ks, reads, reps, min_depth=3):
    L = mf.load()
    st = mf.FilterStats()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    precs = np.zeros(max(R, 1), mf.PLACE_RECORD)
    urecs = np.zeros(max(R, 1), mf.PILEUP_RECORD)
    pile = np.zeros(max(P, 1), mf.PILEUP)
    cons = np.zeros(max(P, 1), np.uint8)
    unplaced = np.zeros(2, np.uint64)
    f = lambda: mf._chk(L.mf_filter(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, C.byref(st)))
    p = lambda: mf._chk(L.mf_place(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, None, precs.ctypes.data, unplaced.ctypes.data, None))
    u = lambda: mf._chk(L.mf_pileup(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, None, None, None, urecs.ctypes.data, unplaced.ctypes.data, None))
    uo = lambda: mf._chk(L.mf_pileup(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, None, pile.ctypes.data, cons.ctypes.data, urecs.ctypes.data,
                                     unplaced.ctypes.data, None))
    out = {"tables_ms_with_first_call": round(timed(u), 2)}
    ms_f = per_pass(f, reps)
    p(); p(); u(); u()
    tp, tu = [], []
    for _ in range(reps):          # alternately, so that a drift of the box touches both alike
        tp.append(timed(p)); tu.append(timed(u))
    ms_p, ms_u = statistics.median(tp), statistics.median(tu)
    ms_uo = per_pass(uo, max(reps // 2, 3))
    out.update({"records": R, "positions": P, "n_pass": int(st.n_pass), "min_depth": min_depth, "ms_filter": round(ms_f, 4), "ms_place": round(ms_p, 4),
                "ms_pileup": round(ms_u, 4), "pileup_over_place": round(ms_u / ms_p, 3), "ms_pileup_minus_place": round(ms_u - ms_p, 4),
                "ms_place_spread": [round(min(tp), 4), round(max(tp), 4)], "ms_pileup_spread": [round(min(tu), 4), round(max(tu), 4)],
                "ms_pileup_with_outputs": round(ms_uo, 4), "output_bytes": P * (mf.PILEUP.itemsize + 1),
                "bases": int(urecs["bases"].sum()), "placed_base_sum": int(precs["base_sum"].sum()),
                "called": int(urecs["called"].sum()), "ambiguous": int(urecs["ambiguous"].sum()), "variants": int(urecs["variants"].sum()),
                "mismatch_share": round(float(urecs["mismatches"].sum()) / max(float(urecs["bases"].sum()), 1.0), 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--stacked", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--only", default="headline,eight,stacked")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    from tools.bench_assign import mutated
    out = {}
    tmp = tempfile.mkdtemp(prefix="bench_pileup_")
    if not a.no_files:          # (inputs made before this process touches the GPU)
        prefix = os.path.join(tmp, "pe")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), prefix, "--pairs", str(a.pairs)])
        for m in ("1", "2"):
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "pgzip.py"), "%s_%s.fq" % (prefix, m), "%s_%s.fq.gz" % (prefix, m), "--procs", "16"])
            os.unlink("%s_%s.fq" % (prefix, m))
    bait = make_bait()
    g = bait_records(bait)[0]
    ks = mf.KmerSet.from_text(bait, 31)
    if only & {"headline", "eight"}:
        reads = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
        if "headline" in only:
            out["headline"] = passes(mf, ks, reads, a.reps)
        if "eight" in only:
            eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
            ks8 = mf.KmerSet.from_text(eight, 31)
            out["eight"] = passes(mf, ks8, reads, a.reps)
            ks8.close()
        reads.close()
    if "stacked" in only:
        # every read the same 150 bases of the bait (or their reverse complement): packed on the host, 2 bits a base
        code = {"A": 0, "C": 1, "G": 2, "T": 3}
        fwd = np.array([code[c] for c in g[4000:4150].upper()], np.uint64)
        both = np.concatenate([fwd, 3 - fwd[::-1]])
        n = a.stacked - a.stacked % 2
        bases = np.tile(both, n // 2)
        pad = (-bases.size) % 16
        bases = np.concatenate([bases, np.zeros(pad, np.uint64)]).reshape(-1, 16)
        words = (bases << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
        offsets = np.arange(n + 1, dtype=np.uint64) * 150
        stacked = mf.Reads.from_packed(words, offsets, np.zeros(0, np.uint64))
        out["stacked"] = passes(mf, ks, stacked, a.reps)
        stacked.close()
    if not a.no_files:
        f1, f2 = prefix + "_1.fq.gz", prefix + "_2.fq.gz"
        o1, o2 = os.path.join(tmp, "o1.fq"), os.path.join(tmp, "o2.fq")

        def t(fn, n=5):
            fn()
            v = []
            for _ in range(n):
                t0 = time.perf_counter(); fn(); v.append(time.perf_counter() - t0)
            return statistics.median(v), min(v), max(v)
        s_f = t(lambda: mf.filter_fastq_files(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER))
        path = mf.last_ingest_stats()["path"]
        s_p = t(lambda: mf.filter_fastq_files_placed(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER))
        s_u = t(lambda: mf.filter_fastq_files_pileup(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER, min_depth=3))
        out["files"] = {"pairs": a.pairs, "s_filter": round(s_f[0], 4), "s_placed": round(s_p[0], 4), "s_pileup": round(s_u[0], 4),
                        "pileup_over_filter": round(s_u[0] / s_f[0], 3),
                        "s_filter_spread": [round(s_f[1], 4), round(s_f[2], 4)], "s_pileup_spread": [round(s_u[1], 4), round(s_u[2], 4)],
                        "path": "device" if path == 1 else "host", "same_path": mf.last_ingest_stats()["path"] == path}
    ks.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
