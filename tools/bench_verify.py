#!/usr/bin/env python3
"""Cost of verifying the placed reads (mf_verify, mf_filter_fastq_files_verified) next to the PARENT commit's pile-up; prints one JSON
object.

The two libraries run in ONE process: this tree's through mitoflex_amd.mitofilter, the parent's through the mitofilter.py of a
checkout of the parent commit whose library is built (--parent-root DIR: DIR/mitoflex_amd/mitofilter.py and
DIR/mitoflex_amd/libmitofilter_hip.so).  Each builds its own k-mer set and its own read set from the same seed.

  headline     an mf_verify pass at 1000 permille (pile-up on, record summaries and unplaced only: no per-read or per-position array is
               copied back) against an mf_pileup pass of the parent's library with the same outputs, on bench.py's resident set
               (33.3 M x 150 b, 0.5 % bait reads, k = 31) and its 16.5 kbp one-record bait; the two are taken alternately, --reps (5)
               runs a side, ms a pass.  `inside_parent_range`: the change's median lies inside the parent's own min .. max.
               Also mf_verify without the pile (`ms_verify_no_pile`) and this tree's own mf_pileup (`ms_pileup_here`: the untouched
               instantiation, a control).
               Where the parent's library has mf_verify itself: this tree's mf_verify against the parent's, with and without the pile
               (`verify_vs_parent_verify_ms`, `verify_no_pile_vs_parent_verify_ms`) -- what a change to the verifying kernel is held
               to.  Where this tree's library has mf_verify_keep: a pass at MF_KEEP_ACCEPTED and a cut of 30 (no keep_bits copied
               back) against mf_verify at the same cut, both of THIS build (`keep_accepted_vs_verify_cut30_ms`; its "parent" side is
               mf_verify).
  eight        the same against the 8-record, ~132 kbp bait of tools/bench_assign.py
  files        filter_fastq_files_pileup of the parent against filter_fastq_files_verified at 1000 permille, wall seconds, alternately,
               5 warm calls a side, on a ~2 M-pair PE set from tools/make_fastq.py compressed with tools/pgzip.py
  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (the program after `--`): place_kernel, whose
  third template argument is true in the verifying instantiations.

    python tools/bench_verify.py --parent-root DIR [--reads N] [--pairs N] [--reps 5] [--no-files] [--only headline,eight]
"""
import argparse
import ctypes as C
import importlib.util
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
    return time.perf_counter() - t0


def alternately(fa, fb, reps):
    """fa and fb warmed twice, then taken alternately reps times a side (a drift of the machine touches both alike) -> two lists"""
    for f in (fa, fb, fa, fb):
        f()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa)); tb.append(timed(fb))
    return ta, tb


def side(v, scale, digits):
    return {"median": round(statistics.median(v) * scale, digits), "min": round(min(v) * scale, digits), "max": round(max(v) * scale, digits),
            "runs": [round(x * scale, digits) for x in v]}


def compared(parent, change, scale=1e3, digits=4):
    p, c = side(parent, scale, digits), side(change, scale, digits)
    return {"parent": p, "change": c, "change_over_parent": round(c["median"] / p["median"], 4),
            "inside_parent_range": p["min"] <= c["median"] <= p["max"]}


def load_parent(root):
    spec = importlib.util.spec_from_file_location("mitofilter_parent", os.path.join(root, "mitoflex_amd", "mitofilter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.load(os.path.join(root, "mitoflex_amd", "libmitofilter_hip.so"))
    return mod


def passes(mf, ks, reads, pf, pks, preads, reps, min_depth=3):
    """mf, ks, reads: this tree's; pf, pks, preads: the parent's"""
    L, PL = mf.load(), pf.load()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    precs, urecs, srecs = np.zeros(max(R, 1), mf.PLACE_RECORD), np.zeros(max(R, 1), mf.PILEUP_RECORD), np.zeros(max(R, 1), mf.SCORE_RECORD)
    purecs = np.zeros(max(R, 1), pf.PILEUP_RECORD)
    unplaced, punplaced = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    pu = lambda: pf._chk(PL.mf_pileup(pks._h, preads._h, 1, pf.MODE_SCREENED, min_depth, None, None, None, purecs.ctypes.data, punplaced.ctypes.data, None))
    u = lambda: mf._chk(L.mf_pileup(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, None, None, None, urecs.ctypes.data, unplaced.ctypes.data, None))

    def verify(pile):
        return lambda: mf._chk(L.mf_verify(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 1000, None, None, None, None, precs.ctypes.data, None, None,
                                           urecs.ctypes.data if pile else None, srecs.ctypes.data, unplaced.ctypes.data, None))
    out = {"records": R, "positions": P, "min_depth": min_depth, "tables_ms_with_first_call": round(timed(verify(True)) * 1e3, 2)}
    tp, tv = alternately(pu, verify(True), reps)
    out["verify_vs_parent_pileup_ms"] = compared(tp, tv)
    same = all(np.array_equal(urecs[f], purecs[f]) for f in pf.PILEUP_RECORD.names) and unplaced.tolist() == punplaced.tolist()
    out.update({"same_pileup_records_as_parent": bool(same), "accepted": int(srecs["accepted"].sum()), "rejected": int(srecs["rejected"].sum()),
                "compared": int(srecs["compared"].sum()), "mismatches": int(srecs["mismatches"].sum()), "unplaced": unplaced.tolist(),
                "hist": [int(x) for x in srecs["hist"].sum(axis=0)]})
    tp, tn = alternately(pu, verify(False), reps)
    out["verify_no_pile_vs_parent_pileup_ms"] = compared(tp, tn)
    tp, th = alternately(pu, u, reps)
    out["pileup_here_vs_parent_pileup_ms"] = compared(tp, th)
    if hasattr(PL, "mf_verify"):
        pprecs, psrecs = np.zeros(max(R, 1), pf.PLACE_RECORD), np.zeros(max(R, 1), pf.SCORE_RECORD)

        def pverify(pile):
            return lambda: pf._chk(PL.mf_verify(pks._h, preads._h, 1, pf.MODE_SCREENED, min_depth, 1000, None, None, None, None, pprecs.ctypes.data, None, None,
                                                purecs.ctypes.data if pile else None, psrecs.ctypes.data, punplaced.ctypes.data, None))
        for pile, name in ((True, "verify_vs_parent_verify_ms"), (False, "verify_no_pile_vs_parent_verify_ms")):
            tp, tv = alternately(pverify(pile), verify(pile), reps)
            out[name] = compared(tp, tv)
        out["same_score_records_as_parent"] = bool(all(np.array_equal(srecs[f], psrecs[f]) for f in pf.SCORE_RECORD.names))
    if hasattr(L, "mf_verify_keep"):
        cut30 = lambda: mf._chk(L.mf_verify(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 30, None, None, None, None, precs.ctypes.data, None, None,
                                            urecs.ctypes.data, srecs.ctypes.data, unplaced.ctypes.data, None))
        keep30 = lambda: mf._chk(L.mf_verify_keep(ks._h, reads._h, 1, mf.MODE_SCREENED, min_depth, 30, mf.KEEP_ACCEPTED, None, None, None, None, None,
                                                  precs.ctypes.data, None, None, urecs.ctypes.data, srecs.ctypes.data, unplaced.ctypes.data, None))
        tv, tk = alternately(cut30, keep30, reps)
        out["keep_accepted_vs_verify_cut30_ms"] = compared(tv, tk)
        out["rejected_at_30"] = int(srecs["rejected"].sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--only", default="headline,eight")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    from tools.bench_assign import mutated
    out = {}
    tmp = tempfile.mkdtemp(prefix="bench_verify_")
    if not a.no_files:          # (inputs made before this process touches the GPU)
        prefix = os.path.join(tmp, "pe")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), prefix, "--pairs", str(a.pairs)])
        for m in ("1", "2"):
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "pgzip.py"), "%s_%s.fq" % (prefix, m), "%s_%s.fq.gz" % (prefix, m), "--procs", "16"])
            os.unlink("%s_%s.fq" % (prefix, m))
    pf = load_parent(a.parent_root)
    bait = make_bait()
    g = bait_records(bait)[0]
    ks, pks = mf.KmerSet.from_text(bait, 31), pf.KmerSet.from_text(bait, 31)
    if only & {"headline", "eight"}:
        synth = dict(seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
        reads, preads = mf.Reads.synth(a.reads, 150, **synth), pf.Reads.synth(a.reads, 150, **synth)
        if "headline" in only:
            out["headline"] = passes(mf, ks, reads, pf, pks, preads, a.reps)
        if "eight" in only:
            eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
            ks8, pks8 = mf.KmerSet.from_text(eight, 31), pf.KmerSet.from_text(eight, 31)
            out["eight"] = passes(mf, ks8, reads, pf, pks8, preads, a.reps)
            ks8.close(); pks8.close()
        reads.close(); preads.close()
    if not a.no_files:
        f1, f2 = prefix + "_1.fq.gz", prefix + "_2.fq.gz"
        o1, o2 = os.path.join(tmp, "o1.fq"), os.path.join(tmp, "o2.fq")
        res = {}
        fp = lambda: res.__setitem__("p", pf.filter_fastq_files_pileup(pks, f1, f2, o1, o2, 1, pf.PAIR_EITHER, min_depth=3))
        fv = lambda: res.__setitem__("v", mf.filter_fastq_files_verified(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER, min_depth=3, max_permille=1000))
        tp, tv = alternately(fp, fv, 5)
        v, p = res["v"], res["p"]
        out["files"] = {"pairs": a.pairs, "verified_vs_parent_pileup_s": compared(tp, tv, 1.0, 4),
                        "same_consensus_as_parent": bool(np.array_equal(v.consensus, p[3]) and np.array_equal(v.pileup, p[2])),
                        "kept": [int(v.kept), int(p[0])], "rejected": int(v.score_records["rejected"].sum()),
                        "path": "device" if mf.last_ingest_stats()["path"] == 1 else "host"}
    ks.close(); pks.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
