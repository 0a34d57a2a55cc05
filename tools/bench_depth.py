#!/usr/bin/env python3
"""Cost of k-mer depth (mf_depth, mf_filter_fastq_files_depth) next to the filter and record assignment; prints one JSON object.

  headline     mf_filter, mf_assign and mf_depth, ms a pass, on bench.py's resident set (33.3 M x 150 b, 0.5 % bait reads, k = 31) and its
               16.5 kbp one-record bait; also mf_depth with the counters indexed by table slot (depth_index=1: the scattered atomics) --
               the same results, measured against the representative-position counters
  eight        the same reads against the 8-record, ~132 kbp bait of tools/bench_assign.py
  lowcomplex   filter / depth on a set with mf_reads_synth_ex's microsatellite (2 %) and NUMT-like (0.5 %) reads
  protein      filter / depth on the generated 4 030-record protein clade of tools/bench_group_assign.py (kp = 9, code 5)
  files        filter_fastq_files against filter_fastq_files_depth, wall seconds, median of 5 warm calls, on a ~2 M-pair PE set from
               tools/make_fastq.py compressed with tools/pgzip.py
  The count kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script (depth_kernel).

    python tools/bench_depth.py [--reads N] [--pairs N] [--reps 10] [--no-files] [--only headline,eight,lowcomplex,protein]
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
GATHER_ROOF = 265e9


def per_pass(fn, reps):
    fn(); fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def passes(mf, ks, reads, reps, assign=True):
    """ms a pass of the filter, the assignment (nucleotide sets) and depth (records and profile copied back)"""
    L = mf.load()
    st = mf.FilterStats()
    starts = ks.record_starts
    R, P = len(starts) - 1, int(starts[-1])
    prof = np.zeros(max(P, 1), np.uint32)
    recs = np.zeros(max(R, 1), mf.DEPTH_RECORD)
    f = lambda: mf._chk(L.mf_filter(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, C.byref(st)))
    d = lambda: mf._chk(L.mf_depth(ks._h, reads._h, 1, mf.MODE_SCREENED, None, prof.ctypes.data, recs.ctypes.data, None))
    t0 = time.perf_counter()
    d()
    out = {"depth_tables_build_ms_with_first_call": round((time.perf_counter() - t0) * 1e3, 2)}
    ms_f, ms_d = per_pass(f, reps), per_pass(d, reps)
    out.update({"records": R, "positions": P, "n_pass": int(st.n_pass), "ms_filter": round(ms_f, 4), "ms_depth": round(ms_d, 4),
                "depth_over_filter": round(ms_d / ms_f, 3)})
    if assign:
        counts = np.zeros(R + 2, dtype=np.uint64)
        a = lambda: mf._chk(L.mf_assign(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, counts.ctypes.data, None))
        ms_a = per_pass(a, reps)
        out.update({"ms_assign": round(ms_a, 4), "depth_over_assign": round(ms_d / ms_a, 3)})
    out["mean_depth_head"] = [round(float(r["depth_sum"]) / max(int(r["windows"]), 1), 3) for r in recs[:min(R, 8)]]
    out["covered_fraction"] = round(float(recs["covered"].sum()) / max(float(recs["windows"].sum()), 1.0), 4)
    return out, prof, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--only", default="headline,eight,lowcomplex,protein")
    a = ap.parse_args()
    only = set(a.only.split(","))
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    from tools.bench_assign import mutated
    out = {}
    tmp = tempfile.mkdtemp(prefix="bench_depth_")
    if not a.no_files:          # (inputs made before this process touches the GPU)
        prefix = os.path.join(tmp, "pe")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), prefix, "--pairs", str(a.pairs)])
        for m in ("1", "2"):
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "pgzip.py"), "%s_%s.fq" % (prefix, m), "%s_%s.fq.gz" % (prefix, m), "--procs", "16"])
            os.unlink("%s_%s.fq" % (prefix, m))
    bait = make_bait()
    ks = mf.KmerSet.from_text(bait, 31)
    if only & {"headline", "eight"}:
        reads = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
        if "headline" in only:
            h, prof, recs = passes(mf, ks, reads, a.reps)
            windows = h["n_pass"] * (150 - 31 + 1)
            h["lookups"] = windows * 2
            h["atomic_bytes_if_coalesced"] = windows * 4
            mf.set_option("depth_index", 1)
            try:
                ks_slot = mf.KmerSet.from_text(bait, 31)
            finally:
                mf.set_option("depth_index", 0)
            s, sprof, srecs = passes(mf, ks_slot, reads, a.reps, assign=False)
            h["ms_depth_by_slot"] = s["ms_depth"]
            h["by_slot_same_results"] = bool(np.array_equal(prof, sprof) and np.array_equal(recs, srecs))
            ks_slot.close()
            out["headline"] = h
        if "eight" in only:
            g = bait_records(bait)[0]
            eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
            ks8 = mf.KmerSet.from_text(eight, 31)
            out["eight"], _, _ = passes(mf, ks8, reads, a.reps)
            ks8.close()
        reads.close()
    if "lowcomplex" in only:
        lc = mf.Reads.synth(a.reads, 150, seed=20261004, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000,
                            msat_ppm=20000, numt_ppm=5000)
        out["lowcomplex"], _, _ = passes(mf, ks, lc, a.reps, assign=False)
        lc.close()
    if "protein" in only:
        from tests.clade_data import GENES, Clade, gene_dna
        clade = Clade(n_species=310, seed=7)
        dna = gene_dna(clade.unseen(0.06, seed=8), 5, seed=9)
        gene_fa = "".join(">%s\n%s\n" % (g, dna[g]) for g in GENES)
        pr = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=gene_fa)
        kp = mf.KmerSet.protein_from_text(clade.text, 9, 5)
        out["protein"], _, _ = passes(mf, kp, pr, a.reps, assign=False)
        pr.close(); kp.close()
    if not a.no_files:
        f1, f2 = prefix + "_1.fq.gz", prefix + "_2.fq.gz"
        o1, o2 = os.path.join(tmp, "o1.fq"), os.path.join(tmp, "o2.fq")

        def t(fn, n=5):
            fn()
            v = []
            for _ in range(n):
                t0 = time.perf_counter(); fn(); v.append(time.perf_counter() - t0)
            return statistics.median(v)
        s_f = t(lambda: mf.filter_fastq_files(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER))
        path = mf.last_ingest_stats()["path"]
        s_d = t(lambda: mf.filter_fastq_files_depth(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER))
        out["files"] = {"pairs": a.pairs, "s_filter": round(s_f, 4), "s_depth": round(s_d, 4), "ratio": round(s_d / s_f, 3),
                        "path": "device" if path == 1 else "host", "same_path": mf.last_ingest_stats()["path"] == path}
    ks.close()
    out["gather_roof_per_s"] = GATHER_ROOF
    print(json.dumps(out))


if __name__ == "__main__":
    main()
