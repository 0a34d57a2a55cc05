#!/usr/bin/env python3
"""Cost of record assignment (mf_assign, mf_filter_fastq_files_by_record) next to the filter alone; prints one JSON object.

  headline     mf_filter against mf_assign, ms a pass, on bench.py's resident set (33.3 M x 150 b, 0.5 % bait reads, k = 31) and its
               16.5 kbp one-record bait
  eight        the same reads against an 8-record, ~132 kbp bait (the mitogenome and seven copies mutated at 2 .. 14 %)
  lookups      table look-ups the assign kernel makes on the headline set (key + owner per window of a passing read), and that count
               over the extra time an assign pass takes (an upper bound of the kernel's own time: a rocprofv3 --kernel-trace --stats run
               gives the kernel alone) as a fraction of the 265 G/s gather roof of tools/gather_roof.hip
  files        filter_fastq_files against filter_fastq_files_by_record, wall seconds, median of 5 warm calls, on a ~2 M-pair PE set from
               tools/make_fastq.py compressed with tools/pgzip.py

    python tools/bench_assign.py [--reads N] [--pairs N] [--reps 20] [--no-files]
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


def mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    s = np.frombuffer(seq.encode(), dtype=np.uint8).copy()
    at = np.nonzero(rng.random(len(s)) < rate)[0]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in at:
        s[i] = acgt[(int(np.nonzero(acgt == s[i])[0][0]) + int(rng.integers(1, 4))) % 4] if s[i] in acgt else s[i]
    return s.tobytes().decode()


def per_pass(fn, reps):
    fn(); fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def pair_of_passes(mf, ks, reads, reps):
    L = mf.load()
    n_rec = len(ks.record_names)
    counts = np.zeros(n_rec + 2, dtype=np.uint64)
    st = mf.FilterStats()
    f = lambda: mf._chk(L.mf_filter(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, C.byref(st)))
    a = lambda: mf._chk(L.mf_assign(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, counts.ctypes.data, None))
    ms_f, ms_a = per_pass(f, reps), per_pass(a, reps)
    return {"ms_filter": round(ms_f, 4), "ms_assign": round(ms_a, 4), "ratio": round(ms_a / ms_f, 3), "n_pass": int(st.n_pass),
            "records": n_rec, "counts_head": [int(x) for x in counts[:min(n_rec, 8)]], "ambiguous": int(counts[n_rec]), "unassigned": int(counts[n_rec + 1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-files", action="store_true")
    a = ap.parse_args()
    from mitoflex_amd import mitofilter as mf
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    out = {}
    tmp = tempfile.mkdtemp(prefix="bench_assign_")
    if not a.no_files:          # (inputs made before this process touches the GPU)
        prefix = os.path.join(tmp, "pe")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), prefix, "--pairs", str(a.pairs)])
        for m in ("1", "2"):
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "pgzip.py"), "%s_%s.fq" % (prefix, m), "%s_%s.fq.gz" % (prefix, m), "--procs", "16"])
            os.unlink("%s_%s.fq" % (prefix, m))
    bait = make_bait()
    reads = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
    ks = mf.KmerSet.from_text(bait, 31)
    t0 = time.perf_counter()
    mf.assign_reads(ks, mf.Reads.synth(1000, 150, seed=1, bait_text=bait), 1)
    out["owner_table_build_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["headline"] = pair_of_passes(mf, ks, reads, a.reps)
    h = out["headline"]
    looks = h["n_pass"] * (150 - 31 + 1) * 2
    extra_s = max(h["ms_assign"] - h["ms_filter"], 1e-6) / 1e3
    out["lookups"] = {"lookups": looks, "per_s_upper_bound_time": looks / extra_s, "fraction_of_gather_roof": round(looks / extra_s / GATHER_ROOF, 4),
                      "note": "time = assign pass minus filter pass (pass list, kernel, counter copy); the kernel alone comes from rocprofv3"}
    g = bait_records(bait)[0]
    eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
    ks8 = mf.KmerSet.from_text(eight, 31)
    out["eight"] = pair_of_passes(mf, ks8, reads, a.reps)
    out["eight"]["bait_bases"] = sum(len(r) for r in bait_records(eight))
    reads.close()
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
        s_a = t(lambda: mf.filter_fastq_files_by_record(ks, f1, f2, o1, o2, 1, mf.PAIR_EITHER))
        out["files"] = {"pairs": a.pairs, "s_filter": round(s_f, 4), "s_by_record": round(s_a, 4), "ratio": round(s_a / s_f, 3),
                        "path": "device" if path == 1 else "host", "same_path": mf.last_ingest_stats()["path"] == path}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
