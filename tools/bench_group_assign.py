#!/usr/bin/env python3
"""Cost of group assignment (mf_assign_groups) next to the filter alone and to record assignment; prints one JSON object.

  protein      mf_filter against mf_assign_groups, ms a pass, on 33.3 M x 150 b reads (tools/bench_protein.py's shape: 0.5 % of them
               sampled from gene DNA of a species the set does not hold) against a generated clade of ~4 000 records (~1.2 M
               residues, tests/clade_data.py), kp = 9, code 5, grouped by gene; the one-time group-owner build
  headline     mf_assign against mf_assign_groups under the identity grouping and under a field grouping, on bench.py's resident set
               (33.3 M x 150 b, k = 31) and its 16.5 kbp one-record bait
  eight        the same on the 8-record bait of tools/bench_assign.py (the mitogenome and seven copies mutated at 2 .. 14 %)
  The assign kernel alone: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_group_assign.py --only protein`.

    python tools/bench_group_assign.py [--reads N] [--reps 20] [--only protein|nucleotide]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_pass(fn, reps):
    fn(); fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def protein(mf, a):
    from tests.clade_data import GENES, Clade, gene_dna
    clade = Clade(n_species=310, seed=7)
    dna = gene_dna(clade.unseen(0.06, seed=8), 5, seed=9)
    gene_fa = "".join(">%s\n%s\n" % (g, dna[g]) for g in GENES)
    reads = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=gene_fa)
    ks = mf.KmerSet.protein_from_text(clade.text, 9, 5)
    ks.group_records("_", 4)
    L = mf.load()
    G = len(ks.group_names)
    t0 = time.perf_counter()
    mf.assign_groups(ks, mf.Reads.synth(1000, 150, seed=1, bait_text=gene_fa), 1)
    build_ms = (time.perf_counter() - t0) * 1e3
    counts = np.zeros(G + 2, dtype=np.uint64)
    st = mf.FilterStats()
    f = lambda: mf._chk(L.mf_filter(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, C.byref(st)))
    g = lambda: mf._chk(L.mf_assign_groups(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, counts.ctypes.data, None))
    ms_f, ms_g = per_pass(f, a.reps), per_pass(g, a.reps)
    out = {"records": len(clade.records), "residues": sum(len(r[3]) for r in clade.records), "keys": int(ks.info.n_keys), "groups": G,
           "group_owner_build_ms_with_first_call": round(build_ms, 2), "ms_filter": round(ms_f, 4), "ms_assign_groups": round(ms_g, 4),
           "ratio": round(ms_g / ms_f, 3), "n_pass": int(st.n_pass), "windows": int(st.n_pass) * 2 * (150 - 27 + 1),
           "gene_reads": {n: int(c) for n, c in zip(ks.group_names, counts[:G])}, "ambiguous": int(counts[G]), "unassigned": int(counts[G + 1])}
    reads.close(); ks.close()
    return out


def nucleotide(mf, a):
    from mitoflex_amd.utility.synth_bait import bait_records, make_bait
    from tools.bench_assign import mutated
    bait = make_bait()
    reads = mf.Reads.synth(a.reads, 150, seed=20261003, bait_text=bait, mito_ppm=5000, sub_ppm=10000, n_read_ppm=10000, n_base_ppm=1000)
    g = bait_records(bait)[0]
    eight = ">mito\n%s\n" % g + "".join(">copy_%d\n%s\n" % (i, mutated(g, 0.02 * i, i)) for i in range(1, 8))
    L = mf.load()
    out = {}
    for name, text in (("headline", bait), ("eight", eight)):
        ks = mf.KmerSet.from_text(text, 31)
        R = len(ks.record_names)
        rc = np.zeros(R + 2, dtype=np.uint64)
        gc = np.zeros(R + 2, dtype=np.uint64)
        a_rec = lambda: mf._chk(L.mf_assign(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, rc.ctypes.data, None))
        a_grp = lambda: mf._chk(L.mf_assign_groups(ks._h, reads._h, 1, mf.MODE_SCREENED, None, None, gc.ctypes.data, None))
        ms_rec, ms_id = per_pass(a_rec, a.reps), per_pass(a_grp, a.reps)
        same = bool(np.array_equal(rc, gc))
        ks.group_records("_", 1)                     # "copy" / "mito": two groups on the eight-record bait
        G = len(ks.group_names)
        gc = np.zeros(G + 2, dtype=np.uint64)
        ms_field = per_pass(a_grp, a.reps)
        out[name] = {"records": R, "ms_assign": round(ms_rec, 4), "ms_assign_groups_identity": round(ms_id, 4),
                     "ratio_identity": round(ms_id / ms_rec, 3), "identity_counts_equal": same, "groups_by_field": G,
                     "ms_assign_groups_field": round(ms_field, 4), "ratio_field": round(ms_field / ms_rec, 3)}
        ks.close()
    reads.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=33_333_334)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["protein", "nucleotide"])
    a = ap.parse_args()
    from mitoflex_amd import mitofilter as mf
    out = {}
    if a.only != "nucleotide":
        out["protein"] = protein(mf, a)
    if a.only != "protein":
        out.update(nucleotide(mf, a))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
