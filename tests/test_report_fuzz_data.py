"""tests/report_fuzz_data.py gives what tests/test_gpu_report_fuzz.py relies on, evaluated with the oracles alone (no device), so that no
seed of the GPU test passes on data that never reaches the code it is meant for: every default seed has reads that pass and reads that
are placed, and across the default seeds every case the report kernels treat apart -- overhangs on both sides, both strands, invalid
bases in placed reads, ties, passing reads without a vote, reads the cut rejects, gapped alignments both ways, extension piles, variant
calls, rescued and unrescued mates, more than 64 vote candidates, sets of one read length, the bait sizes around the placement tile --
occurs in at least three seeds, and the k at which the key layout changes occur with placed reads."""
import functools
import time

import numpy as np
import pytest

from tests import pair_oracle as pa
from tests import place_oracle as po
from tests import report_fuzz_data as fd

SEEDS = 24
EACH_IN = 3


@functools.lru_cache(maxsize=None)
def facts(seed):
    """what one seed reaches, from its oracle results (computed once)"""
    c = fd.config(seed)
    t0 = time.perf_counter()
    e = fd.expected(c)
    seconds = time.perf_counter() - t0
    o, s1 = e["o"], c["seqs1"]
    passes, rows = e["place"][0], e["place"][1]
    placed = rows[:, 0] < po.AMBIGUOUS
    lens = np.array([o.lens[int(j)] if ok else 0 for j, ok in zip(rows[:, 0], placed)])
    has_n = np.array(["N" in po.kb._norm(s) for s in s1])
    al = e["align"]
    gapped_ok = al["accepted"] & (c["band"] > 0)
    kinds = e["pairs"]["pairs"][:, 0]
    f = {
        "k": c["k"], "seconds": seconds, "passing": int(passes.sum()), "placed": int(placed.sum()),
        "start_below_0": int((placed & (rows[:, 2] < 0)).sum()),
        "end_beyond": int((placed & (rows[:, 3] > lens)).sum()),
        "strand_1": int((placed & (rows[:, 1] == 1)).sum()),
        "placed_with_n": int((placed & has_n).sum()),
        "ties": int(((rows[:, 0] == po.AMBIGUOUS) & (rows[:, 5] > 0)).sum()),
        "passing_no_window": int((passes & (rows[:, 0] == po.AMBIGUOUS) & (rows[:, 5] == 0)).sum()),
        "cut_rejects": int((placed & ~e["verify"]["accepted"]).sum()),
        "insertions": int((gapped_ok & (al["aligns"][:, 2] > 0)).sum()),
        "deletions": int((gapped_ok & (al["aligns"][:, 3] > 0)).sum()),
        "gapped": int((gapped_ok & (al["aligns"][:, 2:4].sum(axis=1) > 0)).sum()),
        "extension_pile": int(e["ext"].sum()) if e["ext"] is not None else 0,
        "variants": int(e["Pile"].call(e["pile"], c["min_depth"])[1][:, 5].sum()),
        "rescued": int(np.isin(kinds, (pa.RESCUED_1, pa.RESCUED_2)).sum()),
        "unrescued": sum(w is not None for w in e["pairs"]["why"]),
        "over_64_candidates": sum(len(v) > 64 for _, v, _ in e["t1"]),
        "uniform": int(c["uniform"] > 0 and {len(s) for s in s1} == {c["uniform"]} and {len(s) for s in c["seqs2"]} == {c["uniform"]}),
        "total_at_tile": int(int(o.starts[-1]) in (fd.PS_TILE, fd.PS_TILE + 1)),
        "total_over_8192": int(int(o.starts[-1]) > 8192),
    }
    assert int(o.starts[-1]) == c["what"]["total"] <= 12000 and 2 <= len(o.recs) <= 7
    assert sum(n >= 200 for n in o.lens) >= 2 and 200 <= len(s1) == len(c["seqs2"]) <= 600
    assert 1 <= c["min_insert"] <= c["max_insert"] and c["max_insert"] - c["min_insert"] + 1 <= fd.RESCUE_MAX
    print("seed %2d k %2d: %s" % (seed, c["k"], " ".join("%s=%s" % (n, round(v, 2) if n == "seconds" else v) for n, v in f.items() if n != "k")))
    return f


CASES = ("start_below_0", "end_beyond", "strand_1", "placed_with_n", "ties", "passing_no_window", "cut_rejects", "insertions", "deletions",
         "extension_pile", "variants", "rescued", "unrescued", "over_64_candidates", "uniform", "total_at_tile", "total_over_8192")


@pytest.mark.parametrize("seed", range(SEEDS))
def test_every_seed_has_reads_that_pass_and_reads_that_are_placed(seed):
    f = facts(seed)
    assert f["passing"] >= 40 and f["placed"] >= 20, f
    assert f["seconds"] < 5, f


@pytest.mark.parametrize("case", CASES)
def test_every_case_occurs_in_three_seeds(case):
    seeds = [s for s in range(SEEDS) if facts(s)[case] > 0]
    assert len(seeds) >= EACH_IN, (case, seeds)


def test_every_k_occurs_and_the_layout_changes_hold_placed_reads():
    assert {facts(s)["k"] for s in range(SEEDS)} == set(fd.K_LIST) and len(fd.K_LIST) == 20
    for k in (11, 33, 48, 49, 63):
        assert any(facts(s)["k"] == k and facts(s)["placed"] >= 20 for s in range(SEEDS)), k


def test_config_is_a_function_of_the_seed():
    a, b = fd.config(5), fd.config(5)
    assert a["text"] == b["text"] and a["seqs1"] == b["seqs1"] and a["seqs2"] == b["seqs2"] and a["told"] == b["told"]
    assert fd.config(6)["seqs1"] != a["seqs1"]
