"""Conditions on the INPUTS of tests/test_gpu_handle_sequences.py (tests/sequence_data.py), held against the C oracle alone: no GPU.
A sequence of calls on one read-set handle shows a buffer left over from the call before only if that call's result differs from this
one's -- so every expected value passes some reads and not all, and any two different expected values differ; a pass bit that moved to the
neighbouring read shows only where one of the two is set -- so every expected bitmap has such a pair; and the random sequences change the set
often enough and reach every kind of op."""
import itertools

import numpy as np
import pytest

from tests import sequence_data as sd


@pytest.fixture(scope="module")
def ol():
    from oracle import oracle_lib
    oracle_lib.lib()
    return oracle_lib


@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_read_sets(ol, layout):
    seqs = sd.read_seqs(layout)
    lens = np.array([len(s) for s in seqs])
    assert len(seqs) == sd.N_READS == 6000
    if layout == "uniform":
        assert set(lens.tolist()) == {150}
    else:
        assert lens.min() == 0 and lens.max() > 300 and np.unique(lens).size > 100 and (lens == 150).sum() > 1000
    R = sd.packed(layout)
    assert R.n_reads == sd.N_READS and int(R.offsets[-1]) == int(lens.sum()) and R.npos.size > 0
    assert sd.read_seqs(layout) is seqs and sd.packed(layout) is R          # (computed once)


@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_every_expected_value_passes_some_reads_and_not_all(ol, layout):
    counts = {(key, thr): sd.expected(layout, key, thr).n_pass for key in sd.KEYS for thr in sd.THRESHOLDS}
    print(layout, counts)
    assert all(0 < n < sd.N_READS for n in counts.values()), counts
    e = sd.expected(layout, "k31", 1)
    assert sd.expected(layout, "k31", 1) is e and not e.bits.flags.writeable and not e.hits.flags.writeable
    assert e.hits.size == sd.N_READS and e.bits.size == (sd.N_READS + 31) // 32


@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_a_moved_pass_bit_shows_in_every_expected_value(ol, layout):
    """every expected bitmap -- each is compared with the rows of an rbits3 op somewhere -- has a read r with bit r set and bit r ^ 1 clear:
    a pass bit written to the neighbouring read leaves every count right and changes the bitmap only there"""
    lacking = [(key, thr) for key in sd.KEYS for thr in sd.THRESHOLDS if not sd.moved_bit_shows(sd.expected(layout, key, thr).bits, sd.N_READS)]
    assert not lacking, lacking


def test_moved_bit_shows():
    bits = lambda *reads: np.array([sum(1 << r for r in reads)], dtype=np.uint32)
    assert not sd.moved_bit_shows(bits(), 6) and not sd.moved_bit_shows(bits(0, 1, 4, 5), 6) and not sd.moved_bit_shows(bits(0, 1, 2, 3, 4, 5), 6)
    assert sd.moved_bit_shows(bits(3), 6) and sd.moved_bit_shows(bits(0, 1, 2), 6) and sd.moved_bit_shows(bits(4), 5) and not sd.moved_bit_shows(bits(2, 3), 5)


@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_any_two_expected_values_differ(ol, layout):
    """Any op may follow any other in a random sequence.  Two entries of different keys differ in their bits AND in their hit counts; two
    thresholds of one key differ in their bits (a read's hit count is what it is at every threshold: asserted, too) and in how many pass."""
    entries = [(key, thr) for key in sd.KEYS for thr in sd.THRESHOLDS]
    for a, b in itertools.combinations(entries, 2):
        ea, eb = sd.expected(layout, *a), sd.expected(layout, *b)
        assert not np.array_equal(ea.bits, eb.bits), (a, b)
        if a[0] != b[0]:
            assert not np.array_equal(ea.hits, eb.hits), (a, b)
        else:
            assert np.array_equal(ea.hits, eb.hits) and ea.n_pass != eb.n_pass, (a, b)
    # the counts themselves are all distinct at threshold 1: a stale tally of another set is a wrong n_pass, whichever set left it
    ones = [sd.expected(layout, key, 1).n_pass for key in sd.KEYS]
    assert len(set(ones)) == len(ones), dict(zip(sd.KEYS, ones))


def test_sets_and_keys():
    assert [k for k, _ in (sd.SETS[s] for s in ("k21", "k29", "k31", "k33", "k41", "k47", "k48", "k63"))] == [21, 29, 31, 33, 41, 47, 48, 63]
    assert sd.SETS["k31f2"] == (31, {"front": 2}) and sd.SETS["k31f3c"] == (31, {"front": 3, "canon": 1}) and sd.SETS["k31f4"] == (31, {"front": 4})
    assert sd.SETS["k21f1"] == (21, {"front": 1}) and sd.SETS["prot"][0] == 7 and sd.PROT_CODE == 5
    assert all(set(forced) <= set(sd.BUILD_DEFAULTS) for _, forced in sd.SETS.values())
    assert sd.KEYS == ("k21", "k29", "k31", "k33", "k41", "k47", "k48", "k63", "prot")
    assert [sd.key_of(s) for s in ("k31f2", "k31f3c", "k31f4", "k21f1", "prot")] == ["k31", "k31", "k31", "k21", "prot"]
    assert sum(len(set(sd.grid("k31", thr))) for thr in sd.THRESHOLDS) == 3 * 7 * 2 * 6 and sd.STEPS["rbits3"] == 3 and set(sd.STEPS) == set(sd.CALLS)
    for opts in sd.OPTIONS:
        assert all(o.split("=")[0] in sd.CALL_DEFAULTS for o in opts)


def test_which_ops_run_screen_and_finish_passes():
    """the ops that are compared on n_pass alone: the rule, case by case"""
    f = sd.finish_pass
    assert f(sd.op("k31")) and f(sd.op("k63", 1, "res3")) and f(sd.op("k41", 1, "rbits3")) and not f(sd.op("k41", 2, "rbits3")) and f(sd.op("k29", 1, "passes4", "S", "exact_co=1")) and f(sd.op("k31f2", 1, "res5", "S", "finish_streams=2"))
    assert not f(sd.op("k31", 2)) and not f(sd.op("k31", 1, "hits")) and not f(sd.op("k31", 1, "bits", "E")) and not f(sd.op("k31", 1, "res3", "S", "pass=split"))
    assert not f(sd.op("prot")) and not f(sd.op("k21")) and not f(sd.op("k21f1", 1, "res5", "S", "exact_co=1"))
    assert f(sd.op("k21", 1, "bits", "S", "s8_finish=1")) and f(sd.op("k21", 1, "res3", "S", "pass=serial")) and not f(sd.op("k21", 1, "res3", "S", "s8_finish=1", "pass=split"))
    share = [f(o) for s in sd.SETS for thr in sd.THRESHOLDS for o in sd.grid(s, thr)]
    assert 0.08 < sum(share) / len(share) < 0.12          # a tenth of the grid's 3276 ops: the rest is compared on n_candidates too


def test_directed_sequences():
    seq = sd.directed()
    assert set(seq) == {"a", "b", "c", "d", "e", "f", "g31", "g21"}
    for ops in list(seq.values()) + [sd.RICH_SEQUENCE]:
        assert all(o.set in sd.SETS and o.thr in sd.THRESHOLDS and o.call in sd.CALLS and o.mode in sd.MODES for o in ops)
        assert all(o.split("=")[0] in sd.CALL_DEFAULTS for x in ops for o in x.opts)
        run = sd.with_recomputes(ops)
        assert len(run) == len(ops) + sum(o.call not in ("bits", "hits", "rbits3") for o in ops)
        for x, y in zip(run, run[1:]):          # a resident call that returns no bits is followed by the recompute of them
            if x.call not in ("bits", "hits", "rbits3"):
                assert y == sd.Op(x.set, x.thr, "bits", x.mode, ())
    assert [(o.set, o.call) for o in seq["a"]] == [("k63", "res3"), ("k31", "bits"), ("k31", "bits"), ("k31", "bits"), ("k63", "rbits3"), ("k21", "bits")]
    assert [o.set for o in seq["b"]] == ["k63", "k31", "k31"] and {o.call for o in seq["b"]} == {"bits"}
    assert [(o.set, o.call) for o in seq["c"]][:4] == [("k48", "res5"), ("k47", "res5"), ("k41", "passes4"), ("k33", "bits")]
    assert [(o.set, o.call) for o in seq["c"]][4:] == [("k48", "rbits3"), ("k31", "bits"), ("k41", "rbits3"), ("k63", "bits")]
    assert [(o.set, o.thr) for o in seq["f"]][:4] == [("k31f2", 1), ("k31f2", 2), ("k21", 1), ("k21", 2)] and seq["f"][-1].set == "k31f2"
    assert [o.opts for o in seq["g21"]][2:6] == [("s8_finish=1", "pass=split")] * 2 + [("s8_finish=1", "pass=serial")] * 2
    assert [o.set for o in sd.RICH_SEQUENCE] == ["k31", "k31", "k63", "k63", "k31", "k21", "k31", "k41", "k31", "k63", "k41", "k31", "k21"]
    assert len(seq["g31"]) == len(seq["g21"]) == 8 + 9 and [o.call for o in seq["g31"]][:8] == ["bits", "res3"] * 4
    assert [o.opts for o in seq["g21"] if o.call == "rbits3"] == [("s8_finish=1",), ("s8_finish=1", "pass=split"), ("s8_finish=1", "pass=serial")]
    # an rbits3 op of a directed sequence follows a call of another set -- its passes write into bitmaps that hold that set's result, which differs
    # (test_any_two_expected_values_differ) -- and a single pass of a third set follows it
    for name, ops in list(seq.items()) + [("rich", sd.RICH_SEQUENCE)]:
        run = sd.with_recomputes(ops)
        at = [i for i, o in enumerate(run) if o.call == "rbits3"]
        assert bool(at) == (name in ("a", "c", "g31", "g21", "rich")), name
        for i in at:
            keys = [sd.key_of(run[j].set) for j in (i - 1, i, i + 1)]
            assert len(set(keys)) == 3 and run[i + 1].call == "bits" and run[i].thr == run[i + 1].thr == 1, (name, i, keys)
    # in every directed sequence, neighbours that differ in (key, threshold) exist: it changes what a call expects
    for name, ops in seq.items():
        assert len({(sd.key_of(o.set), o.thr, o.call == "hits", o.mode) for o in ops}) > 1 or name.startswith("g"), name


def test_random_sequences_change_the_set_and_reach_every_op():
    assert sd.N_SEEDS >= 1
    all_ops = []
    for seed in range(24):          # (the conditions are stated for the 24 seeds of a default run)
        ops = sd.random_sequence(seed)
        assert ops == sd.random_sequence(seed) and len(ops) == sd.SEQ_LEN == 16
        assert sum(a.set != b.set for a, b in zip(ops, ops[1:])) >= 8, (seed, sd.show(ops))
        all_ops += ops
    assert {o.set for o in all_ops} == set(sd.SETS)
    assert {(o.call, o.mode) for o in all_ops} == set(itertools.product(sd.CALLS, sd.MODES))
    assert {o.opts for o in all_ops} == set(sd.OPTIONS)
    assert {(o.call, o.opts) for o in all_ops} == set(itertools.product(sd.CALLS, sd.OPTIONS))
    assert {o.thr for o in all_ops} == set(sd.THRESHOLDS)


def test_report_sequences_are_what_they_are_meant_to_be():
    """every order holds every distinct op once, neighbours differ in k, the
    shrinking pairs stay pairs, and the seven orders differ"""
    orders = sd.report_orders()
    assert len(orders) == 7 and len(set(orders.values())) == 7
    names = sorted(name for u in sd.REPORT_UNITS for name in u)
    for order in orders.values():
        seq = sd.report_sequence(order)
        assert sorted(name for name, _ in seq) == names and len(names) == 12
        assert all(a[1] != b[1] for a, b in zip(seq, seq[1:])) and all(k > sd.REPORT_BANDS.get(name, 0) for name, k in seq)
        at = {name: i for i, (name, _) in enumerate(seq)}
        assert at["align4"] == at["align30"] + 1 and at["extend16"] == at["extend4096"] + 1
    assert {k for order in orders.values() for _, k in sd.report_sequence(order)} == set(sd.REPORT_KS)
