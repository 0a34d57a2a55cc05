"""Randomised differential test of the report kernels (mf_assign, mf_assign_groups, mf_depth, mf_place, mf_pileup, mf_verify and the keep
rule, mf_align, mf_align_gapped, mf_align_extended, mf_place_pairs with rescue) against their plain-Python oracles, as
tests/test_gpu_fuzz.py is for the filter: every seed of tests/report_fuzz_data.py draws a k, a bait, two mate sets and one value of
every parameter; the set is built once, each read set is uploaded once, and every call runs on those handles and is compared exactly
through the comparison functions of the directed tests, so the fuzz asserts what they assert.  tests/test_report_fuzz_data.py holds the
generator to what it is meant to reach.  Seeds are fixed, so a failure reproduces; the assertion message carries the configuration."""
import contextlib

import numpy as np
import pytest

from tests import report_fuzz_data as fd
from tests import test_gpu_align as t_align
from tests import test_gpu_assign as t_assign
from tests import test_gpu_depth as t_depth
from tests import test_gpu_extend as t_extend
from tests import test_gpu_gapped as t_gapped
from tests import test_gpu_group_assign as t_group
from tests import test_gpu_keep as t_keep
from tests import test_gpu_pairs as t_pairs
from tests import test_gpu_pileup as t_pileup
from tests import test_gpu_place as t_place
from tests import test_gpu_verify as t_verify
from tests.report_data import mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.util_data import bits_to_bool

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def told(c, call):
    """an assertion that fails inside carries the call and the seed's configuration"""
    try:
        yield
    except AssertionError as err:
        raise AssertionError("%s: %s\n%s" % (call, c["told"], err)) from err


def same(a, b, fields):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f


@pytest.mark.parametrize("seed", range(fd.N_SEEDS))
def test_report_calls_match_their_oracles(mf, ol, seed):
    c = fd.config(seed)
    e = fd.expected(c)
    k, text, s1, s2, thr, mode = c["k"], c["text"], c["seqs1"], c["seqs2"], c["thr"], c["mode"]
    min_depth, cut, band, keep, E = c["min_depth"], c["max_permille"], c["band"], c["keep"], c["extend"]
    lo, hi, rescue_permille = c["min_insert"], c["max_insert"], c["rescue_permille"]
    o, n = e["o"], len(s1)
    modes = (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE)
    ks = mf.KmerSet.from_text(text, k)
    r1, r2 = upload(mf, ol, s1), upload(mf, ol, s2)
    filtered = {(r, m): mf.filter_reads(ks, rd, thr, m)[0] for r, rd in ((1, r1), (2, r2)) for m in modes}

    with told(c, "build"):
        assert np.array_equal(ks.record_starts, o.starts)
        assert bytes(ks.bait_letters).decode() == e["Pile"].bait
        assert np.array_equal(ks.export_table(), ol.OracleTable(text, k).keys)
        assert r1.info.uniform_len == r2.info.uniform_len == c["uniform"]

    with told(c, "assign_reads"):
        for m in modes:
            bits, _, _ = t_assign.check_assign(mf, ol, ks, text, s1, k, thr, m, reads=r1)
            assert np.array_equal(bits, filtered[1, m])
    with told(c, "assign_groups %r" % (c["group"],)):
        sep, field = c["group"]
        ks.group_records(sep, field)
        G = t_group.Oracle(text, k, None, sep, field)
        keys = G.keys(s1)
        t_group.check(mf, r1, ks, G, s1, thr, keys, mode)
        assert np.array_equal(mf.assign_groups(ks, r1, thr, mode)[0], filtered[1, mode])
        ks.group_records(None, 0)
    with told(c, "record_depth"):
        t_depth.check(mf, ks, r1, t_depth.Oracle(text, k), keys, thr, mode)

    with told(c, "place_reads"):
        for m in modes:
            t_place.check(mf, ks, r1, o, e["t1"], thr, m)
    with told(c, "pileup_reads"):
        passes, rows, _, _, unplaced = e["place"]
        t_pileup.check(mf, ks, r1, e["Pile"], s1, e["t1"], thr, mode, min_depth, (passes, rows, unplaced, e["pile"]))
        assert np.array_equal(mf.pileup_reads(ks, r1, thr, mode, min_depth)[0], filtered[1, mode])
    with told(c, "verify_reads"):
        for m in modes:
            v = t_verify.check(mf, ks, r1, e["V"], s1, e["verify"], thr, m, min_depth, cut)
            w = t_keep.verify_keep(mf, ks, r1, thr, m, min_depth, cut, keep)
            t_verify.check_result(w, e["V"], s1, e["verify"], min_depth)
            t_keep.same_but_keep_bits(w, v)
            t_keep.check_keep_bits(w, e["verify"], keep, n)
            assert np.array_equal(v.bits, filtered[1, m])

    with told(c, "align_reads"):
        a = t_align.check(mf, ks, r1, o, s1, e["align"], band, cut, keep, min_depth, threshold=thr, mode=mode)
        assert np.array_equal(a.bits, filtered[1, mode])
        assert np.array_equal(bits_to_bool(a.keep_bits, n), t_align.ao.keep_bits(e["align"], keep))
    with told(c, "align_reads, band 0 is verify_reads"):
        v = t_keep.verify_keep(mf, ks, r1, thr, mode, min_depth, cut, keep)
        z = a if band == 0 else mf.align_reads(ks, r1, 0, min_depth, cut, keep, threshold=thr, mode=mode)
        same(z, v, t_align.SHARED)
        assert np.array_equal(z.align["compared"], v.score["compared"]) and np.array_equal(z.align["mismatches"], v.score["mismatches"])
        for f in ("accepted", "rejected", "compared", "mismatches", "hist"):
            assert np.array_equal(z.align_records[f], v.score_records[f]), f
        assert not t_align.table(z.align_records, ("insertions", "deletions", "gapped")).any() and not t_align.table(z.indels, ("del", "ins", "ins_bases")).any()
    if band > 0:
        with told(c, "align_reads, gapped"):
            g = mf.align_reads(ks, r1, band, min_depth, cut, keep, threshold=thr, mode=mode, gapped=True)
            t_align.check_result(mf, g, o, s1, e["align"], keep, min_depth)
            t_gapped.check_gapped(g, e["G"], e["align"], e["ins"], min_depth, band)
            same(g, a, t_gapped.OLD)
    if E > 0:
        with told(c, "align_reads, extend"):
            x = mf.align_reads(ks, r1, band, min_depth, cut, keep, threshold=thr, mode=mode, extend=E, gapped=True)
            t_align.check_result(mf, x, o, s1, e["align"], keep, min_depth)
            t_gapped.check_gapped(x, e["G"], e["align"], e["ins"], min_depth, band)
            t_extend.check_extended(x, e["X"], e["align"], e["ins"], e["ext"], min_depth, E)
            same(x, a, t_gapped.OLD)

    with told(c, "place_pairs, rescue"):
        p = t_pairs.check(mf.place_pairs(ks, r1, r2, lo, hi, True, rescue_permille, min_depth, cut, threshold=thr, mode=mode), e["P"], e["pairs"], n, min_depth)
        assert np.array_equal(p.bits1, filtered[1, mode]) and np.array_equal(p.bits2, filtered[2, mode])
    with told(c, "place_pairs, no rescue"):
        q = t_pairs.check(mf.place_pairs(ks, r1, r2, lo, hi, False, rescue_permille, min_depth, cut, threshold=thr, mode=mode), e["P"], e["pairs_alone"], n,
                          min_depth)
        v1 = mf.verify_reads(ks, r1, thr, mode, min_depth, cut)
        v2 = mf.verify_reads(ks, r2, thr, mode, min_depth, cut)
        assert np.array_equal(q.bits1, v1.bits) and np.array_equal(q.bits2, v2.bits) and np.array_equal(v2.bits, filtered[2, mode])
        assert np.array_equal(q.place1, v1.place) and np.array_equal(q.place2, v2.place)
        assert np.array_equal(q.score1, v1.score) and np.array_equal(q.score2, v2.score)
        assert np.array_equal(q.base_depth, v1.base_depth + v2.base_depth)
        for f in ("forward", "reverse", "over_begin", "over_end", "base_sum"):
            assert np.array_equal(q.place_records[f], v1.place_records[f] + v2.place_records[f]), f
        for f in mf.SCORE_RECORD.names:
            assert np.array_equal(q.score_records[f], v1.score_records[f] + v2.score_records[f]), f
        for f in mf.PILEUP.names:
            assert np.array_equal(q.pileup[f], v1.pileup[f] + v2.pileup[f]), f
        for f in ("bases", "matches", "mismatches"):
            assert np.array_equal(q.pileup_records[f], v1.pileup_records[f] + v2.pileup_records[f]), f
        assert q.unplaced.tolist() == (v1.unplaced + v2.unplaced).tolist()
        assert not np.isin(q.pairs["kind"], (mf.PAIR_RESCUED_1, mf.PAIR_RESCUED_2)).any() and int(q.pair_records["rescued"].sum()) == 0
    r1.close(); r2.close(); ks.close()
