"""One read-set handle held to the oracles over SEQUENCES of calls.  A handle carries state from call to call -- three rotating buffer
sets (result bits, candidate bitmap, record lists), a pinned tally block of three regions a set, the parity of the pipelined passes, the
feedback that picks the next call's pass kind, the events between the streams, the hit counters, the report scratch that only grows --
and which of it a pass touches depends on the k-mer set, the threshold, the call and the options.  Every other GPU test uploads a fresh
handle for the one set it tests; here the read set stays and everything else changes under it (tests/sequence_data.py: the inputs, the
sequences and what each directed one is written for; tests/test_sequence_data.py: their conditions, without a device).

After EVERY op: bits equal the oracle's (a resident call that returns none is followed by a filter_reads of the same set and threshold,
an op like any other, which recomputes them; filter_resident_bits returns what every one of its passes left in its own buffer set, and
every row equals the oracle's), hit counts equal the oracle's when asked for, stats.n_pass is the oracle's count, every entry of
filter_resident_passes and of filter_resident_bits is, and stats.n_candidates is what the same op gives as the first call of a freshly uploaded handle (the 6 000-read sets: below 100 000
reads nothing adapts, so the pass kind is a function of the op).  test_fresh_handles_agree_on_every_op establishes first that two fresh
handles agree on that figure: they do for every op but those that run screen + finish passes (sequence_data.finish_pass says why),
which are compared on n_pass alone.  All comparisons are exact."""
import contextlib
import functools

import numpy as np
import pytest

from tests import extend_data as xd
from tests import pileup_oracle as pio
from tests import sequence_data as sd
from tests import verify_oracle as vo
from tests.report_data import mf, ol  # noqa: F401  (fixtures)
from tests.report_data import upload as report_upload
from tests.test_gpu_align import check_result as align_check_result
from tests.test_gpu_assign import oracle_assign, owners
from tests.test_gpu_depth import Oracle as DepthOracle
from tests.test_gpu_depth import check as depth_check
from tests.test_gpu_extend import check_extended, ends_want, placement
from tests.test_gpu_gapped import check_gapped
from tests.test_gpu_keep import check_keep_bits
from tests.test_gpu_pileup import check as pileup_check
from tests.test_gpu_place import check as place_check
from tests.test_gpu_verify import check_result as verify_check_result
from tests.util_data import bits_to_bool

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def forced(mf, options, defaults):
    """options in force inside the block only"""
    try:
        for name, value in options.items():
            mf.set_option(name, value)
        yield
    finally:
        for name in options:
            mf.set_option(name, defaults[name])


@functools.lru_cache(maxsize=None)
def depth_oracle(text, k):
    return DepthOracle(text, k)


def call_options(o):
    return dict(x.split("=") for x in o.opts)


@pytest.fixture(scope="module")
def sets(mf, ol):
    """every k-mer set of the sequences, built once; the forced options hold only while a set is built"""
    nuc, prot = sd.baits()
    out = {}
    for name, (k, build_options) in sd.SETS.items():
        with forced(mf, build_options, sd.BUILD_DEFAULTS):
            out[name] = mf.KmerSet.protein_from_text(prot, k, sd.PROT_CODE) if name == "prot" else mf.KmerSet.from_text(nuc, k)
    yield out
    for ks in out.values():
        ks.close()


def upload(mf, layout):
    R = sd.packed(layout)
    return mf.Reads.from_packed(R.words, R.offsets, R.npos)


@pytest.fixture(scope="module")
def handles(mf, ol):
    """the shared handles: one upload a layout for every random sequence of this module"""
    out = {layout: upload(mf, layout) for layout in sd.LAYOUTS}
    yield out
    for r in out.values():
        r.close()


def run_op(mf, sets, reads, o):
    """-> (bits or None, hits or None, stats, passing reads of every pass or None, bits of every pass or None)"""
    ks, mode = sets[o.set], mf.MODE_SCREENED if o.mode == "S" else mf.MODE_EXHAUSTIVE
    with forced(mf, call_options(o), sd.CALL_DEFAULTS):
        if o.call in ("bits", "hits"):
            bits, hits, st = mf.filter_reads(ks, reads, o.thr, mode, want_hits=o.call == "hits")
            return bits, hits, st, None, None
        if o.call == "passes4":
            per, st = mf.filter_resident_passes(ks, reads, o.thr, mode, sd.STEPS[o.call])
            return None, None, st, per, None
        if o.call == "rbits3":
            rows, per, st = mf.filter_resident_bits(ks, reads, o.thr, mode, sd.STEPS[o.call])
            assert rows.shape[0] == len(per) == sd.STEPS[o.call]
            return None, None, st, per, rows
        return None, None, mf.filter_resident(ks, reads, o.thr, mode, sd.STEPS[o.call]), None, None


def check_op(got, want, what):
    bits, hits, st, per, rows = got
    assert st.n_reads == want.hits.size, what
    if bits is not None:
        assert np.array_equal(bits, want.bits), what
    if hits is not None:
        assert np.array_equal(hits, want.hits), what
    assert st.n_pass == want.n_pass, (st.n_pass, want.n_pass, what)
    if per is not None:
        assert [int(x) for x in per] == [want.n_pass] * len(per), what
    if rows is not None:
        wrong = [i for i, row in enumerate(rows) if not np.array_equal(row, want.bits)]
        assert not wrong, ("passes whose own bits differ from the oracle's", wrong, what)


# what an op gives as the first call of a fresh handle: (n_pass, n_candidates), computed once an op and layout
_FRESH = {}


def fresh(mf, sets, layout, o):
    if (layout, o) not in _FRESH:
        reads = upload(mf, layout)
        try:
            got = run_op(mf, sets, reads, o)
            check_op(got, sd.expected(layout, sd.key_of(o.set), o.thr), ("first call of a fresh handle", layout, sd.show([o])))
            _FRESH[layout, o] = (int(got[2].n_pass), int(got[2].n_candidates))
        finally:
            reads.close()
    return _FRESH[layout, o]


def run_sequence(mf, sets, reads, layout, ops, label):
    """the ops and the recomputes behind the resident ones that return no bits, every one checked; the message of a failure names the ops up to it"""
    done = []
    for o in sd.with_recomputes(ops):
        done.append(o)
        what = "%s on the %s handle, failing at op %d of: %s" % (label, layout, len(done), sd.show(done))
        got = run_op(mf, sets, reads, o)
        check_op(got, sd.expected(layout, sd.key_of(o.set), o.thr), what)
        if not sd.finish_pass(o):
            assert int(got[2].n_candidates) == fresh(mf, sets, layout, o)[1], (int(got[2].n_candidates), fresh(mf, sets, layout, o), what)


# ---------------------------------------------------------------------------------------------------------------------- the sets
def test_sets_take_the_forms_they_are_named_for(sets):
    info = {name: ks.info for name, ks in sets.items()}
    assert [info[s].k for s in sd.SETS] == [k for k, _ in sd.SETS.values()]
    assert [info[s].front_mode for s in ("k31", "k21", "k31f2", "k31f3c", "k31f4", "k21f1")] == [0, 0, 2, 3, 4, 1]
    assert [info[s].canonical_screen for s in ("k31", "k31f2", "k31f3c", "k31f4")] == [0, 0, 1, 0]
    assert [info[s].key_words for s in ("k31", "k33", "k47", "k48", "k63")] == [1, 2, 2, 2, 2]
    assert [info[s].screen_stride for s in ("k21", "k29", "k31", "k63")] == [8, 16, 16, 16]
    assert info["prot"].kind != info["k31"].kind and info["prot"].genetic_code == sd.PROT_CODE


# ----------------------------------------------------------------------------------------- a fresh handle's first call, every op
@pytest.mark.parametrize("thr", sd.THRESHOLDS)
@pytest.mark.parametrize("set_name", list(sd.SETS))
@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_fresh_handles_agree_on_every_op(mf, sets, layout, set_name, thr):
    """every op of the grid as the first call of two freshly uploaded handles: both are right, and both give the same n_candidates --
    which is what lets a sequence compare that figure too.  The ops of screen + finish passes agree on n_pass alone."""
    differ = []
    for o in sd.grid(set_name, thr):
        first = fresh(mf, sets, layout, o)
        del _FRESH[layout, o]
        second = fresh(mf, sets, layout, o)
        if first[0] != second[0] or (first[1] != second[1] and not sd.finish_pass(o)):
            differ.append((sd.show([o]), first, second))
    assert not differ, (len(differ), differ[:5])


# --------------------------------------------------------------------------------------------------------------- directed sequences
@pytest.mark.parametrize("name", list(sd.directed()))
@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_directed_sequence(mf, sets, layout, name):
    """each directed sequence from a known state: a handle uploaded for it (sequence_data.directed says what each is written for)"""
    reads = upload(mf, layout)
    try:
        run_sequence(mf, sets, reads, layout, sd.directed()[name], "sequence %s" % name)
    finally:
        reads.close()


# ----------------------------------------------------------------------------------------------------------------- random sequences
@pytest.mark.parametrize("seed", range(sd.N_SEEDS))
@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_random_sequence(mf, sets, handles, layout, seed):
    """16 random ops on the layout's SHARED handle: whatever the sequences before left there is this one's starting state"""
    run_sequence(mf, sets, handles[layout], layout, sd.random_sequence(seed), "random sequence, seed %d" % seed)


# ----------------------------------------------------------------------------------------------------------- the bait-rich handle
def test_bait_rich_handle_adapts_while_the_set_changes(mf, ol, sets):
    """120 000 reads, all of them bait reads, adaptation left on: the feedback of one call picks the pass kind of the next (the
    candidate-bitmap pass after a screen + finish pass that saw more work items than reads, and back) while the set changes under it.
    Bits and n_pass after every call."""
    reads = mf.Reads.synth(sd.RICH_N, sd.RICH_LEN, sd.RICH_SEED, bait_text=sd.baits()[0], mito_ppm=1_000_000, sub_ppm=30_000, keep_host=True)
    try:
        R = sd.rich_arrays(reads.host_words, reads.host_npos)
        want = {key: sd.rich_expected(R, key) for key in dict.fromkeys(sd.key_of(o.set) for o in sd.RICH_SEQUENCE)}
        counts = {key: w.n_pass for key, w in want.items()}
        assert len(set(counts.values())) == len(counts) and all(0 < n < sd.RICH_N for n in counts.values()), counts
        assert all(sd.moved_bit_shows(w.bits, sd.RICH_N) for w in want.values()), counts          # (the set is made on the device: its conditions are held here)
        done, candidates = [], []
        for o in sd.with_recomputes(sd.RICH_SEQUENCE):
            done.append(o)
            got = run_op(mf, sets, reads, o)
            candidates.append(int(got[2].n_candidates))
            check_op(got, want[sd.key_of(o.set)], "bait-rich handle, failing at op %d of: %s (n_candidates so far %s)" % (len(done), sd.show(done), candidates))
        # the feedback did move: the first k = 31 call is a screen + finish pass (work items: several a bait read), the second a candidate-bitmap pass (candidate reads)
        assert candidates[0] > sd.RICH_N >= candidates[1], candidates
    finally:
        reads.close()


# ======================================================================================================= report calls on one handle
# The report family shares the handle's scratch, which only grows and is cleared piecewise by each call: the assignment lists, the totals,
# sums and per-position sections of depth and of the placement family, the per-read placements, scores, keep bits and alignments, the
# aligner's work memory.  Here one upload of the `ends` reads (tests/extend_data.py) takes every report call in several orders, the set
# changing between neighbours, and every output of every call is held to the plain-Python oracle the call's own test file uses.
REPORT_DEPTH, REPORT_KEEP = xd.MIN_DEPTH, 1          # (KEEP_ACCEPTED)
BANDS = sd.REPORT_BANDS


@functools.lru_cache(maxsize=None)
def report_want(name, k):
    """the oracle's values of one distinct op: computed once, shared, left unchanged"""
    text = xd.ends_bait()[0]
    seqs = xd.ends_reads()[0]
    o = placement(k)
    if name == "assign":
        return oracle_assign(seqs, k, owners(text, k), 1, len(o.recs))
    if name == "depth":
        d = depth_oracle(text, k)
        return d, d.keys(seqs)
    if name == "place":
        return (o.tally(seqs),)
    if name == "pileup":
        P = pio.PileupOracle(o)
        passes, rows, _, _, unplaced = o.place(o.tally(seqs), 1)
        return P, (passes, rows, unplaced, P.pile(seqs, rows))
    if name == "verify_keep":
        V = vo.VerifyOracle(o)
        return V, V.verify(seqs, o.tally(seqs), 1, xd.CUT)
    return ends_want(k, BANDS[name])


def run_report(mf, ks, reads, name, k):
    """one report call, every output it returns against the oracle"""
    seqs = xd.ends_reads()[0]
    n, o = len(seqs), placement(k)
    want = report_want(name, k)
    if name == "assign":
        passes, oassign, ocounts = want
        bits, assign, counts = mf.assign_reads(ks, reads, 1)
        assert np.array_equal(bits_to_bool(bits, n), passes) and np.array_equal(assign, oassign) and np.array_equal(counts, ocounts)
    elif name == "depth":
        depth_check(mf, ks, reads, want[0], want[1], 1)
    elif name == "place":
        place_check(mf, ks, reads, o, want[0], 1, mf.MODE_SCREENED)
    elif name == "pileup":
        pileup_check(mf, ks, reads, want[0], seqs, None, 1, mf.MODE_SCREENED, REPORT_DEPTH, want[1])
    elif name == "verify_keep":
        v = mf.verify_reads(ks, reads, 1, mf.MODE_SCREENED, REPORT_DEPTH, xd.CUT, keep=REPORT_KEEP)
        verify_check_result(v, want[0], seqs, want[1], REPORT_DEPTH)
        check_keep_bits(v, want[1], REPORT_KEEP, n)
    else:
        X, _, awant, ins, ext = want
        band = BANDS[name]
        E = {"extend4096": 4096, "extend16": 16, "extend64_nopile": 64}.get(name, 0)
        a = mf.align_reads(ks, reads, band, REPORT_DEPTH, xd.CUT, REPORT_KEEP, pileup=name != "extend64_nopile", extend=E,
                           gapped=name in ("gapped8", "extend4096", "extend16"))
        align_check_result(mf, a, o, seqs, awant, REPORT_KEEP, REPORT_DEPTH)
        assert (a.pileup is None) == (name == "extend64_nopile") and (a.gapped is None) == (name not in ("gapped8", "extend4096", "extend16")) and (a.extended is None) == (E == 0)
        if a.gapped is not None:
            check_gapped(a, X.G, awant, ins, REPORT_DEPTH, band)
        if E:
            check_extended(a, X, awant, ins, ext[:, :, :E], REPORT_DEPTH, E)


@pytest.fixture(scope="module")
def report_handle(mf, ol):
    """ONE upload of the `ends` reads for every report sequence of this module, and the three sets"""
    text = xd.ends_bait()[0]
    reads = report_upload(mf, ol, xd.ends_reads()[0])
    sets = {k: mf.KmerSet.from_text(text, k) for k in sd.REPORT_KS}
    yield reads, sets
    reads.close()
    for ks in sets.values():
        ks.close()


@pytest.mark.parametrize("order", list(sd.report_orders()))
def test_report_calls_on_one_handle(mf, report_handle, order):
    reads, sets = report_handle
    done = []
    for name, k in sd.report_sequence(sd.report_orders()[order]):
        done.append("%s k%d" % (name, k))
        try:
            run_report(mf, sets[k], reads, name, k)
        except AssertionError as e:
            raise AssertionError("order %s, failing at op %d of: %s" % (order, len(done), "; ".join(done))) from e
