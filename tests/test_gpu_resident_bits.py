"""Every pass of a PIPELINED resident call held to the oracle's bits.  filter_resident_bits (mf_filter_resident_bits, test support) returns
what each of a call's passes left in the result bitmap of its own buffer set: the bitmap is copied out behind the pass's last kernel, on
that kernel's stream, before the screen of a later pass clears it.  Every other check of a pipelined call reads counts, or the bits of one
more pass that recomputes them; a pass bit that lands on another read, in another buffer set or in a bitmap that was not cleared leaves the
counts right and shows only here.

The inputs are those of tests/test_gpu_lone.py (a read passes through ONE window: a dropped or misplaced bit has nowhere to hide; 526
chunks: a finish kernel has a following screen to run under) and of tests/sequence_data.py (the bait-rich set, the protein set), and three
tiny sets around one bitmap word.  Their conditions -- some reads pass and not all, some read r has bit r set and bit r ^ 1 clear -- are
held on the CPU by tests/test_lone_data.py and tests/test_sequence_data.py.  Every comparison is exact, for every pass.

PARITY UNPINNED BY THE REFERENCE (SURVEY.md 8a group B): the oracle is this repository's own.  Bar: bit-exact.
"""
import random

import numpy as np
import pytest

from mitoflex_amd.utility.synth_bait import bait_records
from tests import lone_data as ld
from tests import sequence_data as sd
from tests.test_gpu_fronts import FORMS
from tests.test_gpu_lone import DEFAULTS, Case, case, mf, ol  # noqa: F401  (case, mf, ol: fixtures)
from tests.util_data import bits_to_bool

pytestmark = pytest.mark.gpu

KS = [21, 31, 41, 48, 63]          # the stride-8 plan, the default plan, three buffer sets (two-word keys), the exact kernel behind finish and its co-resident form
STEPS = [2, 3, 4, 7]               # the smallest pipelined call, NSETS, three sets wrapped once, every set used twice at the least


@pytest.fixture()
def option(mf):
    """test_gpu_lone's fixture (adapt off, every option back at its default afterwards), and screen_streams beside them"""
    now = {}

    def set_(name, value):
        mf.set_option(name, value)
        now[name] = value
    set_.now = now
    try:
        set_("adapt", 0)
        yield set_
    finally:
        for name, value in DEFAULTS + (("screen_streams", 2),):
            mf.set_option(name, value)


def rows_equal(c, thr, mode, steps, obits, want, call):
    """one filter_resident_bits call on the case's handle: every pass's bits and count against the oracle's; a failure names the passes that
    differ and, through the case's diagnose, the kind and border of the planted windows of the first one"""
    bits, per, st = c.mf.filter_resident_bits(c.ks, c.reads, thr, mode, steps)
    assert bits.shape == (steps, (c.s.n_reads + 31) // 32) and per.shape == (steps,)
    wrong = [i for i in range(steps) if not np.array_equal(bits[i], obits)]
    if wrong:
        n = c.s.n_reads
        got, exp = bits_to_bool(bits[wrong[0]], n), bits_to_bool(obits, n)
        pytest.fail("the bits pass(es) %s of %d left in their buffer set differ from the oracle's: %s\npass %d: lost %d, spurious %d\n%s"
                    % (wrong, steps, c.ctx(call), wrong[0], int((exp & ~got).sum()), int((got & ~exp).sum()), c.diagnose(got != exp)))
    assert [int(x) for x in per] == [want] * steps and st.n_pass == want, (per.tolist(), want, c.ctx(call))


def every_step(c, call):
    for steps in STEPS:
        rows_equal(c, 1, c.mf.MODE_SCREENED, steps, c.s.obits, c.want, "%s, %d steps" % (call, steps))


# ------------------------------------------------------------------------------------------------------------- a. lone-k-mer streams
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
@pytest.mark.parametrize("k", KS)
def test_every_pass_of_a_pipelined_call_leaves_the_oracles_bits(mf, case, option, k, layout):
    c = case(k, layout)
    for streams in (1, 2):
        option("finish_streams", streams)
        every_step(c, "finish_streams")
    option("finish_streams", 0)
    rows_equal(c, 2, mf.MODE_SCREENED, 3, c.s.obits2, c.want2, "threshold 2")          # the candidate-bitmap pass, pipelined
    rows_equal(c, 1, mf.MODE_EXHAUSTIVE, 3, c.s.obits, c.want, "exhaustive")           # one stream, no rotation: the set stays
    every_step(c, "back at threshold 1")                                                # (over what the two left)
    option("pass", "split")
    every_step(c, "split")
    option("exact_co", 1)
    every_step(c, "split, exact_co")
    option("exact_co", 0)
    option("pass", "serial")
    every_step(c, "serial")
    option("pass", "default")
    option("screen_streams", 1)
    every_step(c, "screen_streams")
    option("screen_streams", 2)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_every_pass_of_a_stride8_set_through_the_finish_kernels(mf, case, option, layout):
    """k < 28: a set built under s8_finish = 1, whose default pass is screen + finish at a sample every 8 bases"""
    option("s8_finish", 1)
    c8 = case(21, layout)
    for streams in (1, 2):
        option("finish_streams", streams)
        every_step(c8, "s8_finish set, finish_streams")


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
@pytest.mark.parametrize("k", KS)
def test_every_pass_at_threshold_2_where_reads_pass_it(mf, case, option, bait_text, k, layout):
    """The same stream, two neighbouring reads taken as one: a read passes threshold 2 when both its halves hold a window.  (The set's own
    threshold-2 bitmap is empty for k >= 48, tests/test_lone_data.py.)  Threshold-1 passes first: the bitmaps then hold more bits than the
    passes under test may leave."""
    c = case(k, layout)
    p = ld.paired_set(k, layout, bait_text)
    reads = mf.Reads.from_packed(c.s.words, p.offsets, c.s.npos)
    try:
        mf.filter_resident(c.ks, reads, 1, mf.MODE_SCREENED, 3)
        want2 = int(bits_to_bool(p.obits2, p.n_reads).sum())
        for steps in (3, 4):
            bits, per, st = mf.filter_resident_bits(c.ks, reads, 2, mf.MODE_SCREENED, steps)
            wrong = [i for i in range(steps) if not np.array_equal(bits[i], p.obits2)]
            assert not wrong, ("threshold 2, reads paired: passes whose bits differ from the oracle's", wrong, k, layout, steps)
            assert per.tolist() == [want2] * steps and st.n_pass == want2, (k, layout, steps, per.tolist(), want2)
    finally:
        reads.close()


# ----------------------------------------------------------------------------------------------------- b. forced large-bait screens
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [21, 31, 41])
def test_every_pass_through_the_forced_screens(mf, case, option, k, form):
    mode, f2, f3 = form[:3]
    option("front", mode)
    option("front2_log2b", f2)
    option("front3_log2b", f3)
    option("canon", form[3] if len(form) > 3 else -1)
    c = case(k, "uniform")
    assert c.ks.info.canonical_screen == (1 if len(form) > 3 and form[3] == 1 else 0)
    rows_equal(c, 1, mf.MODE_SCREENED, 4, c.s.obits, c.want, "forced screen %s" % (form,))


# ------------------------------------------------------------------------------------------------------------------ c. bait-rich set
@pytest.fixture(scope="module")
def rich(mf, ol):
    reads = mf.Reads.synth(sd.RICH_N, sd.RICH_LEN, sd.RICH_SEED, bait_text=sd.baits()[0], mito_ppm=1_000_000, sub_ppm=30_000, keep_host=True)
    R = sd.rich_arrays(reads.host_words, reads.host_npos)
    yield (lambda: mf.Reads.from_packed(R.words, R.offsets, R.npos)), R          # (a fresh handle a case: the feedback starts from nothing)
    reads.close()


@pytest.mark.parametrize("k", [31, 63])
def test_every_pass_on_the_bait_rich_set_while_the_pass_kind_adapts(mf, rich, k):
    """adaptation on: the second call follows the feedback of the first (at k = 31 from screen + finish passes, which saw more work items
    than reads, to candidate-bitmap passes), and its first passes write over what the other kind of pass left in the buffer sets"""
    upload, R = rich
    want = sd.rich_expected(R, "k%d" % k)
    assert 0 < want.n_pass < sd.RICH_N and sd.moved_bit_shows(want.bits, sd.RICH_N), want.n_pass
    ks, reads = mf.KmerSet.from_text(sd.baits()[0], k), upload()
    try:
        candidates = []
        for call in (1, 2):
            bits, per, st = mf.filter_resident_bits(ks, reads, 1, mf.MODE_SCREENED, 3)
            candidates.append(int(st.n_candidates))
            wrong = [i for i in range(3) if not np.array_equal(bits[i], want.bits)]
            assert not wrong, (k, "call %d" % call, "passes that differ", wrong, candidates)
            assert per.tolist() == [want.n_pass] * 3 and st.n_pass == want.n_pass, (k, call, per.tolist(), want.n_pass)
        print("k", k, "n_candidates of the two calls", candidates)
        if k == 31:
            assert candidates[0] > sd.RICH_N >= candidates[1], candidates          # the pass kind did change between the calls
    finally:
        reads.close()
        ks.close()


# -------------------------------------------------------------------------------------------------------------------- d. protein set
@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_every_pass_of_the_protein_set(mf, ol, layout):
    want = sd.expected(layout, "prot", 1)
    R = sd.packed(layout)
    ks, reads = mf.KmerSet.protein_from_text(sd.baits()[1], sd.PROT_KP, sd.PROT_CODE), mf.Reads.from_packed(R.words, R.offsets, R.npos)
    try:
        bits, per, st = mf.filter_resident_bits(ks, reads, 1, mf.MODE_SCREENED, 3)
        assert [i for i in range(3) if not np.array_equal(bits[i], want.bits)] == []
        assert per.tolist() == [want.n_pass] * 3 and st.n_pass == want.n_pass
    finally:
        reads.close()
        ks.close()


# -------------------------------------------------------------------------------------------------------------------------- e. edges
def bait_cuts(bait_text, n, every_other_random):
    """n reads of 150 bases cut from the bait's first record (every second one random bases instead, when asked for)"""
    rec = bait_records(bait_text)[0].upper()
    rng = random.Random(1000 + n)
    seqs = []
    for i in range(n):
        at = rng.randrange(0, len(rec) - 150)
        seqs.append("".join(rng.choice("ACGT") for _ in range(150)) if every_other_random and i % 2 else rec[at:at + 150])
    return seqs


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n", [31, 32, 33])
def test_one_bitmap_word_and_its_borders(mf, ol, bait_text, n, mixed):
    """one bitmap word short of a bit, exactly full, and one bit into a second word: every row equals the oracle's, and the unused bits of the
    last word are zero in every row"""
    R = ol.OracleReads.from_seqs(bait_cuts(bait_text, n, mixed))
    obits, _ = ol.filter_reads(ol.OracleTable(bait_text, 31), R, 1)
    passing = bits_to_bool(obits, n)
    assert passing.tolist() == [not (mixed and i % 2) for i in range(n)]
    ks, reads = mf.KmerSet.from_text(bait_text, 31), mf.Reads.from_packed(R.words, R.offsets, R.npos)
    try:
        for steps in (3, 4):
            bits, per, st = mf.filter_resident_bits(ks, reads, 1, mf.MODE_SCREENED, steps)
            assert bits.shape == (steps, (n + 31) // 32)
            assert all(np.array_equal(row, obits) for row in bits), (n, steps, bits.tolist(), obits.tolist())
            if n % 32:
                assert not (bits[:, -1] >> np.uint32(n % 32)).any(), (n, steps, bits.tolist())
            assert per.tolist() == [int(passing.sum())] * steps
        for steps in (0, -1):
            with pytest.raises(mf.MitoFilterError, match="steps"):
                mf.filter_resident_bits(ks, reads, 1, mf.MODE_SCREENED, steps)
    finally:
        reads.close()
        ks.close()


@pytest.mark.parametrize("layout", sd.LAYOUTS)
def test_a_partial_last_word_stays_clean_in_every_row(mf, ol, layout):
    """6 000 reads: 187 words and 16 bits.  k = 63 rotates three buffer sets, k = 31 two; both on one handle, so that the second call's passes
    write into bitmaps that hold the first one's result"""
    assert sd.N_READS % 32 == 16
    R = sd.packed(layout)
    reads = mf.Reads.from_packed(R.words, R.offsets, R.npos)
    try:
        for k in (63, 31):
            want = sd.expected(layout, "k%d" % k, 1)
            ks = mf.KmerSet.from_text(sd.baits()[0], k)
            try:
                bits, per, _ = mf.filter_resident_bits(ks, reads, 1, mf.MODE_SCREENED, 3)
                assert not (bits[:, -1] >> np.uint32(16)).any(), (k, bits[:, -1].tolist())
                assert [i for i in range(3) if not np.array_equal(bits[i], want.bits)] == [] and per.tolist() == [want.n_pass] * 3, k
            finally:
                ks.close()
    finally:
        reads.close()
