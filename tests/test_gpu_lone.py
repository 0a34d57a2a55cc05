"""GPU parity on reads with ONE bait k-mer (tests/lone_data.py; the input's own conditions are held by tests/test_lone_data.py): a
69 Mbase stream of random reads, one read in five or so with a single bait window, at every alignment of the window against the 64-base
lane pieces, at both ends of a read, across every 16 KiB lane-piece border and every 32 KiB chunk border, with an invalid base beside or
inside it, one base off, or cut in two by a read border.  Nothing else in such a read is a positive, so every shortcut of the threshold-1
pass stands alone: phase 0's runs and the run start left to the lane on the left, phase 1's exact s-mer table and its sixteen owned
windows, the mark kernel's lone positive through stage 2 and stage 3, the exact kernel behind finish for k >= 48, the queue of lone
positives and the turn-by-turn front2 of the large-bait screens.  Every call is bit-exact against the C oracle.

PARITY UNPINNED BY THE REFERENCE (SURVEY.md 8a group B): the oracle is this repository's own.  Bar: bit-exact.
"""
import numpy as np
import pytest

from tests import lone_data as ld
from tests.test_gpu_fronts import FORMS
from tests.util_data import bits_to_bool

pytestmark = pytest.mark.gpu

# every case of screen_geom_for, the one-word / two-word key switch (32 | 33), the exact kernel behind finish (47 | 48)
KS = [19, 21, 22, 23, 25, 27, 28, 29, 30, 31, 32, 33, 41, 47, 48, 63]
DEFAULTS = (("pass", "default"), ("adapt", 1), ("finish_streams", 0), ("exact_co", 0), ("s8_finish", -1), ("front", -1), ("canon", -1),
            ("front2_log2b", 0), ("front3_log2b", -1))


@pytest.fixture(scope="module")
def mf(built_lib):
    from mitoflex_amd import mitofilter
    if mitofilter.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return mitofilter


@pytest.fixture(scope="module")
def ol():
    from oracle import oracle_lib
    oracle_lib.lib()
    return oracle_lib


@pytest.fixture()
def option(mf):
    """set options inside a test (a dict of what is set now goes into the messages); adapt is off -- the set is large enough for
    adapt_after_call to change the later calls otherwise -- and every option is back at its default afterwards"""
    now = {}

    def set_(name, value):
        mf.set_option(name, value)
        now[name] = value
    set_.now = now
    try:
        set_("adapt", 0)
        yield set_
    finally:
        for name, value in DEFAULTS:
            mf.set_option(name, value)


class Case:
    """one (set, k-mer set, resident reads) with the checks of the numbered calls"""

    def __init__(self, mf, s, ks, reads, option):
        self.mf, self.s, self.ks, self.reads, self.option = mf, s, ks, reads, option
        self.want = int(bits_to_bool(s.obits, s.n_reads).sum())
        self.want2 = int(bits_to_bool(s.obits2, s.n_reads).sum())

    def ctx(self, call):
        return dict(k=self.s.k, layout=self.s.layout, L=int(self.reads.info.uniform_len), call=call, options=dict(self.option.now))

    def diagnose(self, differ):
        """the first ten planted reads among the differing ones: kind, g0 mod 64, strand, in-read position, distance to the nearest
        65 536 border (0: the window holds one)"""
        s = self.s
        window_of = np.full(s.n_reads + 1, -1, dtype=np.int64)
        strad = s.kind == ld.STRADDLE
        window_of[s.read[strad] + 1] = np.nonzero(strad)[0]          # (the read a straddling window runs into)
        window_of[s.read] = np.arange(s.read.size)
        differ = np.nonzero(differ)[0]
        w = window_of[differ]
        planted = differ[w >= 0][:10]
        w = w[w >= 0][:10]
        dist = ld.border_distance(s.g0[w], s.k)
        rows = [dict(read=int(r), kind=ld.KINDS[s.kind[i]], g0_mod_64=int(s.g0[i] % 64), strand=int(s.strand[i]), pos=int(s.pos[i]),
                     read_len=int(s.read_len[i]), border_distance=int(d), chunk_border=bool(d == 0 and ((s.g0[i] + s.k - 1) // ld.BORDER) % 2 == 0))
                for r, i, d in zip(planted, w, dist)]
        return dict(differing_reads=int(differ.size), unplanted_among_them=int((window_of[differ] < 0).sum()), first_planted=rows)

    def bits_equal(self, bits, obits, call):
        if not np.array_equal(bits, obits):
            n = self.s.n_reads
            got, want = bits_to_bool(bits, n), bits_to_bool(obits, n)
            pytest.fail("pass bits differ from the oracle's: %s\nlost %d, spurious %d\n%s"
                        % (self.ctx(call), int((want & ~got).sum()), int((got & ~want).sum()), self.diagnose(got != want)))

    def hits_equal(self, hits, call):
        if not np.array_equal(hits, self.s.ohits):
            pytest.fail("hit counts differ from the oracle's: %s\n%s" % (self.ctx(call), self.diagnose(hits != self.s.ohits)))

    def call1(self):
        """the default pass"""
        bits, _, st = self.mf.filter_reads(self.ks, self.reads, 1, self.mf.MODE_SCREENED)
        self.bits_equal(bits, self.s.obits, 1)
        assert st.n_pass == self.want, self.ctx(1)

    def call2(self):
        """hit counts: mark (a lone positive goes through stage 2 and stage 3) and the exact kernel"""
        bits, hits, st = self.mf.filter_reads(self.ks, self.reads, 1, self.mf.MODE_SCREENED, want_hits=True)
        self.hits_equal(hits, 2)
        self.bits_equal(bits, self.s.obits, 2)
        assert st.n_pass == self.want, self.ctx(2)

    def call3(self):
        """threshold 2: nearly all clear"""
        bits, _, st = self.mf.filter_reads(self.ks, self.reads, 2, self.mf.MODE_SCREENED)
        self.bits_equal(bits, self.s.obits2, 3)
        assert st.n_pass == self.want2, self.ctx(3)

    def call4(self):
        bits, hits, st = self.mf.filter_reads(self.ks, self.reads, 1, self.mf.MODE_EXHAUSTIVE, want_hits=True)
        self.hits_equal(hits, 4)
        self.bits_equal(bits, self.s.obits, 4)
        assert st.n_pass == self.want, self.ctx(4)

    def call5(self):
        """four pipelined passes, the finish kernels on one stream and on two: every pass's count, then the bits of a following call
        (the co-resident exact kernel for k >= 48, the three buffer sets of the two-word keys)"""
        for streams in (1, 2):
            self.option("finish_streams", streams)
            per, _ = self.mf.filter_resident_passes(self.ks, self.reads, 1, self.mf.MODE_SCREENED, 4)
            assert [int(x) for x in per] == [self.want] * 4, self.ctx(5)
            bits, _, st = self.mf.filter_reads(self.ks, self.reads, 1, self.mf.MODE_SCREENED)
            self.bits_equal(bits, self.s.obits, 5)
            assert st.n_pass == self.want, self.ctx(5)
        self.option("finish_streams", 0)


@pytest.fixture()
def case(mf, ol, bait_text, option):
    """case(k, layout) -> a Case on a k-mer set built under the options set so far; everything is closed afterwards"""
    opened = []

    def open_(k, layout):
        s = ld.cached_set(k, layout, bait_text)
        ks = mf.KmerSet.from_text(bait_text, k)
        reads = mf.Reads.from_packed(s.words, s.offsets, s.npos)
        opened.extend((reads, ks))
        return Case(mf, s, ks, reads, option)
    yield open_
    for x in opened:
        x.close()


@pytest.mark.parametrize("layout", ld.LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_lone_kmer_reads_match_oracle(mf, case, option, k, layout):
    c = case(k, layout)
    c.call1()
    c.call2()
    c.call3()
    c.call4()
    c.call5()
    option("pass", "split")                      # the candidate-bitmap pass: screen, mark, exact
    c.call1()
    c.call5()
    option("exact_co", 1)                        # ... its exact kernel in the co-resident form behind every screen
    c.call1()
    c.call5()
    option("exact_co", 0)
    option("pass", "serial")                     # one stream; k < 28: the stride-8 geometries through the finish kernels
    c.call1()
    option("pass", "default")
    if k < 28:
        option("s8_finish", 1)                   # a set whose default pass is screen + finish at a sample every 8 bases
        c8 = case(k, layout)
        c8.call1()
        c8.call5()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [21, 31, 41])
def test_lone_kmer_reads_through_the_forced_screens(mf, case, option, k, form):
    """the large-bait screens forced onto the small bait: screen3_kernel's queue of lone positives and screen2_kernel's turn-by-turn
    front2 are the paths a read with one positive takes"""
    mode, f2, f3 = form[:3]
    option("front", mode)
    option("front2_log2b", f2)
    option("front3_log2b", f3)
    option("canon", form[3] if len(form) > 3 else -1)
    c = case(k, "uniform")
    assert c.ks.info.canonical_screen == (1 if len(form) > 3 and form[3] == 1 else 0)
    c.call1()
    c.call2()
    c.call5()
