"""GPU parity on reads with ONE bait k-mer at uniform read lengths other than 150 (tests/lone_data.py, the layout ("uniform", L); the
input's own conditions are held by tests/test_lone_data.py).  A set whose reads share one length takes code of its own in every filter
kernel: read_holding's division by multiplication (len_magic, and its L == 1 case), the 32-bit one of the mark and finish kernels for
2 <= L <= 4096 (the chunk base rq * L + rrem, the straddle test offr + span > L, phase 0 handing a run start to the lane on the left),
their ragged-style branch for L > 4096, and b0 = r * L in the exact kernel and the finish kernel's items.  At L = 150 a read never starts
on an odd base; here the lengths are k and k + 1 (a read holds one window, or two), lengths of every gcd with 16 and 64, PE100 / 125 /
151 / 250, both sides of the 4096 limit and, for k = 31 and 63, a read longer than a 65 536-base lane piece.  The calls are those of
tests/test_gpu_lone.py, every one bit-exact against the C oracle.

PARITY UNPINNED BY THE REFERENCE (SURVEY.md 8a group B): the oracle is this repository's own.  Bar: bit-exact.
"""
import pytest

from tests import lone_data as ld
from tests.test_gpu_fronts import FORMS
from tests.test_gpu_lone import case, mf, ol, option          # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KL = [(k, L) for k in ld.LENGTH_KS for L in ld.lengths_for(k)]


def open_uniform(case, k, L):
    c = case(k, ("uniform", L))
    assert c.reads.info.uniform_len == L and c.reads.info.n_reads == c.s.n_reads          # the path under test is the one that runs
    return c


@pytest.mark.parametrize("k,L", KL)
def test_lone_kmer_reads_at_uniform_lengths(mf, case, option, k, L):          # noqa: F811
    c = open_uniform(case, k, L)
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
        c8 = open_uniform(case, k, L)
        c8.call1()
        c8.call5()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,L", [(k, L) for k in (21, 31, 41) for L in (k, 101, 4097)])
def test_lone_kmer_reads_at_uniform_lengths_through_the_forced_screens(mf, case, option, k, L, form):          # noqa: F811
    """the large-bait screens forced onto the small bait, as in tests/test_gpu_lone.py: a read of k bases, PE101, and the ragged-style
    branch of the follow-up kernels (L > 4096)"""
    mode, f2, f3 = form[:3]
    option("front", mode)
    option("front2_log2b", f2)
    option("front3_log2b", f3)
    option("canon", form[3] if len(form) > 3 else -1)
    c = open_uniform(case, k, L)
    assert c.ks.info.canonical_screen == (1 if len(form) > 3 and form[3] == 1 else 0)
    c.call1()
    c.call2()
    c.call5()
