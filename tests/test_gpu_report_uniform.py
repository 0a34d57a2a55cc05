"""The report calls behind a filter pass (mf_assign, mf_depth, mf_place, mf_pileup, mf_verify) on read sets that are uniform at a length
other than 150: the read start b0 = r * L of mf_assign.hip and mf_tally_dev.h and, before it, the filter pass's own uniform code.  The
sets of the modules these checks come from are ragged, or 150 bases long (tests/test_gpu_depth.py's "uniform" sets end in three reads
of other lengths).  75 and 101: a length that is 11 mod 16 and an odd one that is 5 mod 16, so reads start on every base of a stream word.
Same plain-Python oracles, compared exactly."""
import numpy as np
import pytest

from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests import verify_oracle as vo
from tests.report_data import eight_record_bait, mf, mutate, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.test_gpu_assign import check_assign
from tests.test_gpu_depth import Oracle as DepthOracle, check as check_depth, depth_bait
from tests.test_gpu_pileup import check as check_pileup, drawn
from tests.test_gpu_place import check as check_place, place_bait, place_reads
from tests.test_gpu_verify import check as check_verify
from tests.util_data import make_reads, revcomp

pytestmark = pytest.mark.gpu

K, N = 31, 1200


def uploaded(mf, ol, seqs, L):
    reads = upload(mf, ol, seqs)
    assert reads.info.uniform_len == L and reads.info.n_reads == len(seqs)          # the path under test is the one that runs
    return reads


@pytest.mark.parametrize("L", [75, 101])
def test_assign_and_depth_on_uniform_reads(mf, ol, L):
    bait8 = eight_record_bait()
    ks = mf.KmerSet.from_text(bait8, K)
    seqs = make_reads(bait8, N, seed=2100 + L, read_len=L, uniform=True, mito_frac=0.5)
    seqs = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(seqs)]
    uploaded(mf, ol, seqs, L).close()
    for thr in (1, 3):
        for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
            _, _, counts = check_assign(mf, ol, ks, bait8, seqs, K, thr, mode)
    assert int(counts[:8].sum()) > 200                                            # reads went to records
    ks.close()

    text, _ = depth_bait()
    o = DepthOracle(text, K)
    ks = mf.KmerSet.from_text(text, K)
    assert np.array_equal(ks.record_starts, o.starts)
    seqs = make_reads(text, N, seed=2200 + L, read_len=L, uniform=True, mito_frac=0.5)
    seqs = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(seqs)]
    keys = o.keys(seqs)
    reads = uploaded(mf, ol, seqs, L)
    for thr in (1, 2):
        results = [check_depth(mf, ks, reads, o, keys, thr, mode) for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE)]
        assert np.array_equal(results[0][0], results[1][0])
        assert int(results[0][1]["depth_max"].max()) > 0
    reads.close()
    ks.close()


@pytest.mark.parametrize("L", [75, 101])
def test_place_pileup_and_verify_on_uniform_reads(mf, ol, L):
    text, parts = place_bait()
    o = po.PlaceOracle(text, K)
    P = pio.PileupOracle(o)
    V = vo.VerifyOracle(o)
    ks = mf.KmerSet.from_text(text, K)
    assert np.array_equal(ks.record_starts, o.starts)
    # 1000 of the mixed bag and 200 of a sample that differs from the bait at 1 % of its positions (mismatches, variants, reads to cut)
    _, seqs = place_reads(text, parts, K, N - 200, seed=2300 + L, uniform=True, read_len=L)
    seqs = seqs + drawn(mutate(parts["g"], 0.01, 77), 200, seed=2400 + L, lo=L, hi=L)
    assert len(seqs) == N
    tallies = o.tally(seqs)
    reads = uploaded(mf, ol, seqs, L)
    cut = {}
    for thr in (1, 3):
        results = [check_place(mf, ks, reads, o, tallies, thr, mode) for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE)]
        assert np.array_equal(results[0], results[1])
        want = None
        for min_depth in (1, 3):
            for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                want = check_pileup(mf, ks, reads, P, seqs, tallies, thr, mode, min_depth, want)
        rec = P.call(want[3], 3)[1]
        assert int(rec[:, 5].sum()) > 0 and int(rec[:, 2].sum()) > 0              # variants, mismatches
        for max_permille in (1000, 20, 0):
            wantv = V.verify(seqs, tallies, thr, max_permille)
            for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                check_verify(mf, ks, reads, V, seqs, wantv, thr, mode, 2, max_permille)
            cut[(thr, max_permille)] = int(wantv["score_rec"][:, 1].sum())
    assert cut[(1, 1000)] == 0 and 0 < cut[(1, 20)] < cut[(1, 0)]                 # the cuts cut
    reads.close()
    ks.close()
