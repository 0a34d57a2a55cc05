"""tests/pair_align_oracle.py held to hand-written cases on the 120-base record of tests/test_pair_oracle.py, k = 11, band 4: a rescued
mate with a 2-base deletion, with a 3-base insertion run and over each end of the record; a vote-placed mate with an indel that the
ungapped cut at 30 rejects and the aligned cut accepts, whose pair goes from single to proper; and band 0 against PairOracle.pairs field
by field.  No device."""
import numpy as np

from tests import pair_align_oracle as pao
from tests import pair_oracle as pa
from tests import place_oracle as po
from tests.test_pair_oracle import K, diverged, record
from tests.util_data import revcomp

W = 4


def run(rec, s1, s2, lo, hi, rescue=1, permille=600, max_permille=1000, band=W, E=8):
    o = po.PlaceOracle(">r\n%s\n" % rec, K)
    P = pao.PairAlignOracle(o)
    return P.pairs([s1], [s2], o.tally([s1]), o.tally([s2]), 1, max_permille, band, lo, hi, rescue, permille, 1, E)


def test_a_rescued_mate_with_a_two_base_deletion():
    rec = record()
    a = rec[10:50]
    t = diverged(rec[70:88] + rec[90:112])          # 40 bases that lack rec[88:90]; its longer side lies behind the deletion
    w = run(rec, a, revcomp(t), 95, 110)
    assert not w["passes2"][0]
    # the seed is the ungapped candidate with the fewest mismatches: the 22 bases behind the deletion on their diagonal, d = 112 - 10
    assert w["pairs"][0].tolist() == [pao.RESCUED_2, 102] and w["rows2"][0].tolist() == [0, 1, 72, 112, 0, 0]
    # the alignment around it opens the deletion: every base compared, the five substitutions left, the footprint from 70
    assert w["aligns2"][0].tolist() == [40, 5, 0, 2, 70, 112]
    assert w["depth"][70:112].tolist() == [1] * 42 and int(w["depth"].sum()) == 82          # the deleted positions count as covered
    assert int(w["indels"][:, 0].sum()) == 2 and set(np.nonzero(w["indels"][:, 0])[0]) <= set(range(86, 92)) and int(w["indels"][:, 1:].sum()) == 0
    assert w["place_rec"][0].tolist() == [1, 1, 0, 0, 82, 82] and w["footprints"].tolist() == [82]
    r = w["align_rec"][0]
    assert r[:7].tolist() == [2, 0, 80, 5, 0, 2, 1] and r[7 + 0] == 1 and r[7 + 7] == 1 and int(r[7:].sum()) == 2
    assert int(w["counts"].sum()) == 80 and w["unplaced"] == [0, 0] and w["pair_rec"][0].tolist() == [0, 0, 0, 1, 0, 102]
    assert w["gapped_records"][0] == [118, 2, 0, 0]          # (a depth of 1: the one read's deletion is a strict majority, 2 * 1 > 1)


def test_a_rescued_mate_with_a_three_base_insertion_run():
    rec = record()
    a = rec[10:50]
    extra = "TAT"          # (letters that cannot slide into the record's own on either side of the run)
    assert rec[89] not in extra and rec[90] not in extra
    t = diverged(rec[64:90]) + extra + diverged(rec[90:101])          # 26 bases, three more, 11 bases: the longer side lies before the run
    w = run(rec, a, revcomp(t), 90, 105)
    assert w["pairs"][0].tolist() == [pao.RESCUED_2, 94] and w["rows2"][0].tolist() == [0, 1, 64, 104, 0, 0]
    assert w["aligns2"][0].tolist() == [37, 4, 3, 0, 64, 101]
    assert w["indels"][89].tolist() == [0, 1, 3] and int(w["indels"].sum()) == 4          # one run of three behind position 89
    assert w["ins_pile"][89].sum(axis=1).tolist()[:4] == [1, 1, 1, 0]
    assert ["ACGT"[int(np.argmax(w["ins_pile"][89][q]))] for q in range(3)] == list(extra)
    assert w["depth"][64:101].tolist() == [1] * 37 and int(w["depth"][101:].sum()) == 0
    assert w["align_rec"][0][:7].tolist() == [2, 0, 77, 4, 3, 0, 1]
    g = w["gapped"].decode()
    assert w["gapped_records"][0] == [123, 0, 1, 3] and g[90:93] == extra and len(g) == 123


def test_a_rescued_mate_over_each_end_of_the_record():
    rec = record()
    # over the begin: a forward target behind a reverse mate
    t = diverged("GATTC" + rec[0:35])
    w = run(rec, revcomp(rec[60:100]), t, 100, 110, permille=200)
    assert w["pairs"][0].tolist() == [pao.RESCUED_2, 105] and w["rows2"][0].tolist() == [0, 0, -5, 35, 0, 0]
    assert w["aligns2"][0].tolist() == [35, 4, 0, 0, -5, 35] and w["place_rec"][0].tolist() == [1, 1, 1, 0, 75, 75]
    assert w["ext_pile"][0, 0].sum(axis=1).tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and int(w["ext_pile"][0, 1].sum()) == 0
    assert "".join("ACGT"[int(np.argmax(w["ext_pile"][0, 0, e]))] for e in range(5)) == t[:5][::-1]
    assert w["extended"].decode()[:5] == t[:5] and w["extend_records"][0][:3] == [125, 5, 0]
    # over the end: a reverse target behind a forward mate
    t = diverged(rec[85:120] + "GATTC")
    w = run(rec, rec[10:50], revcomp(t), 110, 120, permille=200)
    assert w["pairs"][0].tolist() == [pao.RESCUED_2, 115] and w["rows2"][0].tolist() == [0, 1, 85, 125, 0, 0]
    assert w["aligns2"][0].tolist() == [35, 4, 0, 0, 85, 125] and w["place_rec"][0].tolist() == [1, 1, 0, 1, 75, 75]
    assert w["ext_pile"][0, 1].sum(axis=1).tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and int(w["ext_pile"][0, 0].sum()) == 0
    assert w["extended"].decode()[-5:] == t[-5:] and w["extend_records"][0][:3] == [125, 0, 5]


def test_a_vote_placed_mate_with_an_indel_is_settled_by_the_aligned_cut_alone():
    rec = record()
    a = rec[5:45]
    t = rec[60:78] + rec[79:111]          # 50 bases that lack rec[78]; the vote goes by the 32 bases behind it
    for band, kind in ((0, [pao.SINGLE_1, -1]), (W, [pao.PROPER, 106])):
        w = run(rec, a, revcomp(t), 100, 110, max_permille=30, band=band)
        assert w["rows2"][0].tolist()[:4] == [0, 1, 61, 111] and w["rows2"][0][4] > 0          # placed by vote either way, on one diagonal
        assert w["pairs"][0].tolist() == kind, band
    w0, w4 = run(rec, a, revcomp(t), 100, 110, max_permille=30, band=0), run(rec, a, revcomp(t), 100, 110, max_permille=30, band=W)
    # ungapped the 18 bases before the deletion are a column off: rejected at 30, the pair is single and -- placed and rejected -- no target
    assert w0["aligns2"][0][1] >= 10 and w0["align_rec"][0][:2].tolist() == [1, 1] and w0["why"][0] is None and int(w0["depth"][50:].sum()) == 0
    # aligned: one edit in 51 columns
    assert w4["aligns2"][0].tolist() == [50, 0, 0, 1, 60, 111] and w4["align_rec"][0][:2].tolist() == [2, 0] and w4["pair_rec"][0].tolist() == [1, 0, 0, 0, 0, 106]
    assert w4["depth"][60:111].tolist() == [1] * 51


def test_band_0_is_the_pair_oracle_field_by_field():
    rec = record()
    s1 = [rec[10:50], rec[10:50], rec[5:45], rec[10:50], diverged(rec[10:50]), diverged(rec[10:50])]
    s2 = [revcomp(diverged(rec[70:110])), revcomp(rec[70:110]), revcomp(rec[60:78] + rec[79:111]), revcomp(diverged(rec[85:120] + "GATTC")), revcomp(rec[70:110]),
          revcomp(diverged(rec[70:110]))]
    o = po.PlaceOracle(">r\n%s\n" % rec, K)
    t1, t2 = o.tally(s1), o.tally(s2)
    for max_permille in (1000, 30):
        for rescue in (0, 1):
            a = pao.PairAlignOracle(o).pairs(s1, s2, t1, t2, 1, max_permille, 0, 95, 120, rescue, 200)
            v = pa.PairOracle(o).pairs(s1, s2, t1, t2, 1, max_permille, 95, 120, rescue, 200)
            for m in ("1", "2"):
                assert np.array_equal(a["rows" + m], v["rows" + m]) and np.array_equal(a["passes" + m], v["passes" + m])
                assert np.array_equal(a["aligns" + m][:, :2], v["scores" + m]) and not a["aligns" + m][:, 2:4].any()
                placed = a["rows" + m][:, 0] < po.AMBIGUOUS
                assert np.array_equal(a["aligns" + m][placed, 4:], a["rows" + m][placed, 2:4]) and not a["aligns" + m][~placed].any()
            assert np.array_equal(a["pairs"], v["pairs"]) and np.array_equal(a["pair_rec"], v["pair_rec"]) and a["none"] == v["none"] and a["why"] == v["why"]
            assert np.array_equal(a["depth"], v["depth"]) and np.array_equal(a["place_rec"], v["place_rec"]) and np.array_equal(a["counts"], v["counts"])
            assert a["unplaced"] == v["unplaced"]
            assert np.array_equal(a["align_rec"][:, :4], v["score_rec"][:, :4]) and np.array_equal(a["align_rec"][:, 7:], v["score_rec"][:, 4:])
            assert not a["align_rec"][:, 4:7].any() and not a["indels"].any() and a["gapped"] == bytes(pa.PairOracle(o).V.P.call(v["counts"], 1)[0])
    assert sorted(set(a["pairs"][:, 0].tolist())) == [pao.NONE, pao.PROPER, pao.RESCUED_1, pao.RESCUED_2, pao.SINGLE_1]
