"""tests/pair_oracle.py held to hand-written cases on a 120-base record, k = 11: a diverged mate rescued at a stated start on either
strand, a window that reaches the mate only at d = min_insert and only at d = max_insert, a candidate with compared = k - 1 refused, a
tie inside a tandem copy, and rescue = 0.  No device."""
import random

import numpy as np

from tests import pair_oracle as pa
from tests import place_oracle as po
from tests.util_data import revcomp

K = 11


def record(seed=4):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(120))


def diverged(s, every=8, first=3):
    """s with another letter every `every` bases: no K-mer of it is left"""
    t = list(s)
    for i in range(first, len(t), every):
        t[i] = "CGTA"["ACGT".index(t[i])]
    return "".join(t)


def run(rec, s1, s2, lo, hi, rescue=1, permille=200, max_permille=1000):
    o = po.PlaceOracle(">r\n%s\n" % rec, K)
    P = pa.PairOracle(o)
    return P.pairs([s1], [s2], o.tally([s1]), o.tally([s2]), 1, max_permille, lo, hi, rescue, permille)


def test_a_diverged_mate_is_rescued_behind_a_forward_mate():
    rec = record()
    a, b = rec[10:50], revcomp(diverged(rec[70:110]))
    w = run(rec, a, b, 90, 110)
    assert w["rows1"][0].tolist()[:4] == [0, 0, 10, 50] and w["rows1"][0][4] > 0
    assert not w["passes2"][0]                                     # it shares no 11-mer with the record
    assert w["rows2"][0].tolist() == [0, 1, 70, 110, 0, 0]         # votes 0 marks the rescue
    assert w["scores2"][0].tolist() == [40, 5]
    assert w["pairs"][0].tolist() == [pa.RESCUED_2, 100]
    assert w["pair_rec"][0].tolist() == [0, 0, 0, 1, 0, 100] and w["none"] == 0
    # it counts as an accepted placed read everywhere, and has left the reads that do not pass
    assert w["unplaced"] == [0, 0]
    assert w["place_rec"][0].tolist() == [1, 1, 0, 0, 80, 80]
    assert w["depth"][10:50].tolist() == [1] * 40 and w["depth"][70:110].tolist() == [1] * 40 and int(w["depth"].sum()) == 80
    s = w["score_rec"][0]
    assert s[:4].tolist() == [2, 0, 80, 5] and s[4 + 0] == 1 and s[4 + 5] == 1 and int(s[4:].sum()) == 2
    # the piled bases are the mate's own: along its footprint five positions hold another letter than the record
    letters = np.argmax(w["counts"][70:110], axis=1)
    assert sum("ACGT"[x] != c for x, c in zip(letters, rec[70:110])) == 5 and int(w["counts"].sum()) == 80


def test_a_diverged_mate_is_rescued_behind_a_reverse_mate():
    rec = record()
    a, b = diverged(rec[10:50]), revcomp(rec[70:110])
    w = run(rec, a, b, 90, 110)
    assert w["rows2"][0].tolist()[:4] == [0, 1, 70, 110]
    assert w["rows1"][0].tolist() == [0, 0, 10, 50, 0, 0] and w["scores1"][0].tolist() == [40, 5]
    assert w["pairs"][0].tolist() == [pa.RESCUED_1, 100]
    assert w["unplaced"] == [0, 0] and w["place_rec"][0].tolist()[:2] == [1, 1]


def test_the_window_reaches_the_mate_at_its_first_and_at_its_last_insert_only():
    rec = record()
    a, b = rec[10:50], revcomp(diverged(rec[70:110]))
    for lo, hi, rescued in ((100, 110, True), (90, 100, True), (100, 100, True), (101, 110, False), (90, 99, False)):
        w = run(rec, a, b, lo, hi)
        assert (w["pairs"][0].tolist() == [pa.RESCUED_2, 100]) == rescued, (lo, hi)
        if not rescued:
            assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] == "cut" and w["rows2"][0][0] == po.NONE
            assert w["unplaced"] == [0, 1] and w["pair_rec"][0].tolist() == [0, 0, 0, 0, 1, 0]


def test_the_cut_is_rescue_permille():
    rec = record()
    a, b = rec[10:50], revcomp(diverged(rec[70:110]))
    assert run(rec, a, b, 90, 110, permille=125)["pairs"][0].tolist() == [pa.RESCUED_2, 100]          # 5 * 1000 <= 125 * 40
    w = run(rec, a, b, 90, 110, permille=124)
    assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] == "cut"
    # max_permille is the vote-placed reads' cut, not the rescued mate's
    assert run(rec, a, b, 90, 110, permille=125, max_permille=0)["pairs"][0].tolist() == [pa.RESCUED_2, 100]


def test_a_candidate_that_compares_k_minus_1_bases_is_refused():
    rec = record()
    rng = random.Random(9)
    tail = "".join(rng.choice("ACGT") for _ in range(30))
    a = rec[60:100]
    # K - 1 bases of the mate lie inside the record: the candidate matches them all and is refused
    w = run(rec, a, revcomp(rec[110:120] + tail), 90, 90)
    assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] == "short"
    # K + 3 bases, one of them substituted so that the vote still finds no 11-mer: rescued, clipped at the record's end
    inside = rec[106:113] + "CGTA"["ACGT".index(rec[113])] + rec[114:120]
    w = run(rec, a, revcomp(inside + tail[:26]), 86, 86)
    assert not w["passes2"][0]
    assert w["pairs"][0].tolist() == [pa.RESCUED_2, 86]
    assert w["rows2"][0].tolist() == [0, 1, 106, 146, 0, 0] and w["scores2"][0].tolist() == [K + 3, 1]
    assert w["place_rec"][0].tolist() == [1, 1, 0, 1, 54, 54]
    # the rule itself at the boundary (such a mate would be placed by its one window: the rule is asked directly): K compared bases do
    P = pa.PairOracle(po.PlaceOracle(">r\n%s\n" % rec, K))
    row = (0, 0, 60, 100, 1, 1)
    assert P.rescue(revcomp(rec[109:120] + tail[:29]), row, 89, 89, 0) == ((109, 89, K, 0), None)
    assert P.rescue(revcomp(rec[110:120] + tail), row, 90, 90, 1000) == (None, "short")


def test_a_tie_inside_a_tandem_copy_leaves_the_mate_as_it_was():
    rng = random.Random(12)
    u, v, t = ("".join(rng.choice("ACGT") for _ in range(n)) for n in (30, 20, 50))
    rec = u + v + v + t
    a, b = rec[0:28], revcomp(v)
    w = run(rec, a, b, 50, 70)                                     # candidates at 30 .. 50: both copies
    assert w["passes2"][0] and w["single"][1]["rows"][0][0] == po.AMBIGUOUS          # it passes and has no anchor window
    assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] == "tie"
    assert w["rows2"][0][0] == po.AMBIGUOUS and w["unplaced"] == [1, 0]
    w = run(rec, a, b, 50, 69)                                     # the first copy alone
    assert w["pairs"][0].tolist() == [pa.RESCUED_2, 50] and w["rows2"][0].tolist()[:5] == [0, 1, 30, 50, 0]
    assert w["unplaced"] == [0, 0]                                 # it has left the passing reads that are not placed
    # one substitution in the first copy's first base: the mate goes to the second.  (Its own first window would now be an anchor there
    # and place it by vote; a substitution of its own in its second base keeps it without one.)
    rec2 = u + diverged(v, every=100, first=0) + v + t
    w = run(rec2, a, revcomp(diverged(v, every=100, first=1)), 50, 70)
    assert w["single"][1]["rows"][0][0] == po.AMBIGUOUS
    assert w["pairs"][0].tolist() == [pa.RESCUED_2, 70] and w["rows2"][0].tolist()[:4] == [0, 1, 50, 70] and w["scores2"][0].tolist() == [20, 1]


def test_without_rescue_the_reports_are_the_two_single_calls_added_up():
    rec = record()
    a, b = rec[10:50], revcomp(diverged(rec[70:110]))
    w = run(rec, a, b, 90, 110, rescue=0)
    assert w["pairs"][0].tolist() == [pa.SINGLE_1, -1] and w["why"][0] is None
    v1, v2 = w["single"]
    assert np.array_equal(w["rows1"], v1["rows"]) and np.array_equal(w["rows2"], v2["rows"])
    assert np.array_equal(w["depth"], v1["depth"] + v2["depth"]) and np.array_equal(w["counts"], v1["counts"] + v2["counts"])
    assert np.array_equal(w["score_rec"], v1["score_rec"] + v2["score_rec"])
    assert np.array_equal(w["place_rec"][:, :4], v1["place_rec"][:, :4] + v2["place_rec"][:, :4])
    assert w["unplaced"] == [v1["unplaced"][0] + v2["unplaced"][0], v1["unplaced"][1] + v2["unplaced"][1]]


def test_two_settled_mates_proper_discordant_and_their_insert():
    rec = record()
    a, b = rec[10:50], revcomp(rec[70:110])
    assert run(rec, a, b, 90, 110)["pairs"][0].tolist() == [pa.PROPER, 100]
    assert run(rec, a, b, 101, 110)["pairs"][0].tolist() == [pa.DISCORDANT, 100]
    assert run(rec, a, revcomp(a), 1, 4096)["pairs"][0].tolist() == [pa.PROPER, 40]
    assert run(rec, a, rec[70:110], 1, 4096)["pairs"][0].tolist() == [pa.DISCORDANT, -1]          # one strand
    w = run(rec, diverged(a), diverged(b), 1, 4096)
    assert w["pairs"][0].tolist() == [pa.NONE, -1] and w["none"] == 1 and w["unplaced"] == [0, 2] and int(w["pair_rec"].sum()) == 0
    # the reverse mate ends before the forward mate starts: no insert
    assert run(rec, rec[70:110], revcomp(rec[10:50]), 1, 4096)["pairs"][0].tolist() == [pa.DISCORDANT, -1]
