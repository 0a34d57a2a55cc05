"""tests/pair_align_data.py holds what it claims, by the oracle alone (no device): at RESCUE_PERMILLE and WINDOW at least 20 rescued mates
whose alignment has an insertion run of at least 2, a deletion, ref_begin < 0 or ref_end > len with at least 3 extension columns, or
that hold an N -- each on both strands and from both sets --, at least 20 pairs of every refusal and of every kind, and at least 20 pairs
whose kind differs between band 0 and band 8 at max_permille = 30."""
import functools

import numpy as np

from tests import align_oracle as ao
from tests import pair_align_data as pd
from tests import pair_align_oracle as pao
from tests import place_oracle as po

K = 21
LO, HI = pd.WINDOW


@functools.lru_cache(maxsize=None)
def oracle():
    text, recs, sample = pd.bait()
    o = po.PlaceOracle(text, K)
    return o, pao.PairAlignOracle(o)


@functools.lru_cache(maxsize=None)
def wanted(mixed, band, max_permille):
    o, P = oracle()
    s1, s2, what = pd.pair_set(mixed=mixed)
    return s1, s2, what, P.pairs(s1, s2, o.tally(s1), o.tally(s2), 1, max_permille, band, LO, HI, 1, pd.RESCUE_PERMILLE, 2, 8)


def rescued_rows(mixed):
    """-> [(class, set, strand, the mate, its alignment with its steps, its record's length)] of the rescued mates"""
    o, P = oracle()
    s1, s2, what, w = wanted(mixed, 8, 1000)
    out = []
    for i, (kind, _) in enumerate(w["pairs"]):
        if kind not in (pao.RESCUED_1, pao.RESCUED_2):
            continue
        m = 1 if kind == pao.RESCUED_1 else 2
        seq, row = (s1, s2)[m - 1][i], w["rows" + str(m)][i]
        assert row[4] == 0
        out.append((what[i][0], m, int(row[1]), seq, P.A.align_row(seq, row, 8), o.lens[int(row[0])]))
    return out


def test_every_class_of_rescued_mate_occurs_on_both_strands_and_from_both_sets():
    rows = rescued_rows(True)
    classes = {
        "an insertion run of at least 2": lambda seq, a, ln: any(n >= 2 for _, n in ao.insertion_runs(a["steps"])),
        "a deletion": lambda seq, a, ln: a["deletions"] >= 1,
        "over the begin by 3 columns": lambda seq, a, ln: sum(mv == ao.DIAG and c < 0 for mv, _, c in a["steps"]) >= 3 and a["ref_begin"] < 0,
        "over the end by 3 columns": lambda seq, a, ln: sum(mv == ao.DIAG and c >= ln for mv, _, c in a["steps"]) >= 3 and a["ref_end"] > ln,
        "an N": lambda seq, a, ln: "N" in seq,
    }
    for name, holds in classes.items():
        hit = [(m, strand) for _, m, strand, seq, a, ln in rows if holds(seq, a, ln)]
        assert len(hit) >= 20, (name, len(hit))
        assert set(hit) == {(1, 0), (1, 1), (2, 0), (2, 1)}, (name, sorted(set(hit)))


def test_the_uniform_form_holds_the_same_pairs_with_the_anchor_first():
    s1, s2, what, w = wanted(False, 8, 1000)
    m1, m2, what2, wm = wanted(True, 8, 1000)
    assert what == what2 and all(len(s) == 150 for s in s1) and len({len(s) for s in s2}) > 20
    assert all((a, b) == ((x, y) if t[1] == 2 else (y, x)) for a, b, x, y, t in zip(s1, s2, m1, m2, what))
    assert int(np.isin(w["pairs"][:, 0], (pao.RESCUED_1, pao.RESCUED_2)).sum()) == int(np.isin(wm["pairs"][:, 0], (pao.RESCUED_1, pao.RESCUED_2)).sum()) >= 100
    assert not (w["pairs"][:, 0] == pao.RESCUED_1).any()


def test_every_refusal_and_every_kind_occurs():
    s1, s2, what, w = wanted(True, 8, 1000)
    for why in ("tie", "cut", "short"):
        assert w["why"].count(why) >= 20, (why, w["why"].count(why))
    kinds = np.bincount(w["pairs"][:, 0], minlength=7)
    assert (kinds >= 20).all(), kinds.tolist()
    assert int(w["pair_rec"][:, 2].sum()) >= 20          # cross
    assert int(w["pair_rec"][:, :5].sum()) + w["none"] == len(s1)


def test_the_aligned_cut_settles_mates_the_ungapped_cut_rejects():
    s1, s2, what, w0 = wanted(True, 0, 30)
    _, _, _, w8 = wanted(True, 8, 30)
    differ = np.nonzero(w0["pairs"][:, 0] != w8["pairs"][:, 0])[0]
    assert len(differ) >= 20, len(differ)
    placed = [i for i in differ if what[i][0] == "indel_placed"]
    assert len(placed) >= 20 and all(w8["pairs"][i, 0] == pao.PROPER and w0["pairs"][i, 0] in (pao.SINGLE_1, pao.SINGLE_2) for i in placed)
