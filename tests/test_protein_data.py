"""The builders of tests/protein_data.py against the string-level Spec P (oracle/prot_bait_ref.py) alone: the six-frame database is
large enough to load a small bit table, the split-hit reads have one hit a frame, an N on base i leaves the hits its place allows, a
broken codon lets windows regrow behind it, a probe for the wrapping keys has to wrap.  Conditions on the INPUT of
tests/test_gpu_protein_forms.py, not on the kernel: no GPU."""
import pytest

from oracle import kmer_bait_ref as kb
from oracle import prot_bait_ref as pr
from tests import protein_data as pd

KPS = [4, 7, 9]                   # the kp of test_gpu_protein_forms.py (kp = 12: too few split-hit positions in 3000 bases to rely on)
CODE = 5


@pytest.mark.parametrize("kp", KPS)
def test_six_frame_db_loads_a_small_bit_table(kp):
    db = pd.cached_db(CODE)
    recs = pr.protein_records(db.fasta)
    assert len(db.D) == pd.DB_BASES and recs == pr.six_frames(db.D, CODE) and any("*" in r for r in recs)
    assert len(db.bait(kp)) >= 4000               # 2^7 blocks at log2w 8: about 30 keys a 64-bit block, the table decides
    assert pd.six_frame_db(pd.SEED, pd.DB_BASES, CODE) == (db.D, db.fasta)            # seeded


@pytest.mark.parametrize("kp", KPS)
def test_split_hit_reads_have_one_hit_a_frame(kp):
    db = pd.cached_db(CODE)
    split = pd.cached_split(kp, CODE)
    print(kp, len(split), "split-hit positions of", len(db.D) - (3 * kp + 2) + 1)
    assert len(split) >= 200
    bait = db.bait(kp)
    for s in split[::7]:
        assert len(s) == 3 * kp + 2
        frames = pr.six_frames(s, CODE)
        assert [len(f) for f in frames] == [kp] * 6                                   # one window a frame ...
        assert all(pr.pep_code(f) in bait for f in frames)                            # ... and each of them a hit: at most 2 a lane
        assert pr.read_hits(pr.revcomp_any(s), kp, CODE, bait) == 6


@pytest.mark.parametrize("kp", KPS)
def test_n_scan_hit_pattern(kp):
    db = pd.cached_db(CODE)
    bait = db.bait(kp)
    want = pd.n_scan_hits(kp)
    assert want[:3] == [4, 2, 0] and want[-3:] == [0, 2, 4] and len(want) == 3 * kp + 2 and not any(want[2:-2])
    split = pd.cached_split(kp, CODE)
    for s in split[:200]:
        scan = pd.n_scan(s)
        assert len(scan) == len(s) and all(t.count("N") == 1 and t[i] == "N" for i, t in enumerate(scan))
        assert [pr.read_hits(t, kp, CODE, bait) for t in scan] == want, s


@pytest.mark.parametrize("kp", KPS)
def test_regrow_reads_lose_and_regain_windows(kp):
    db = pd.cached_db(CODE)
    bait = db.bait(kp)
    rg = pd.cached_regrow(kp, CODE)
    n_cod = kp + pd.REGROW_EXTRA
    assert len(rg.base) == 6 and len(rg.seqs) == 6 * n_cod * 3
    full = 6 * (pd.REGROW_EXTRA + 1)
    for s in rg.base:
        assert len(s) == 3 * n_cod + 2 and pr.read_hits(s, kp, CODE, bait) == full
    hits = [pr.read_hits(s, kp, CODE, bait) for s in rg.seqs]
    for b in range(len(rg.base)):
        for kind in pd.REGROW_KINDS:
            over_c = [h for h, (ob, c, ok) in zip(hits, rg.origin) if ob == b and ok == kind]
            assert len(over_c) == n_cod and max(over_c) < full
            assert len(set(over_c)) >= 3, (kp, b, kind, over_c)       # windows before and behind the break survive, those across it do not
    # the three breaks on the strands they are meant for: the phase-0 frame of the forward strand, and the reverse frame of the same codons
    s = rg.base[0]
    for c in (0, n_cod // 2, n_cod - 1):
        fwd, rev, mid = (rg.seqs[3 * c + j] for j in range(3))
        rc_frame = lambda t: pr.translate(pr.revcomp_any(t)[2:], CODE)            # the codons 0, 3, 6 .. of the read, read backwards
        assert pr.translate(fwd, CODE)[c] == "*" and "*" not in rc_frame(fwd)
        assert "*" not in pr.translate(rev, CODE) and rc_frame(rev)[n_cod - 1 - c] == "*"
        assert pr.translate(mid, CODE)[c] == "X" and rc_frame(mid)[n_cod - 1 - c] == "X"
        assert len({fwd, rev, mid, s}) == 4


def test_group_edge_sets_and_ragged_twin():
    split = pd.cached_split(7, CODE)
    sets = pd.group_edge_sets(split)
    assert [len(s) for s in sets] == pd.group_edge_counts == [1, 255, 256, 257, 511, 513, 768]
    assert all(r in split for s in sets for r in s)
    twin = pd.ragged_twin(sets[0])
    assert twin[:-1] == sets[0] and len(twin[-1]) < 12 and len(twin[-1]) != len(twin[0])
    assert pr.read_hits(twin[-1], 4, CODE, pd.cached_db(CODE).bait(4)) == 0
    with pytest.raises(AssertionError):
        pd.ragged_twin(["AC", "ACGT"])


@pytest.mark.parametrize("kp", [4, 9, 12])
def test_wrap_db_keys_lie_before_their_home_slot(kp):
    w = pd.wrap_db(pd.SEED, kp, CODE)
    tab = pr.table_layout(w.fasta, kp)
    keys = [pr.pep_code(p) for p in w.peptides]
    assert len(tab) == w.slots == 1024 and keys == sorted(keys) and len(set(keys)) == 4
    assert all(kb.fold32(k) & 1023 == 1023 for k in keys)
    assert [tab.index(k) for k in keys] == [1023, 0, 1, 2]                            # three of the four are found only by wrapping
    bait = pr.bait_set(w.fasta, kp)
    assert len(w.seqs) == 8 and all(len(s) == 3 * kp and pr.read_hits(s, kp, CODE, bait) >= 1 for s in w.seqs)
