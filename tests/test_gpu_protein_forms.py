"""The four instantiations of `pfilter_kernel` (key bit table in LDS | read through L2, all hits | early exit) against the six-frame
oracle (oracle/kmer_bait_oracle.c's Spec-P functions, pinned to oracle/prot_bait_ref.py), on the reads of tests/protein_data.py: hits
that reach the threshold only as the sum over a read's three lanes, an invalid base at every offset, windows that regrow behind a
break on one strand, read counts at the 256-read group, a grid that takes a second turn, bit tables forced from saturated (2^8 words
for >= 4000 keys: the open-address table decides nearly every probe) to 2^24 words, and the default sizing on both sides of its switch.
`MF_KBLOOM_LOG2W` is set around the construction of the protein set only, and `info.bloom_words` says which form the set took
(<= 16384 words: LDS).  Bar: bit-exact hits, bits and n_pass, for the counting call and the early-exit call, uniform and ragged."""
import functools
import random
import re

import numpy as np
import pytest

from tests import protein_data as pd
from tests.util_data import bits_to_bool, make_protein_bait, make_reads, revcomp

pytestmark = pytest.mark.gpu

FORMS = [None, 8, 11, 14, 15, 18, 24]           # log2 words of the key bit table: None the default sizing, <= 14 staged in LDS, >= 15 in L2
KPS = [4, 7, 9]
CODE = 5
LDS_WORDS = 16384


def _form_id(lg):
    return "default" if lg is None else "lg%d" % lg


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


def protein_set(mf, monkeypatch, fasta, kp, code, lg):
    """the protein set of (fasta, kp, code) with its bit table forced to 2^lg words (None: sized by protset_new); the variable is set for
    the construction alone -- the nucleotide builder reads it too"""
    with monkeypatch.context() as m:
        if lg is None:
            m.delenv("MF_KBLOOM_LOG2W", raising=False)
        else:
            m.setenv("MF_KBLOOM_LOG2W", str(lg))
        ks = mf.KmerSet.protein_from_text(fasta, kp, code)
    if lg is not None:
        assert ks.info.bloom_words == 1 << lg
    return ks


@functools.lru_cache(maxsize=None)
def oracle_table(fasta, kp):
    from oracle import oracle_lib
    return oracle_lib.OracleTable(fasta, kp, protein=True)


class ReadSet:
    """a read set, packed once, with the oracle's answers per (database, kp, code, threshold) and its device copy: computed once, shared
    by every form, never written to"""

    def __init__(self, seqs):
        from oracle import oracle_lib
        self.n = len(seqs)
        self.lens = {len(s) for s in seqs}
        self.R = oracle_lib.OracleReads.from_seqs(seqs)
        self._want, self._dev = {}, None

    def want(self, fasta, kp, code, thr):
        from oracle import oracle_lib
        key = (fasta, kp, code, thr)
        if key not in self._want:
            obits, ohits = oracle_lib.pfilter_reads(oracle_table(fasta, kp), self.R, code, thr, threads=8)
            obits.flags.writeable = ohits.flags.writeable = False
            self._want[key] = (obits, ohits)
        return self._want[key]

    def device(self, mf):
        if self._dev is None:
            self._dev = mf.Reads.from_packed(self.R.words, self.R.offsets, self.R.npos)
            assert self._dev.info.n_reads == self.n
            assert self._dev.info.uniform_len == (next(iter(self.lens)) if len(self.lens) == 1 else 0)          # the twin takes the path it is meant for
        return self._dev


def twins(seqs):
    """the read set as it is (one length: `b0 = r * L`) and with one short read behind it (the `offsets` path)"""
    assert len({len(s) for s in seqs}) == 1
    return {"uniform": ReadSet(seqs), "ragged": ReadSet(pd.ragged_twin(seqs))}


def hold(mf, ks, fasta, kp, code, rs, thr, ctx):
    """the counting call and the early-exit call of one (set, read set, threshold) against the oracle -> (reads that pass, hits)"""
    obits, ohits = rs.want(fasta, kp, code, thr)
    n_pass = int(bits_to_bool(obits, rs.n).sum())
    reads = rs.device(mf)
    bits, hits, st = mf.filter_reads(ks, reads, thr, want_hits=True)
    assert np.array_equal(hits, ohits), (ctx, thr, "hits", np.nonzero(hits != ohits)[0][:10].tolist())
    assert np.array_equal(bits, obits), (ctx, thr, "bits")
    assert st.n_pass == n_pass, (ctx, thr, "n_pass", st.n_pass, n_pass)
    bits2, _, st2 = mf.filter_reads(ks, reads, thr)                                  # early exit: a lane stops at `thr` hits of its own
    assert np.array_equal(bits2, obits), (ctx, thr, "early-exit bits", np.nonzero(bits2 != obits)[0][:10].tolist())
    assert st2.n_pass == n_pass, (ctx, thr, "early-exit n_pass", st2.n_pass, n_pass)
    return n_pass, hits


# ------------------------------------------------------------------------------------------------ the read sets (one a module run)
@functools.lru_cache(maxsize=None)
def split_sets(kp):
    return twins(list(pd.cached_split(kp, CODE)))


@functools.lru_cache(maxsize=None)
def scan_sets(kp):
    split = pd.cached_split(kp, CODE)
    picked = split[::len(split) // 40][:40]
    assert len(picked) == 40
    return twins([t for s in picked for t in pd.n_scan(s)])


@functools.lru_cache(maxsize=None)
def regrow_sets(kp):
    rg = pd.cached_regrow(kp, CODE)
    seqs = rg.base + rg.seqs
    return twins(seqs + [revcomp(s) for s in seqs])          # the same breaks seen from the other strand: run_r sees what run_f saw


@functools.lru_cache(maxsize=None)
def edge_sets(kp):
    return [twins(s) for s in pd.group_edge_sets(pd.cached_split(kp, CODE))]


@functools.lru_cache(maxsize=None)
def stride_sets(kp, n):
    split = pd.cached_split(kp, CODE)
    rng = random.Random(pd.SEED + n)
    L = 3 * kp + 2
    junk = "".join(rng.choices("ACGT", k=n * L))
    return twins([rng.choice(split) if rng.random() < 0.5 else junk[i * L:(i + 1) * L] for i in range(n)])


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("lg", FORMS, ids=_form_id)
@pytest.mark.parametrize("kp", KPS)
def test_split_hits_pass_by_the_sum(mf, ol, monkeypatch, kp, lg):
    """every read has 6 hits, at most 2 on a lane: thresholds 3 .. 6 are reached only by the sum over the three lanes in `s_hits`, 7 by
    nothing.  A kernel that lets a lane's own count decide, or loses the count of a lane that left its loop early, fails here."""
    db = pd.cached_db(CODE)
    ks = protein_set(mf, monkeypatch, db.fasta, kp, CODE, lg)
    assert ks.info.n_keys >= 4000
    for twin, rs in split_sets(kp).items():
        n_split = rs.n - (twin == "ragged")                                          # (the twin's extra read is too short for a window)
        assert n_split >= 200
        for thr in range(1, 8):
            n_pass, hits = hold(mf, ks, db.fasta, kp, CODE, rs, thr, (kp, lg, twin))
            assert n_pass == (n_split if thr <= 6 else 0), (kp, lg, twin, thr, n_pass)
            assert np.all(hits[:n_split] == 6)


@pytest.mark.parametrize("lg", FORMS, ids=_form_id)
@pytest.mark.parametrize("kp", KPS)
def test_invalid_base_at_every_offset(mf, ol, monkeypatch, kp, lg):
    """40 split-hit reads with an N on every base in turn: at each of the three offsets inside a codon, in every phase, at both read ends"""
    db = pd.cached_db(CODE)
    ks = protein_set(mf, monkeypatch, db.fasta, kp, CODE, lg)
    L = 3 * kp + 2
    for twin, rs in scan_sets(kp).items():
        for thr in (1, 2, 4):
            n_pass, hits = hold(mf, ks, db.fasta, kp, CODE, rs, thr, (kp, lg, twin))
            assert np.array_equal(hits[:40 * L].reshape(40, L), np.tile(np.array(pd.n_scan_hits(kp), dtype=np.uint32), (40, 1)))
            assert n_pass == 40 * {1: 4, 2: 4, 4: 2}[thr]


@pytest.mark.parametrize("lg", FORMS, ids=_form_id)
@pytest.mark.parametrize("kp", KPS)
def test_windows_regrow_behind_a_break(mf, ol, monkeypatch, kp, lg):
    """a forward stop, a stop of the reverse strand alone and an N in every codon of phase 0, and the reverse complements of those
    reads: the windows of the broken strand come back exactly kp codons behind the break, those of the other strand never left"""
    db = pd.cached_db(CODE)
    ks = protein_set(mf, monkeypatch, db.fasta, kp, CODE, lg)
    for twin, rs in regrow_sets(kp).items():
        for thr in (1, 10, 20):
            n_pass, hits = hold(mf, ks, db.fasta, kp, CODE, rs, thr, (kp, lg, twin))
        assert len(set(hits.tolist())) >= 8 and int(hits.max()) == 6 * (pd.REGROW_EXTRA + 1)


@pytest.mark.parametrize("lg", [8, 15], ids=_form_id)
def test_group_edges_dense(mf, ol, monkeypatch, lg):
    """1 .. 768 reads, all of them passing: three lanes a read up to the last lane of a workgroup's turn, the ballot words of a group
    that is not full, a second and a third group"""
    kp = 7
    db = pd.cached_db(CODE)
    ks = protein_set(mf, monkeypatch, db.fasta, kp, CODE, lg)
    for n, tw in zip(pd.group_edge_counts, edge_sets(kp)):
        for twin, rs in tw.items():
            for thr in (1, 6, 7):
                n_pass, _ = hold(mf, ks, db.fasta, kp, CODE, rs, thr, (n, lg, twin))
                assert n_pass == (n if thr <= 6 else 0), (n, lg, twin, thr, n_pass)


@pytest.mark.parametrize("lg", [None, 15, 8], ids=_form_id)
def test_grid_stride_second_turn(mf, ol, monkeypatch, lg):
    """launch_pfilter starts two workgroups a CU and a workgroup takes 256 reads a turn, so the grid-stride loop takes a second turn
    only beyond 2 * CUs * 256 reads: the read count is that (from the device's CU count) and 8928 more -- 140 000 on 256 CUs"""
    kp = 9
    n_cu = int(re.search(r"(\d+) CUs", mf.device_name(0)).group(1))
    n = 2 * n_cu * 256 + 8928
    db = pd.cached_db(CODE)
    ks = protein_set(mf, monkeypatch, db.fasta, kp, CODE, lg)
    for twin, rs in stride_sets(kp, n).items():
        for thr in (1, 4):
            n_pass, hits = hold(mf, ks, db.fasta, kp, CODE, rs, thr, (n, lg, twin))
            assert 0.4 * n < n_pass < 0.6 * n                                        # the split-hit half; both turns hold reads of both kinds
            assert hits[2 * n_cu * 256:n].max() == 6 and hits[2 * n_cu * 256:n].min() == 0


@functools.lru_cache(maxsize=None)
def switch_db(kp):
    """256 records of 512 + kp - 1 random residues (2^17 windows exactly), a record of one window more, and the DNA of forty of them"""
    from oracle import prot_bait_ref as pr
    rng = random.Random(pd.SEED + kp)
    prots = ["".join(rng.choices(pr.AA, k=512 + kp - 1)) for _ in range(256)]
    at = "".join(f">p{i}\n{p}\n" for i, p in enumerate(prots))
    above = at + ">one\n" + "".join(rng.choices(pr.AA, k=kp)) + "\n"
    genes = "".join(f">g{i}\n{pr.back_translate(p, CODE, rng)}\n" for i, p in enumerate(prots[:40]))
    return {"at": at, "above": above}, ReadSet(make_reads(genes, 5000, seed=kp, uniform=False, mito_frac=0.3))


@pytest.mark.parametrize("side", ["at", "above"])
def test_default_sizing_at_the_switch(mf, ol, monkeypatch, side):
    """2^17 windows: the largest database whose bit table is staged in LDS, at its largest size (2^14 words: 64 KiB beside the codon
    table); one window more: the table moves to L2"""
    kp = 8
    dbs, rs = switch_db(kp)
    fasta = dbs[side]
    ks = protein_set(mf, monkeypatch, fasta, kp, CODE, None)
    info = ks.info
    if side == "at":
        assert info.n_windows == 1 << 17 and info.bloom_words == LDS_WORDS
    else:
        assert info.n_windows == (1 << 17) + 1 and info.bloom_words > LDS_WORDS
    t = oracle_table(fasta, kp)
    assert info.n_keys == t.n_keys and np.array_equal(ks.export_table(), t.keys)
    for thr in (1, 2, 9):
        n_pass, hits = hold(mf, ks, fasta, kp, CODE, rs, thr, (side,))
    assert int(hits.max()) > 20 and rs.R.npos.size > 100


@pytest.mark.parametrize("kp,code", [(4, 1), (7, 5), (9, 2), (12, 9), (6, 14), (8, 4), (7, 13)])
def test_genetic_codes_in_the_l2_form(mf, ol, monkeypatch, kp, code):
    """the (kp, code) pairs of test_gpu_protein.test_six_frame_filter_matches_oracle, ragged reads with N's, with the bit table in L2:
    the run counters are fed from every table's flag words"""
    prot_fa, gene_fa = make_protein_bait(code=code)
    ks = protein_set(mf, monkeypatch, prot_fa, kp, code, 15)
    rs = ReadSet(make_reads(gene_fa, 5000, seed=kp * 31 + code, uniform=False, mito_frac=0.4))
    for thr in (1, 2, 9):
        n_pass, hits = hold(mf, ks, prot_fa, kp, code, rs, thr, (kp, code))
    assert int(hits.max()) > 20


@pytest.mark.parametrize("lg", FORMS, ids=_form_id)
@pytest.mark.parametrize("kp", [4, 9, 12])
def test_probe_wraps_at_the_table_end(mf, ol, monkeypatch, kp, lg):
    """four keys whose home is the table's last slot: three of them lie at its start and are found only by a probe that wraps"""
    w = pd.wrap_db(pd.SEED, kp, CODE)
    ks = protein_set(mf, monkeypatch, w.fasta, kp, CODE, lg)
    assert np.array_equal(ks.export_table(), oracle_table(w.fasta, kp).keys)
    for twin, rs in twins(w.seqs).items():
        n_pass, hits = hold(mf, ks, w.fasta, kp, CODE, rs, 1, (kp, lg, twin))
        assert n_pass == 8 and np.all(hits[:8] >= 1)
