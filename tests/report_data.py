"""What the GPU tests of the reports on the baited reads share (test_gpu_assign.py, test_gpu_group_assign.py, test_gpu_depth.py):
bait and read generators, the keys of a read's windows as the oracles count them, the upload of a read set, and the module fixtures
(imported by name where they are used)."""
import random

import pytest

from oracle import kmer_bait_ref as kb
from oracle import prot_bait_ref as pr
from tests.util_data import bait_records, make_bait


def mutate(seq, rate, seed):
    rng = random.Random(seed)
    s = list(seq)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = rng.choice([b for b in "ACGT" if b != s[i]])
    return "".join(s)


def fasta(records):
    return "".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))) for n, s in records)


def eight_record_bait():
    """8 records: the synthetic mitogenome, copies mutated at 1 % and 10 %, an exact duplicate (every key of it shared), a record
    shorter than k, the second record of the synthetic bait (IUPAC codes, N), a 10 % copy of it, an unrelated random record"""
    r = bait_records(make_bait())
    g = r[0][:6000]
    rng = random.Random(5)
    m1 = mutate(g, 0.01, 1)
    return fasta([("mito desc", g), ("mito_1pc", m1), ("mito_10pc", mutate(g, 0.10, 2)), ("mito_1pc_dup", m1), ("tiny", "ACGTTGCA"),
                  ("rec2", r[1]), ("rec2_10pc", mutate(kb._norm(r[1]).replace("N", "A"), 0.10, 3)), ("rand", "".join(rng.choices("ACGT", k=3000)))])


def keys_nuc(seq, k):
    s = kb._norm(seq)
    return [kb.canonical_code(s[p:p + k]) for p in range(len(s) - k + 1) if "N" not in s[p:p + k]]


def keys_prot(seq, kp, code):
    """the peptide key of every hits-eligible (frame, window) pair of a read"""
    out = []
    for pep in pr.six_frames(seq, code):
        for i in range(len(pep) - kp + 1):
            v = pr.pep_code(pep[i:i + kp])
            if v is not None:
                out.append(v)
    return out


def upload(mf, ol, seqs):
    R = ol.OracleReads.from_seqs(seqs)
    return mf.Reads.from_packed(R.words, R.offsets, R.npos)


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
