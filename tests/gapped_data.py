"""Inputs of the gapped-consensus tests (test_gapped_oracle.py, test_gpu_gapped.py), from seeded generators: the reconstruction case --
a one-record bait, a sample that differs from it by a deletion, an insertion and three substitutions, and reads that tile the sample --
and the stacks of identical reads whose insertions agree, differ in one letter, or are carried by exactly half."""
import random

import numpy as np

from tests.util_data import revcomp

BAIT_LEN, READ_LEN, DEL_AT, INS_AT, SUBS = 1500, 150, 400, 900, (200, 700, 1200)


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def reconstruction(band, seed=61):
    """-> (bait, sample, reads): the sample is the bait without min(3, band) bases at 400, with min(5, band) random bases more at 900 and
    with three substitutions; the 150-base reads start at every third offset of the sample, on random strands: 451 reads"""
    rng = random.Random(seed)
    bait = _rand(rng, BAIT_LEN)
    s = list(bait)
    for p in SUBS:
        s[p] = rng.choice([b for b in "ACGT" if b != s[p]])
    # an inserted stretch that neither repeats the base before it nor runs into the base behind it: the rule's order of moves then
    # leaves the insertion where it was made
    ins = _rand(rng, min(5, band))
    while ins[0] == s[INS_AT - 1] or ins[-1] == s[INS_AT] or ins[0] == s[INS_AT]:
        ins = _rand(rng, min(5, band))
    sample = "".join(s[:DEL_AT]) + "".join(s[DEL_AT + min(3, band):INS_AT]) + ins + "".join(s[INS_AT:])
    reads = [sample[a:a + READ_LEN] for a in range(0, len(sample) - READ_LEN + 1, 3)]
    assert len(reads) == 451
    return bait, sample, [r if rng.random() < 0.5 else revcomp(r) for r in reads]


def stack_bait(seed=67):
    return _rand(random.Random(seed), 600)


def stack_reads(bait, carriers, plain, inserted="TCCT", other=None, n_other=0, at=250, start=200, length=150):
    """`plain` copies of bait[start : start + length], `carriers` copies of the same stretch with `inserted` behind position `at` - 1 (cut
    to the same length), and n_other copies with `other` inserted instead.  The insertion lies a third into the read: placement goes by
    the longer part behind it.  The default letters (and TGCT as `other`) match the bait of stack_bait nowhere around position 250, so
    the rule's order of moves leaves each insertion one run of four; letters that match by chance would split it."""
    def carrier(ins):
        return (bait[start:at] + ins + bait[at:start + length])[:length]
    return [bait[start:start + length]] * plain + [carrier(inserted)] * carriers + ([carrier(other)] * n_other if other else [])


def structured(mf, want, band):
    """the oracle's unclamped arrays as the arrays the wrapper gives (valid where nothing is clamped)"""
    P = len(want["depth"])
    indels = np.zeros(P, dtype=mf.INDEL)
    for i, f in enumerate(("del", "ins", "ins_bases")):
        indels[f] = want["indels"][:, i]
    ins = np.zeros((P, 2 * band), dtype=mf.PILEUP)
    for i, f in enumerate("acgt"):
        ins[f] = want["ins_pile"][:, :, i]
    return want["depth"].astype(np.uint32), indels, ins
