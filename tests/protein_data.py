"""Reads for the forms of the protein kernel ("The protein kernel's bit-table forms"): a database that holds ALL SIX frames of
one random DNA, so that a read cut from that DNA has database peptides in every frame, and from it the reads whose answer hangs on one
detail of `pfilter_kernel` -- hits that reach the threshold only summed over the three lanes of a read, an invalid base at every offset
of a codon, windows that come back behind a stop codon on one strand alone, read counts around the 256-read group.

Pure Python on oracle/prot_bait_ref.py (the string-level Spec P), seeded; no GPU, no C oracle.  tests/test_protein_data.py holds every
builder to its conditions with that reference."""
from __future__ import annotations

import functools
import random
from types import SimpleNamespace
from typing import List, Sequence, Set, Tuple

from oracle import kmer_bait_ref as kb
from oracle import prot_bait_ref as pr

SEED = 20261020
DB_BASES = 3000
group_edge_counts = [1, 255, 256, 257, 511, 513, 768]          # around the 256 reads (768 lanes, 8 bitmap words) of a workgroup's turn
FWD_STOP, REV_STOP, MID_N = "TAA", "TTA", "N"                   # regrow_reads' three breaks: TAA is '*' (in every table but 14), TTA is L and its reverse complement is TAA
REGROW_KINDS = (FWD_STOP, REV_STOP, MID_N)
REGROW_EXTRA = 4                                                # codons beyond kp in a regrow read: 5 windows a frame


def six_frame_db(seed: int, n_bases: int, code: int) -> Tuple[str, str]:
    """-> (D, protein FASTA): a random DNA and the database whose six records are its six translations, '*' left where a stop codon
    stands (it breaks windows as every invalid residue does, Spec P1)."""
    rng = random.Random(seed)
    D = "".join(rng.choices("ACGT", k=n_bases))
    return D, "".join(f">frame{i}\n{p}\n" for i, p in enumerate(pr.six_frames(D, code)))


def split_hit_reads(D: str, kp: int, code: int, bait: Set[int]) -> List[str]:
    """Every substring of D of 3 kp + 2 bases with exactly 6 hits.  Such a read holds ONE window in each of its six frames (kp codons fit
    from offset 0, 1 and 2), so 6 hits are one hit a frame: a lane of the kernel (one codon phase, both strands) counts at most 2."""
    L = 3 * kp + 2
    return [D[i:i + L] for i in range(len(D) - L + 1) if pr.read_hits(D[i:i + L], kp, code, bait) == 6]


def n_scan(read: str) -> List[str]:
    """The len(read) copies of `read` with base i replaced by N.  Of a split-hit read: phase p spans bases p .. p + 3 kp - 1, so an N on
    base 0 or the last base breaks one phase (4 hits left), on base 1 or the last but one two (2 left), anywhere else all three."""
    return [read[:i] + "N" + read[i + 1:] for i in range(len(read))]


def n_scan_hits(kp: int) -> List[int]:
    return [4, 2] + [0] * (3 * kp - 2) + [2, 4]


def regrow_reads(D: str, kp: int, code: int, bait: Set[int] = None, max_base: int = 6) -> SimpleNamespace:
    """Reads of 3 (kp + 4) + 2 bases of D with no stop codon in any frame (5 windows a frame: 30 hits), and of each of them, for every
    codon c of phase 0 and each kind of REGROW_KINDS, the read with that codon broken: replaced by TAA (a stop on the forward strand, L
    on the reverse one), by TTA (L forward, a stop on the reverse strand), or its middle base by N (invalid on both).  The windows of
    the broken strand that lie wholly before or wholly behind codon c survive; those across it do not.
    -> base (the unbroken reads, `max_base` of them spread over D), seqs (the broken ones), origin ((index into base, c, kind) each)."""
    assert pr.translate_codon(FWD_STOP, code) == "*" and pr.translate_codon(pr.revcomp_any(FWD_STOP), code) in pr.AA
    assert pr.translate_codon(REV_STOP, code) in pr.AA and pr.translate_codon(pr.revcomp_any(REV_STOP), code) == "*"
    n_cod = kp + REGROW_EXTRA
    L = 3 * n_cod + 2
    whole = [D[i:i + L] for i in range(len(D) - L + 1) if "*" not in "".join(pr.six_frames(D[i:i + L], code))]
    if bait is not None:
        assert all(pr.read_hits(s, kp, code, bait) == 6 * (REGROW_EXTRA + 1) for s in whole)
    step = max(1, len(whole) // max_base)
    base = whole[::step][:max_base]
    seqs, origin = [], []
    for b, s in enumerate(base):
        for c in range(n_cod):
            for kind in REGROW_KINDS:
                cod = s[3 * c] + "N" + s[3 * c + 2] if kind == MID_N else kind
                seqs.append(s[:3 * c] + cod + s[3 * c + 3:])
                origin.append((b, c, kind))
    return SimpleNamespace(kp=kp, code=code, n_codons=n_cod, base=base, seqs=seqs, origin=origin)


def ragged_twin(seqs: Sequence[str], extra: str = "AC") -> List[str]:
    """`seqs` and one read of another length behind them: a set of equal-length reads then takes the kernels' `offsets` path and not
    `b0 = r * L` (Reads.from_packed finds a uniform set by itself).  `extra` is too short for a codon window: it never has a hit."""
    assert all(len(s) != len(extra) for s in seqs)
    return list(seqs) + [extra]


def group_edge_sets(split: Sequence[str], seed: int = SEED) -> List[List[str]]:
    """one set of n passing split-hit reads for every n of group_edge_counts (drawn with replacement: a dense bitmap)"""
    rng = random.Random(seed)
    return [rng.choices(list(split), k=n) for n in group_edge_counts]


def wrap_db(seed: int, kp: int, code: int, n: int = 4) -> SimpleNamespace:
    """A database of n one-window records whose keys all have the table's LAST slot as their home (1024 slots: Spec P5's minimum), so
    that linear probing lays all but the smallest of them at the table's start, and for each the two reads (a back-translation and its
    reverse complement) that hold that peptide alone.  A probe that does not wrap at the table's end finds only the smallest key.
    -> fasta, peptides (ascending by key), seqs, slots."""
    rng = random.Random(seed)
    slots, found = 1024, {}
    while len(found) < n:
        pep = "".join(rng.choices(pr.AA, k=kp))
        if kb.fold32(pr.pep_code(pep)) & (slots - 1) == slots - 1:
            found[pr.pep_code(pep)] = pep
    peptides = [found[v] for v in sorted(found)]
    fasta = "".join(f">w{i}\n{p}\n" for i, p in enumerate(peptides))
    assert pr.table_slots(fasta, kp) == slots
    seqs = []
    for p in peptides:
        dna = pr.back_translate(p, code, rng)
        seqs += [dna, pr.revcomp_any(dna)]
    return SimpleNamespace(kp=kp, code=code, fasta=fasta, peptides=peptides, seqs=seqs, slots=slots)


@functools.lru_cache(maxsize=8)
def cached_db(code: int = 5, n_bases: int = DB_BASES, seed: int = SEED) -> SimpleNamespace:
    """the six-frame database of (seed, n_bases, code), shared by the tests of a module; `bait(kp)` is its reference key set"""
    D, fa = six_frame_db(seed, n_bases, code)
    return SimpleNamespace(D=D, fasta=fa, code=code, bait=functools.lru_cache(maxsize=None)(lambda kp: frozenset(pr.bait_set(fa, kp))))


@functools.lru_cache(maxsize=8)
def cached_split(kp: int, code: int = 5) -> Tuple[str, ...]:
    db = cached_db(code)
    return tuple(split_hit_reads(db.D, kp, code, db.bait(kp)))


@functools.lru_cache(maxsize=8)
def cached_regrow(kp: int, code: int = 5) -> SimpleNamespace:
    db = cached_db(code)
    return regrow_reads(db.D, kp, code)
