"""Inputs of the extended-record tests (test_extend_data.py, test_extend_oracle.py, test_gpu_extend.py), from seeded generators: the
reconstruction case -- a bait cut out of the middle of a random genome and reads that tile the genome across both of its ends -- and
the `ends` set: three records that are adjacent in global positions, and reads built around every end of every record."""
import random

import numpy as np

from tests.util_data import revcomp

GENOME_LEN, BAIT_LO, BAIT_HI, READS_LO, READS_HI = 1200, 500, 700, 300, 900
# (k, band, E, min_depth, read length, step between the reads' offsets) of the three reconstruction shapes
SHAPES = ((31, 4, 64, 3, 100, 4), (41, 8, 64, 3, 100, 3), (21, 0, 16, 3, 60, 4))
CUT = 30                      # the cut of the `ends` set: it rejects the 6 % copies
MIN_DEPTH = 3                 # the depth its stacks are built around
END_LENS = (300, 200, 400)
TIE_END, TIE_AT = (0, 1), 7           # the end (record, side) that only the tie stacks reach, and the column they differ in
DEPTH_END = (1, 0)                    # the end that only the depth stacks reach: MIN_DEPTH reads over 20 columns, MIN_DEPTH - 1 over 40
OPEN_ENDS = ((0, 0), (1, 1), (2, 0), (2, 1))          # the ends every other group reaches


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _strand(rng, s):
    return s if rng.random() < 0.5 else revcomp(s)


def reconstruction(read_len=100, step=4, seed=71):
    """-> (genome, bait, reads): the bait is genome[500:700]; the reads are read_len bases from genome[300:900] at every step-th offset,
    on random strands"""
    rng = random.Random(seed)
    genome = _rand(rng, GENOME_LEN)
    reads = [genome[a:a + read_len] for a in range(READS_LO, READS_HI - read_len + 1, step)]
    return genome, genome[BAIT_LO:BAIT_HI], [_strand(rng, r) for r in reads]


def ends_bait(seed=73):
    """-> (FASTA text, [record sequences], [flank before, flank behind] of every record): three records, adjacent in global positions; each
    was cut out of a random stretch of its own, whose flanks are what the sample holds beside it"""
    rng = random.Random(seed)
    recs, flanks = [], []
    for n in END_LENS:
        s = _rand(rng, 150 + n + 150)
        recs.append(s[150:150 + n])
        flanks.append((s[:150], s[150 + n:]))
    text = "".join(">e%d\n%s\n" % (j, r) for j, r in enumerate(recs))
    return text, recs, flanks


def _mutated(rng, s, rate):
    out = list(s)
    for p in rng.sample(range(len(s)), max(1, int(round(len(s) * rate)))):
        out[p] = rng.choice([b for b in "ACGT" if b != out[p]])
    return "".join(out)


def ends_reads(seed=79, uniform=None):
    """The read set around the ends -> (reads, {group: (first, last + 1)}).  uniform: every read cut or built to exactly that length
    (the read shorter than k is left out then).  sample_j = flank + record + flank; a read is a stretch of its record's sample.
    Two ends are kept for the stacks, whose counts must be exact; every other group reaches the four OPEN_ENDS, which hold a begin and an
    end of a record, the two sides of the boundary between records 1 and 2 and the two ends of the whole bait.
      over     reads that overhang an end by 5 .. 60 bases, both strands
      far      reads whose overhang is 100 bases and more: beyond E = 1, 16, 64
      n        overhanging reads with an N among the overhanging bases
      tie      two stacks of MIN_DEPTH reads each, one a strand, over TIE_END that differ in the letter TIE_AT columns from the record:
               emission stops there
      depth    MIN_DEPTH reads over DEPTH_END of which one reaches 20 columns and MIN_DEPTH - 1 reach 40: exactly MIN_DEPTH bases on the
               first 20 columns, MIN_DEPTH - 1 on the next 20
      diverged 6 % diverged copies of overhanging reads, which the cut of 30 rejects
      indel    overhanging reads with an insertion or a deletion of 1 .. 4 bases 3 .. 10 bases inside the record's end
      short    one read shorter than any k
      random   random reads"""
    rng = random.Random(seed)
    _, recs, flanks = ends_bait()
    samples = [f[0] + r + f[1] for r, f in zip(recs, flanks)]
    seqs, groups = [], {}
    L = uniform

    def cut(j, lo, n):
        """n bases of sample j from record coordinate lo"""
        return samples[j][150 + lo:150 + lo + n]

    def over(j, side, hang, n, more=0):
        """a read of n (or the uniform length) + more bases of which `hang` lie outside record j at `side`"""
        n = (L or n) + more
        return cut(j, -hang, n) if side == 0 else cut(j, len(recs[j]) - (n - hang), n)

    def group(name, reads):
        groups[name] = (len(seqs), len(seqs) + len(reads))
        seqs.extend(reads)

    group("over", [_strand(rng, over(j, side, rng.randrange(5, 61), rng.randrange(90, 141))) for j, side in OPEN_ENDS for _ in range(20)])
    group("far", [_strand(rng, over(j, side, rng.randrange(100, 131), 180)) for j, side in OPEN_ENDS for _ in range(2)]
          if not L or L > 150 else [])
    ns = []
    for j, side in OPEN_ENDS:
        for _ in range(4):
            hang, n = rng.randrange(10, 41), L or rng.randrange(90, 141)
            r = list(over(j, side, hang, n))
            at = rng.randrange(0, hang) if side == 0 else n - 1 - rng.randrange(0, hang)
            r[at] = "N"
            ns.append(_strand(rng, "".join(r)))
    group("n", ns)
    a = over(*TIE_END, 30, 110)
    at = len(a) - 30 + TIE_AT
    b = a[:at] + ("A" if a[at] != "A" else "C") + a[at + 1:]
    group("tie", [a] * MIN_DEPTH + [revcomp(b)] * MIN_DEPTH)
    group("depth", [over(*DEPTH_END, 20, 100)] + [revcomp(over(*DEPTH_END, 40, 120))] * (MIN_DEPTH - 1))
    diverged = []
    for j, side in OPEN_ENDS:
        for _ in range(4):          # (the copy differs inside the record, where the cut counts)
            r = over(j, side, 25, 120)
            diverged.append(_strand(rng, r[:25] + _mutated(rng, r[25:], 0.06) if side == 0 else _mutated(rng, r[:-25], 0.06) + r[-25:]))
    group("diverged", diverged)
    indel = []
    for j, side in OPEN_ENDS:
        for insert in (True, False):
            for _ in range(5):
                hang, n, g, inside = rng.randrange(12, 31), rng.randrange(100, 141), rng.randrange(1, 5), rng.randrange(3, 11)
                r = over(j, side, hang, n, 0 if insert else g)
                at = hang + inside if side == 0 else len(r) - hang - inside
                r = r[:at] + _rand(rng, g) + r[at:] if insert else r[:at] + r[at + g:]
                # (an insertion is cut off at the end that lies inside the record, so that the overhang stays what it is)
                indel.append(_strand(rng, r[:len(r) - g] if insert and side == 0 else r[g:] if insert else r))
    group("indel", indel)
    group("short", [] if L else [recs[0][:15]])
    group("random", [_rand(rng, L or rng.randrange(60, 160)) for _ in range(20)])
    if L:
        assert all(len(s) == L for s in seqs), sorted({len(s) for s in seqs})
    return seqs, groups


def structured(mf, ext):
    """the oracle's unclamped extension pile int[R, 2, E, 4] as the array the wrapper gives (valid where nothing is clamped)"""
    out = np.zeros(ext.shape[:3], dtype=mf.PILEUP)
    for i, f in enumerate("acgt"):
        out[f] = ext[..., i]
    return out
