"""Read baiting for the `bim` loop (SURVEY.md 8f "next" #1).

The reference baits reads by alignment: `bwa_map(threads, fasta_file, basedir, prefix, fastq1,
fastq2, quality=30) -> (bam, fq1, fq2)` runs `bwa index; bwa mem | samtools view -q 30 |
samtools fastq` (bim/bim.py:43-58), and the loop in MitoFlex.py:346-375 hands the BAM to
`cal_insert(bam, basedir, prefix)` (bim/bim.py:65-78: `samtools stats | grep ^IS`, count-weighted mean
of the insert sizes) when `--insert-size-auto` is on, feeds the survivors to `assemble()` and uses the new
contigs as the next bait.

`kmer_bait_map` and `cal_insert` here have the same signatures and return shapes, so the loop runs
unchanged with `from mitoflex_amd.bim.bim import kmer_bait_map as bwa_map, cal_insert`:

* `kmer_bait_map` baits with the GPU k-mer filter -- the bait FASTA of every generation is turned into a
  canonical-k-mer set on the device and the reads are screened against it -- and puts, where the BAM path
  was, the path of a samtools-stats-shaped text file `<prefix>.bait.stats` whose `IS` lines hold an
  insert-size histogram of the kept pairs;
* `cal_insert` reads that file exactly the way the reference reads `samtools stats` (`^IS`, first two
  columns, count-weighted mean) and tees it to `<prefix>.stats` like the reference does.

The histogram comes from k-mer anchors, not alignments: for a kept pair whose mates each hold a bait
k-mer on opposite strands of the same bait record, the first such k-mer of each mate fixes where the
mate starts on the bait, and the outer distance is the insert size (what samtools calls TLEN for an
inward pair).  A sample of the first kept pairs is enough for a mean.

Parity with bwa/samtools is UNPINNED (un-vendored external tools, no reference test pins them): the two
select different read sets by design and the insert size is an estimate from exact k-mer anchors.
What can be stated is measured by tests/test_gpu_parity.py::test_bim_bait_sensitivity (reads drawn from
the bait with 1 % substitutions: > 99 % of pairs kept, no background pair) and by tests/test_bim.py
(insert-size estimate within a base or two of the truth on simulated pairs; a three-generation loop
with a stand-in assembler whose kept sets equal the oracle's and grow).
"""
from __future__ import annotations

import tempfile
from os import path
from typing import Dict, Iterator, List, Optional, Tuple

INSERT_SAMPLE_PAIRS = 20000        # kept pairs looked at for the insert-size histogram
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def _bait_records(fasta_file: str) -> List[str]:
    recs: List[List[str]] = []
    with open(fasta_file) as f:
        for line in f:
            if line.startswith(">"):
                recs.append([])
            elif recs:
                recs[-1].append("".join(line.split()).upper())
    return ["".join(r) for r in recs]


def _anchor_index(records: List[str], k: int) -> Dict[str, Tuple[int, int]]:
    """forward k-mer text -> (record, position); k-mers that occur twice are left out (ambiguous anchors)."""
    seen: Dict[str, Optional[Tuple[int, int]]] = {}
    for ri, rec in enumerate(records):
        for p in range(len(rec) - k + 1):
            w = rec[p:p + k]
            if w.strip("ACGT"):
                continue
            seen[w] = None if w in seen else (ri, p)
    return {w: v for w, v in seen.items() if v is not None}


def _first_anchor(seq: str, k: int, idx: Dict[str, Tuple[int, int]]):
    """(record, start of the read on the bait's forward strand, strand) from the first k-mer of the read that is a
    unique bait k-mer on either strand; None if there is none."""
    s = seq.upper()
    rc = s.translate(_COMP)[::-1]
    L = len(s)
    for o in range(L - k + 1):
        hit = idx.get(s[o:o + k])
        if hit is not None:                          # read lies forward: its first base sits at p - o
            return hit[0], hit[1] - o, +1
        hit = idx.get(rc[L - k - o:L - o])           # the same window on the other strand
        if hit is not None:                          # read lies reversed: the window's bait start is hit[1], the read's last base
            return hit[0], hit[1] - (L - k - o), -1  # maps to hit[1] - (bases of the read behind the window)
    return None


def _fastq_seqs(fq: str) -> Iterator[str]:
    with open(fq) as f:
        for i, line in enumerate(f):
            if i % 4 == 1:
                yield line.rstrip("\r\n")


def estimate_insert_sizes(fasta_file: str, fq1: str, fq2: str, kmer: int = 31, max_pairs: int = INSERT_SAMPLE_PAIRS) -> Dict[int, int]:
    """Insert-size histogram {size: pairs} of up to `max_pairs` pairs of (fq1, fq2) from exact k-mer anchors on the bait."""
    idx = _anchor_index(_bait_records(fasta_file), kmer)
    hist: Dict[int, int] = {}
    for n, (s1, s2) in enumerate(zip(_fastq_seqs(fq1), _fastq_seqs(fq2))):
        if n >= max_pairs:
            break
        a1, a2 = _first_anchor(s1, kmer, idx), _first_anchor(s2, kmer, idx)
        if a1 is None or a2 is None or a1[0] != a2[0] or a1[2] == a2[2]:
            continue
        fwd, rev, rev_len = (a1, a2, len(s2)) if a1[2] > 0 else (a2, a1, len(s1))
        size = rev[1] + rev_len - fwd[1]             # forward mate's first base .. reversed mate's last base on the bait
        if 0 < size <= 100000:
            hist[size] = hist.get(size, 0) + 1
    return hist


def pair_insert_sizes_device(fasta_file: str, fq1: str, fq2: str, kmer: int = 31, max_pairs: Optional[int] = None):
    """Insert size of every pair of (fq1, fq2), int64, -1 where there is none: the two files are loaded onto the device, every mate is
    placed on the bait by the votes of all its anchor k-mers (mitofilter.place_reads, one call per mate) and mitofilter.pair_inserts
    joins the mates.  max_pairs: only the first so many pairs (default: all)."""
    import numpy as np
    from mitoflex_amd import mitofilter as mf
    ks = mf.KmerSet.from_fasta(fasta_file, kmer, 0)
    try:
        places = []
        for fq in (fq1, fq2):
            reads = mf.Reads.from_fastq(fq, 0)
            try:
                places.append(mf.place_reads(ks, reads, 1)[1] if reads.info.n_reads else np.zeros(0, dtype=mf.PLACE))
            finally:
                reads.close()
    finally:
        ks.close()
    n = min(len(places[0]), len(places[1]))
    if max_pairs is not None:
        n = min(n, max_pairs)
    return mf.pair_inserts(places[0][:n], places[1][:n])


def estimate_insert_sizes_device(fasta_file: str, fq1: str, fq2: str, kmer: int = 31, max_pairs: Optional[int] = None) -> Dict[int, int]:
    """estimate_insert_sizes on the device: the same histogram {size: pairs}, from every pair (by default) and from all anchor
    k-mers of a mate instead of its first."""
    import numpy as np
    sizes = pair_insert_sizes_device(fasta_file, fq1, fq2, kmer, max_pairs)
    values, counts = np.unique(sizes[sizes > 0], return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


def kmer_bait_map(threads: int, fasta_file: str, basedir: str, prefix: str,
                  fastq1: str, fastq2: Optional[str], quality: int = 30,
                  kmer: int = 31, threshold: int = 1, devices: int = 1, anchors: str = "host",
                  max_permille: Optional[int] = None, keep: Optional[int] = None, band: Optional[int] = None,
                  gapped: bool = False, extend: int = 0) -> Tuple[str, str, Optional[str]]:
    """Drop-in for `bwa_map`: returns (stats, fq1, fq2).  `stats` stands where the BAM path was and is what `cal_insert`
    takes; `threads` and `quality` are accepted for signature compatibility and ignored.  anchors: "host" estimates the insert
    sizes in Python from the first anchor of each mate of a sample of the kept pairs; "device" places every kept mate on the GPU
    (estimate_insert_sizes_device).
    keep: when given (mitofilter.KEEP_ACCEPTED or KEEP_PLACED; KEEP_PASSING writes what the default does), the bait step is a
    verifying one (mitofilter.filter_fastq_files_verified): every passing mate is placed and scored against the bait, cut at
    max_permille mismatches per thousand compared bases (1000 when not given), and a mate the keep rule drops loses its vote in the
    pair rule -- the reads of a diverged copy (a NUMT, a contaminant) do not reach the assembler or the next generation's bait.
    band: when given with keep (0 .. 31, below kmer), the placed mates are aligned inside that band before the cut
    (mitofilter.filter_fastq_files_aligned): a mate with a true indel against the bait costs its indel's bases, not the mismatches
    behind it, and is kept under a tight cut.  None keeps today's calls.
    gapped: with band, the aligning call is the gapped one (mitofilter.filter_fastq_files_aligned(gapped=True)); the files it writes are
    the same.  Without band it is a ValueError.
    extend: with band, the aligning call is the extending one (mitofilter.filter_fastq_files_aligned(extend=E)); the files it writes are
    the same.  Without band it is a ValueError."""
    from mitoflex_amd import mitofilter as mf
    if gapped and band is None:
        raise ValueError("gapped needs a band: the gapped consensus comes from the banded alignment")
    _check_extend(extend, band)
    if anchors not in ("host", "device"):
        raise ValueError('anchors is "host" or "device"')
    if max_permille is not None and not 0 <= int(max_permille) <= 1000:
        raise ValueError("max_permille is a number from 0 to 1000")
    _check_band(band, kmer)
    if band is not None and keep is None:
        raise ValueError("band needs a keep mode: without one no mate is placed")
    fq1 = path.join(basedir, prefix + ".1.fq")
    fq2 = path.join(basedir, prefix + ".2.fq") if fastq2 is not None else None
    ks = mf.KmerSet.from_fasta(fasta_file, kmer, 0)          # the device-side set builder, once per generation
    try:
        if keep is None:
            mf.filter_fastq_files(ks, fastq1, fastq2, fq1, fq2, threshold, mf.PAIR_EITHER, devices)
        elif band is None:
            mf.filter_fastq_files_verified(ks, fastq1, fastq2, fq1, fq2, threshold, mf.PAIR_EITHER, n_devices=devices, pileup=False,
                                           max_permille=1000 if max_permille is None else int(max_permille), keep=keep)
        else:
            mf.filter_fastq_files_aligned(ks, fastq1, fastq2, fq1, fq2, int(band), threshold, mf.PAIR_EITHER, n_devices=devices, pileup=False,
                                          max_permille=1000 if max_permille is None else int(max_permille), keep=keep, extend=int(extend), gapped=bool(gapped))
    finally:
        ks.close()
    stats = path.join(basedir, prefix + ".bait.stats")
    estimate = estimate_insert_sizes_device if anchors == "device" else estimate_insert_sizes
    hist = estimate(fasta_file, fq1, fq2, kmer) if fq2 is not None else {}
    with open(stats, "w") as f:
        f.write("# insert sizes of kept pairs from k-mer anchors on the bait (mitoflex_amd.bim); samtools-stats IS layout\n")
        for size in sorted(hist):
            f.write(f"IS\t{size}\t{hist[size]}\t{hist[size]}\t0\t0\n")
    return stats, fq1, fq2


def _check_band(band: Optional[int], kmer: int):
    if band is not None and not 0 <= int(band) <= min(31, kmer - 1):
        raise ValueError("band is a number from 0 to 31 and below kmer")


def _check_extend(extend: int, band: Optional[int]):
    if not 0 <= int(extend) <= 4096:
        raise ValueError("extend is a number from 0 to 4096")
    if int(extend) and band is None:
        raise ValueError("extend needs a band: the overhanging bases get their columns from the banded alignment")


def rescue_window(sizes, lo: float = 0.01, hi: float = 0.99) -> Tuple[int, int]:
    """The insert window (min_insert, max_insert) for mitofilter.place_pairs from the inserts of the pairs the vote placed (`sizes`: what
    place_pairs(rescue=False).pairs["insert"] or mitofilter.pair_inserts gives; values <= 0 are no insert): their `lo` and `hi`
    quantiles, and where that is wider than mitofilter.RESCUE_MAX inserts, the RESCUE_MAX inserts around the median.  ValueError when
    no pair has an insert."""
    import numpy as np
    from mitoflex_amd import mitofilter as mf
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError("the quantiles are 0 <= lo <= hi <= 1")
    v = np.asarray(sizes, dtype=np.int64)
    v = np.sort(v[v > 0])
    if v.size == 0:
        raise ValueError("no pair has an insert: the window cannot be estimated")
    a, b = int(v[int(lo * (v.size - 1))]), int(v[int(hi * (v.size - 1))])
    if b - a + 1 > mf.RESCUE_MAX:
        median = int(v[(v.size - 1) // 2])
        a = max(1, median - mf.RESCUE_MAX // 2)
        b = a + mf.RESCUE_MAX - 1
    return a, b


def consensus_bait(fasta_file: str, fq1: str, fq2: Optional[str], out_fasta: str, kmer: int = 31, min_depth: int = 3,
                   max_permille: Optional[int] = None, band: Optional[int] = None, gapped: bool = False,
                   extend: int = 0, pairs: bool = False, min_insert: Optional[int] = None, max_insert: Optional[int] = None,
                   rescue_permille: int = 100):
    """A polished bait for the next generation: the reads of (fq1, fq2) -- the kept reads of a bait step -- are placed on the bait
    `fasta_file` and piled up on the device (mitofilter.filter_fastq_files_pileup), and the consensus is written to `out_fasta` under the
    bait's record names: the reads' letter where at least `min_depth` bases agree on one, N where the most is tied, the bait's own
    letter in lower case elsewhere.  Returns the record summaries (mitofilter.PILEUP_RECORD: bases, matches, mismatches, called,
    ambiguous, variants).
    max_permille: when given (0 .. 1000), every placed read is first scored against the bait along its placement and piled only when
    its mismatches are at most that many per thousand compared bases (mitofilter.filter_fastq_files_verified): reads of a diverged
    copy -- a NUMT, a paralogue, a contaminant -- then stay out of the polished bait.  None: no read is scored.
    band: when given (0 .. 31, below kmer), every placed read is aligned inside that band first (mitofilter.filter_fastq_files_aligned;
    the cut is max_permille edits per thousand alignment columns, 1000 when not given) and its bases pile where the alignment puts
    them: the bases behind an indel no longer pile up as false mismatches.  The consensus still calls substitutions only.  None keeps
    today's calls.
    gapped: with band, the GAPPED consensus is written instead (include/mitofilter.h, gapped consensus): a position that more than half
    of its covering reads delete is left out, the bases that more than half of them insert behind a position are written behind it, and
    the polished bait has the sample's length and coordinates.  Without band it is a ValueError.
    extend: with band (band 0 too), the EXTENDED records are written instead (include/mitofilter.h, extended records): every record's
    gapped consensus between the columns that the reads overhanging its ends agree on, up to `extend` (at most 4096) a side, so that the
    next generation's bait reaches reads the old ends shared no k-mer with.  Without band it is a ValueError.
    pairs: the two files are loaded into memory (mitofilter.Reads.from_fastq) and placed as PAIRS (mitofilter.place_pairs; include/
    mitofilter.h, pairs): a mate the vote cannot place -- in a diverged stretch, a repeat, a stretch two records share -- is looked for
    in the window [min_insert, max_insert] its placed mate implies and piled where it fits at no more than `rescue_permille`
    mismatches per thousand compared bases (100, one base in ten: a policy choice, not a measured value).  The window comes from a
    first pass without rescue (rescue_window) when it is not given.  With band, gapped, extend or without fq2 it is a ValueError."""
    from mitoflex_amd import mitofilter as mf
    if gapped and band is None:
        raise ValueError("gapped needs a band: the gapped consensus comes from the banded alignment")
    _check_extend(extend, band)
    if pairs and (band is not None or gapped or int(extend) or fq2 is None):
        raise ValueError("pairs takes two files and neither band, gapped nor extend: a rescued mate lies on its diagonal (consensus_bait_pairs aligns it)")
    if not pairs and (min_insert is not None or max_insert is not None):
        raise ValueError("min_insert and max_insert belong to pairs=True")
    if (min_insert is None) != (max_insert is None):
        raise ValueError("min_insert and max_insert are given together")
    if not 0 <= int(rescue_permille) <= 1000:
        raise ValueError("rescue_permille is a number from 0 to 1000")
    if min_depth < 1:
        raise ValueError("min_depth is at least 1")
    if max_permille is not None and not 0 <= int(max_permille) <= 1000:
        raise ValueError("max_permille is a number from 0 to 1000")
    _check_band(band, kmer)
    if kmer < 1:
        raise ValueError("kmer is at least 1")
    if path.abspath(out_fasta) == path.abspath(fasta_file):
        raise ValueError("out_fasta would overwrite the bait")
    ks = mf.KmerSet.from_fasta(fasta_file, kmer, 0)
    try:
        names, starts = ks.record_names, ks.record_starts
        with tempfile.TemporaryDirectory(prefix="consensus_bait_") as tmp:          # (the call writes its kept reads; they are not wanted)
            out1, out2 = path.join(tmp, "k.1.fq"), path.join(tmp, "k.2.fq") if fq2 is not None else None
            if pairs:
                consensus, records = _consensus_of_pairs(mf, ks, fq1, fq2, min_depth, 1000 if max_permille is None else int(max_permille), min_insert,
                                                         max_insert, int(rescue_permille))
            elif band is not None:
                v = mf.filter_fastq_files_aligned(ks, fq1, fq2, out1, out2, int(band), 1, mf.PAIR_EITHER, min_depth=min_depth,
                                                  max_permille=1000 if max_permille is None else int(max_permille), extend=int(extend), gapped=bool(gapped))
                consensus, records = v.consensus, v.pileup_records
                if gapped:
                    consensus, starts = v.gapped, v.gapped_starts
                if int(extend):
                    consensus, starts = v.extended, v.extended_starts
            elif max_permille is None:
                _, _, _, consensus, records, _ = mf.filter_fastq_files_pileup(ks, fq1, fq2, out1, out2, 1, mf.PAIR_EITHER, min_depth=min_depth)
            else:
                v = mf.filter_fastq_files_verified(ks, fq1, fq2, out1, out2, 1, mf.PAIR_EITHER, min_depth=min_depth, max_permille=int(max_permille))
                consensus, records = v.consensus, v.pileup_records
    finally:
        ks.close()
    with open(out_fasta, "w") as f:
        f.write(mf.consensus_fasta(names, starts, consensus))
    return records


def consensus_bait_pairs(fasta_file: str, fq1: str, fq2: str, out_fasta: str, kmer: int = 31, min_depth: int = 1,
                         max_permille: Optional[int] = None, band: int = 8, gapped: bool = True, extend: int = 0,
                         min_insert: Optional[int] = None, max_insert: Optional[int] = None, rescue_permille: int = 100):
    """consensus_bait(pairs=True) with a band: the two files are loaded into memory and aligned as PAIRS (mitofilter.align_pairs; include/
    mitofilter.h, pairs with a band).  Both mate sets are aligned inside `band`; a mate the vote cannot place is looked for in the window
    [min_insert, max_insert] its settled mate implies -- the candidates are scored ungapped, at no more than `rescue_permille` mismatches
    per thousand compared bases -- and is then aligned around the candidate that won, so the polished bait has the rescued mates over a
    diverged stretch AND the indels and the ends the banded alignment calls there.  The seed is ungapped: a mate with an indel well inside
    it is found only with a looser rescue_permille (100 is a policy choice, not a measured value).  The window comes from a first call
    without rescue (rescue_window) when it is not given.
    Written to out_fasta under the bait's record names: the extended records when `extend` is given, otherwise the gapped consensus when
    `gapped` is set, otherwise the consensus.  Returns the pile-up's record summaries."""
    from mitoflex_amd import mitofilter as mf
    if fq2 is None:
        raise ValueError("consensus_bait_pairs takes two files")
    if (min_insert is None) != (max_insert is None):
        raise ValueError("min_insert and max_insert are given together")
    if min_insert is not None and (not 1 <= int(min_insert) <= int(max_insert) < 2 ** 31 or int(max_insert) - int(min_insert) + 1 > mf.RESCUE_MAX):
        raise ValueError("the insert window is 1 <= min_insert <= max_insert, at most %d inserts wide" % mf.RESCUE_MAX)
    if not 0 <= int(rescue_permille) <= 1000:
        raise ValueError("rescue_permille is a number from 0 to 1000")
    if min_depth < 1:
        raise ValueError("min_depth is at least 1")
    if max_permille is not None and not 0 <= int(max_permille) <= 1000:
        raise ValueError("max_permille is a number from 0 to 1000")
    if kmer < 1:
        raise ValueError("kmer is at least 1")
    if band is None:
        raise ValueError("band is a number from 0 to 31 and below kmer")
    _check_band(band, kmer)
    _check_extend(extend, band)
    if path.abspath(out_fasta) == path.abspath(fasta_file):
        raise ValueError("out_fasta would overwrite the bait")
    cut = 1000 if max_permille is None else int(max_permille)
    ks = mf.KmerSet.from_fasta(fasta_file, kmer, 0)
    try:
        names, starts = ks.record_names, ks.record_starts
        r1 = mf.Reads.from_fastq(fq1, 0)
        try:
            r2 = mf.Reads.from_fastq(fq2, 0)
            try:
                if min_insert is None:
                    first = mf.align_pairs(ks, r1, r2, 1, mf.RESCUE_MAX, int(band), rescue=False, min_depth=min_depth, max_permille=cut, pileup=False)
                    min_insert, max_insert = rescue_window(first.pairs["insert"])
                p = mf.align_pairs(ks, r1, r2, int(min_insert), int(max_insert), int(band), rescue=True, rescue_permille=int(rescue_permille),
                                   min_depth=min_depth, max_permille=cut, gapped=bool(gapped), extend=int(extend))
            finally:
                r2.close()
        finally:
            r1.close()
    finally:
        ks.close()
    consensus, records = p.consensus, p.pileup_records
    if gapped:
        consensus, starts = p.gapped, p.gapped_starts
    if int(extend):
        consensus, starts = p.extended, p.extended_starts
    with open(out_fasta, "w") as f:
        f.write(mf.consensus_fasta(names, starts, consensus))
    return records


def _consensus_of_pairs(mf, ks, fq1, fq2, min_depth, max_permille, min_insert, max_insert, rescue_permille):
    """consensus and pile-up records of the two files placed as pairs; the window estimated from the vote-placed pairs when not given"""
    r1 = mf.Reads.from_fastq(fq1, 0)
    try:
        r2 = mf.Reads.from_fastq(fq2, 0)
        try:
            if min_insert is None:
                first = mf.place_pairs(ks, r1, r2, 1, mf.RESCUE_MAX, rescue=False, min_depth=min_depth, max_permille=max_permille, pileup=False)
                min_insert, max_insert = rescue_window(first.pairs["insert"])
            p = mf.place_pairs(ks, r1, r2, int(min_insert), int(max_insert), rescue=True, rescue_permille=rescue_permille, min_depth=min_depth,
                               max_permille=max_permille)
            return p.consensus, p.pileup_records
        finally:
            r2.close()
    finally:
        r1.close()


def cal_insert(bam: str, basedir: str, prefix: str) -> float:
    """Mirror of bim/bim.py:65-78 over the stats file `kmer_bait_map` returned in the BAM's place: `^IS` lines, first two
    columns, count-weighted mean; the text is teed to `<prefix>.stats`.  Like the reference it fails (ZeroDivisionError)
    when there is no insert-size line at all."""
    stat_file = path.join(basedir, prefix + ".stats")
    text = open(bam).read()
    with open(stat_file, "w") as f:
        f.write(text)
    stats = [[int(y) for y in x.split("\t")[1:]][:2] for x in text.split("\n") if x.startswith("IS")]
    avg_ins = sum(a * b for a, b in stats) / sum(b for _, b in stats)
    return avg_ins
