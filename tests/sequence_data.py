"""Inputs of the handle-sequence tests (test_sequence_data.py, test_gpu_handle_sequences.py): read sets that stay uploaded on ONE handle
while k-mer sets, thresholds, calls and per-call options change from call to call, the expected bits and hit counts of every (set,
threshold) from the C oracle, and the sequences themselves -- directed ones, each written for one piece of the state a handle carries
from call to call (buffer sets, tally regions, candidate bitmaps, record lists, streams), and seeded random ones.

An op is (set, thr, call, mode, opts):
  set    a name of SETS
  thr    1, 2 or 7
  call   bits      filter_reads
         hits      filter_reads(want_hits=True)
         res2/3/5  filter_resident with that many steps
         passes4   filter_resident_passes with 4 steps
         rbits3    filter_resident_bits with 3 steps: the bits every pass left in its own buffer set, fetched for real
  mode   "S" screened, "E" exhaustive
  opts   "name=value" options in force for that call only

The conditions the sequences rest on -- every expected value passes some reads and not all, any two different expected values differ,
so that a buffer left over from the call before would show, and every expected bitmap has a read r with bit r set and bit r ^ 1 clear, so
that a pass bit moved to the neighbouring read (every count stays right) would show -- are asserted on the CPU by test_sequence_data.py."""
import functools
import os
import random
from collections import namedtuple

import numpy as np

from tests.util_data import bits_to_bool, make_bait, make_protein_bait, make_reads

N_READS, N_GENE = 6000, 600          # reads of a small set; of them, drawn from the protein bait's gene DNA
SEEDS = {"ragged": 901, "uniform": 902}
LAYOUTS = tuple(SEEDS)
SUB_RATE = 0.05          # (at make_reads' 0.01 the uniform set ties: k = 21, 29 and 31 all pass 1647 reads, at every threshold)
THRESHOLDS = (1, 2, 7)
RICH_N, RICH_LEN, RICH_SEED = 120_000, 100, 77          # the bait-rich set: just above adapt_after_call's floor of 100 000 reads
PROT_KP, PROT_CODE = 7, 5

# name -> (k, forced options while the set is built).  Sets of one k expect the same values: the screen's form changes, not the result.
SETS = {"k21": (21, {}), "k29": (29, {}), "k31": (31, {}), "k33": (33, {}), "k41": (41, {}), "k47": (47, {}), "k48": (48, {}), "k63": (63, {}),
        "k31f2": (31, {"front": 2}), "k31f3c": (31, {"front": 3, "canon": 1}), "k31f4": (31, {"front": 4}), "k21f1": (21, {"front": 1}),
        "prot": (PROT_KP, {})}
BUILD_DEFAULTS = {"front": -1, "canon": -1, "front2_log2b": 0, "front3_log2b": -1}
CALLS = ("bits", "hits", "res2", "res3", "res5", "passes4", "rbits3")
STEPS = {"bits": 1, "hits": 1, "res2": 2, "res3": 3, "res5": 5, "passes4": 4, "rbits3": 3}
RETURNS_BITS = ("bits", "hits", "rbits3")          # the calls that hand their own bits back: the others are followed by a recompute
MODES = ("S", "E")
OPTIONS = ((), ("pass=split",), ("pass=serial",), ("s8_finish=1",), ("finish_streams=2",), ("exact_co=1",))
CALL_DEFAULTS = {"pass": "default", "s8_finish": -1, "finish_streams": 0, "exact_co": 0}

Op = namedtuple("Op", "set thr call mode opts")


def op(set_, thr=1, call="bits", mode="S", *opts):
    return Op(set_, thr, call, mode, tuple(opts))


def recompute_of(o):
    """the filter_reads behind a resident call that returns no bits: same set, threshold and mode, no option.  It fetches nothing of what
    the resident call left -- it is one more pass, whose own bits it returns -- and holds the handle's state after the call to the oracle.
    What the passes of a pipelined call themselves wrote is read by rbits3."""
    return Op(o.set, o.thr, "bits", o.mode, ())


def with_recomputes(ops):
    """the sequence as it is run: every resident call that returns no bits followed by its recompute (an op like any other)"""
    out = []
    for o in ops:
        out.append(o)
        if o.call not in RETURNS_BITS:
            out.append(recompute_of(o))
    return out


def moved_bit_shows(bits, n):
    """whether some read r has bit r set and bit r ^ 1 clear: only then does a pass bit that went to the neighbouring read change the bitmap"""
    b = bits_to_bool(bits, n)
    if n % 2:
        b = np.concatenate((b, [False]))
    return bool((b[0::2] != b[1::2]).any())


def show(ops):
    return "; ".join("%s thr%d %s %s%s" % (o.set, o.thr, o.call, o.mode, " " + ",".join(o.opts) if o.opts else "") for o in ops)


def key_of(set_name):
    """what decides a set's expected values: sets of the same key expect the same"""
    return "prot" if set_name == "prot" else "k%d" % SETS[set_name][0]


KEYS = tuple(dict.fromkeys(key_of(s) for s in SETS))


@functools.lru_cache(maxsize=None)
def baits():
    """-> (nucleotide bait FASTA, protein bait FASTA)"""
    return make_bait(), make_protein_bait()[0]


@functools.lru_cache(maxsize=None)
def read_seqs(layout):
    """6 000 reads, ragged or all 150 bases: make_reads' mixed bag from the bait, and among them N_GENE from the DNA of the protein
    bait's genes (so that the protein set passes reads the nucleotide sets do not)"""
    uniform = layout == "uniform"
    seed = SEEDS[layout]
    seqs = make_reads(make_bait(), N_READS - N_GENE, seed=seed, uniform=uniform, sub_rate=SUB_RATE)
    seqs += make_reads(make_protein_bait()[1], N_GENE, seed=seed + 1000, uniform=uniform, mito_frac=0.6, sub_rate=SUB_RATE)
    random.Random(seed + 2000).shuffle(seqs)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def packed(layout):
    from oracle import oracle_lib as ol
    return ol.OracleReads.from_seqs(read_seqs(layout))


@functools.lru_cache(maxsize=None)
def table(key):
    from oracle import oracle_lib as ol
    if key == "prot":
        return ol.OracleTable(baits()[1], PROT_KP, protein=True)
    return ol.OracleTable(baits()[0], int(key[1:]))


Expected = namedtuple("Expected", "bits hits n_pass")


def _expect(key, R, thr, n, threads=4):
    from oracle import oracle_lib as ol
    bits, hits = (ol.pfilter_reads(table(key), R, PROT_CODE, thr, threads=threads) if key == "prot"
                  else ol.filter_reads(table(key), R, thr, threads=threads))
    bits.setflags(write=False)
    hits.setflags(write=False)
    return Expected(bits, hits, int(bits_to_bool(bits, n).sum()))


@functools.lru_cache(maxsize=None)
def expected(layout, key, thr):
    """the oracle's bits, hit counts and passing reads of one (key, threshold) on a small read set; computed once, read-only"""
    return _expect(key, packed(layout), thr, N_READS)


def rich_arrays(host_words, host_npos):
    """the bait-rich set as the oracle reads it, from what Reads.synth(RICH_N, RICH_LEN, RICH_SEED, mito_ppm=1_000_000, keep_host=True) kept"""
    from oracle import oracle_lib as ol
    return ol.OracleReads.from_arrays(host_words, np.arange(RICH_N + 1, dtype=np.uint64) * RICH_LEN, host_npos)


def rich_expected(R, key):
    return _expect(key, R, 1, RICH_N, threads=min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------------------------------------------------------- directed sequences
def directed():
    """name -> ops (without the recomputes).  What each is written for:
    a  a pipelined k = 63 call leaves an exact-kernel tally in the third region of all three buffer sets; k = 31 never writes that region
    b  the same with single passes: the sets alternate, so the third call meets the region the first one wrote
    c  three-set rotation (two-word keys), then two-set rotation, both sides of k = 48 (exact kernel behind finish or not), per-pass tallies
    d  protein and nucleotide passes in turn; hit counts between them
    e  one set through every kind of pass: one-stream with hits, finish, exhaustive, candidate bitmap, and back
    f  record-list geometry: lane records and quad records, canonical and plain keys, the forms of the large-bait screen, thr 1 then thr 2
    g  the pass kind changed by option under one set, single and pipelined calls under each
    In a, c and g a filter_resident_bits call (rbits3) follows a call of ANOTHER set: its first passes write into bitmaps that still hold that
    set's result, and every pass's own bits are compared.  A single pass of a third set follows it: what the log copies left behind."""
    seq = {}
    seq["a"] = [op("k63", 1, "res3")] + [op("k31")] * 3 + [op("k63", 1, "rbits3"), op("k21")]
    seq["b"] = [op("k63"), op("k31"), op("k31")]
    seq["c"] = [op("k48", 1, "res5"), op("k47", 1, "res5"), op("k41", 1, "passes4"), op("k33"), op("k48", 1, "rbits3"), op("k31"), op("k41", 1, "rbits3"), op("k63")]
    seq["d"] = [op("prot"), op("k31"), op("prot", 1, "hits"), op("k21"), op("k31", 2)]
    seq["e"] = [op("k31", 1, "hits"), op("k31"), op("k31", 1, "bits", "E"), op("k31", 2), op("k31"), op("k31", 7, "hits"), op("k31")]
    seq["f"] = [op(s, thr) for s in ("k31f2", "k21", "k31", "k31f3c", "k31f4", "k31f2") for thr in (1, 2)]
    for name, set_, base, other in (("g31", "k31", (), "k41"), ("g21", "k21", ("s8_finish=1",), "k29")):
        seq[name] = [op(set_, 1, call, "S", *(base + extra)) for extra in ((), ("pass=split",), ("pass=serial",), ()) for call in ("bits", "res3")]
        for extra in ((), ("pass=split",), ("pass=serial",)):
            seq[name] += [op(other), op(set_, 1, "rbits3", "S", *(base + extra)), op("k63")]
    return seq


# the bait-rich handle, adaptation on: the feedback turns to the candidate-bitmap pass and back while the set changes under it
RICH_SEQUENCE = [op("k31"), op("k31"), op("k63"), op("k63"), op("k31"), op("k21", 1, "bits", "S", "s8_finish=1"), op("k31"), op("k41", 1, "res3"), op("k31"),
                 op("k63", 1, "rbits3"), op("k41"), op("k31", 1, "rbits3"), op("k21", 1, "bits", "S", "s8_finish=1")]


# ------------------------------------------------------------------------------------------------------------------ random sequences
N_SEEDS = int(os.environ.get("MF_SEQ_SEEDS", "24"))
SEQ_LEN = 16


def random_sequence(seed):
    """SEQ_LEN ops; every odd one takes another set than the op before it (eight changes at the least)"""
    rng = random.Random(31000 + seed)
    names = list(SETS)
    ops = []
    for i in range(SEQ_LEN):
        prev = ops[-1].set if ops else None
        set_ = rng.choice([s for s in names if s != prev] if i % 2 else names)
        ops.append(Op(set_, rng.choice(THRESHOLDS), rng.choice(CALLS), rng.choice(MODES), rng.choice(OPTIONS)))
    return ops


def grid(set_name, thr):
    """every op of one set and threshold"""
    return [Op(set_name, thr, call, mode, opts) for call in CALLS for mode in MODES for opts in OPTIONS]


def finish_pass(o):
    """Whether the op's passes are screen + finish passes on a read set below the adaptation floor (mf_passplan.h, restated): screened,
    threshold 1, no hit counts, not pass=split, and a sample every 16 bases (k >= 28) or pass=serial or s8_finish=1 (the 16.5 kbp bait does
    not turn s8_finish on by itself).  Their n_candidates counts the work items the finish kernels took up, and a finish thread skips
    the records of a read whose pass bit it has seen set -- by whichever thread got there first -- so the figure moves by a few from run to
    run (measured: two fresh handles give 2521 and 2526 for k = 29 on the ragged set).  Such an op is compared on n_pass alone; every
    other op's n_candidates is a function of the op."""
    k = SETS[o.set][0]
    return (o.set != "prot" and o.mode == "S" and o.thr == 1 and o.call != "hits" and "pass=split" not in o.opts
            and (k >= 28 or "pass=serial" in o.opts or "s8_finish=1" in o.opts))


# ------------------------------------------------------------------------------------------------- report calls on one handle
# (tests/test_gpu_handle_sequences.py, second section: the `ends` bait and reads of tests/extend_data.py on one handle)
REPORT_KS = (21, 31, 41)
# units that keep their order: band 30 then band 4 (the insertion span shrinks), E = 4096 then 16 (the extension columns shrink)
REPORT_UNITS = (("assign",), ("depth",), ("place",), ("pileup",), ("verify_keep",), ("align0",), ("align30", "align4"), ("gapped8",),
                ("extend4096", "extend16"), ("extend64_nopile",))
REPORT_ORDERS = {"as_listed": tuple(range(10)), "reversed": tuple(reversed(range(10))), "large_first": (8, 0, 6, 1, 7, 2, 9, 3, 5, 4)}
REPORT_BANDS = {"align0": 0, "align30": 30, "align4": 4, "gapped8": 8, "extend4096": 8, "extend16": 8, "extend64_nopile": 4}


def report_sequence(order):
    """[(op, k)]: the units in that order, every op at another k than the op before it (band 30 needs k > 30)"""
    out = []
    for name in (name for u in order for name in REPORT_UNITS[u]):
        allowed = [k for k in REPORT_KS if k > REPORT_BANDS.get(name, 0) and (not out or k != out[-1][1])]
        out.append((name, allowed[len(out) % len(allowed)]))
    return out


def report_orders():
    orders = dict(REPORT_ORDERS)
    for seed in range(4):
        order = list(range(len(REPORT_UNITS)))
        random.Random(47000 + seed).shuffle(order)
        orders["shuffle%d" % seed] = tuple(order)
    return orders
