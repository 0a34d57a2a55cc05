"""A bait of the size the library is given, built so that the plain-Python oracles stay affordable (tests/test_gpu_report_scale.py,
tests/test_pileup_oracle.py): thousands of short records with runs of tiny and empty ones, record boundaries on the edges the report
kernels tile by (16 positions a thread, 1024 a wave, 4096 a tile), one scaffold record whose gap of N carries the position count beyond
256 tiles, and two neighbouring records behind it.  Seeded, pure Python."""
import random

from tests.report_data import fasta
from tests.util_data import revcomp

TILE, WAVE_SPAN, THREAD_SPAN = 4096, 1024, 16
TINY = (5, 0, 15, 1, 0, 9, 3, 0, 12, 14, 0, 7)          # the lengths the runs of tiny records cycle through


def lengths_for(k):
    """the fixed list the block's record lengths are drawn from"""
    return [0, 1, 5, 15, 16, 17, k - 1, k, k + 1, 64, 150] + list(range(40, 401, 9)) + [400]


def scale_bait(k=31, n_block=2100, front=60000, back=20000, gap_to=255 * TILE + 1000, gap=None, seed=20261019):
    """-> (FASTA text, parts).  The block of n_block short records, the scaffold (front random bases, N up to global position gap_to,
    back random bases), `left`, `right`, and a last run of tiny records.  gap: the length of the gap instead (the small baits).  parts: names, seqs (as
    written), index of the scaffold / left / right, `plain` (block records of 64 bases or more that are random ACGT and nothing else), `tiny_runs` (first index, count), `pads` (index of the record that ends on the edge,
    the edge's modulus), `shared` (pairs of records that share a stretch) and `quiet` (a plain record of 64 positions that scale_reads
    draws no read from)."""
    rng = random.Random(seed)
    rnd = lambda n: "".join(rng.choices("ACGT", k=n))
    lengths = lengths_for(k)
    recs, plain, tiny_runs, pads, shared = [], [], [], [], []
    pos = 0

    def put(name, s):
        nonlocal pos
        recs.append((name, s))
        pos += len(s)

    def tiny_run(n, at):
        tiny_runs.append((len(recs), n))
        for i in range(n):
            put("t%d_%d" % (len(tiny_runs), i), rnd(TINY[(at + i) % len(TINY)]))

    def pad_to(m):
        """a record that ends exactly on a multiple of m, and a plain record behind it, so that the edge is a boundary of two records"""
        n = -pos % m
        n += m if n < 20 else 0
        put("pad%d" % m, rnd(n))
        pads.append((len(recs) - 1, m))
        plain.append(len(recs))
        put("s%d" % len(recs), rnd(150))

    tiny_run(6, 0)                                           # the very front: 5, empty, 15, 1, empty, 9
    pad_at = {n_block // 5: THREAD_SPAN, 2 * n_block // 5: WAVE_SPAN, 3 * n_block // 5: TILE}
    while len(recs) < n_block:
        j = len(recs)
        if j in pad_at:
            pad_to(pad_at[j])
            if pad_at[j] == TILE:
                tiny_run(4, 2)                               # tiny records in the tile's first wave
        elif j % 230 == 115:
            tiny_run(3 + (j // 230) % 4, j // 230)           # the middle: 3 .. 6 in a row
        elif j % 150 == 75:                                  # two records share a stretch, the second holds it reverse-complemented
            a = rnd(220)
            put("s%d" % j, a)
            put("s%d" % (j + 1), rnd(40) + revcomp(a[60:150]) + rnd(50))
            shared.append((j, j + 1))
        elif j % 97 == 50:                                   # invalid and lower-case letters
            a = rnd(200)
            put("s%d" % j, a[:70] + "acgtn" + a[75:120].lower() + "NN" + a[122:160] + "R" + a[161:])
        else:
            n = rng.choice(lengths)
            if n >= 64:
                plain.append(j)
            put("s%d" % j, rnd(n))
    scaffold = len(recs)
    gap = gap_to - (pos + front) if gap is None else gap
    assert gap >= 0
    put("scaffold", rnd(front) + "N" * gap + rnd(back))
    left = len(recs)
    put("left", rnd(600))
    put("right", rnd(600))
    tiny_run(5, 6)                                           # the last records of the bait: 3, empty, 12, 14, empty
    quiet = next((j for j in plain if len(recs[j][1]) == 64), -1)          # a record of 64 positions that scale_reads leaves alone
    parts = {"quiet": quiet, "names": [n for n, _ in recs], "seqs": [s for _, s in recs], "scaffold": scaffold, "front": front, "gap": gap, "back": back,
             "left": left, "right": left + 1, "plain": plain, "tiny_runs": tiny_runs, "pads": pads, "shared": shared}
    return fasta(recs), parts


def _sub(s, rate, rng):
    s = list(s)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = rng.choice([b for b in "ACGT" if b != s[i]])
    return "".join(s)


def scale_reads(parts, k, n, seed, uniform, sub_rate=0.01, read_len=150):
    """n reads in the manner of util_data.make_reads, drawn from every part of the scale bait: the block's records in turn (a read longer
    than its record hangs over both ends, others over one end or none), both flanks of the scaffold and the edges of its gap, `left` and
    `right`; both strands, substitutions, some N, lower case, short and empty reads (ragged only), and random reads that do not pass."""
    rng = random.Random(seed)
    rnd = lambda m: "".join(rng.choices("ACGT", k=m))
    seqs = parts["seqs"]
    sc = seqs[parts["scaffold"]]
    usable = [j for j, s in enumerate(seqs) if len(s) >= k and j not in (parts["scaffold"], parts["quiet"])]
    rng.shuffle(usable)
    gap_lo, gap_hi = parts["front"], parts["front"] + parts["gap"]
    out = []
    for i in range(n):
        L = read_len if uniform else rng.choice([read_len, read_len, rng.randint(0, 40), rng.randint(k, 400), k, k - 1, 0])
        what = i % 10
        if L < k or what == 9:
            s = rnd(L)
        elif what < 6:                                       # a block record, `left` or `right`, in turn
            j = usable[(i // 10 * 5 + what) % len(usable)] if what < 5 else parts["left"] + (i // 10) % 2          # (every tenth: `left` or `right`)
            r = seqs[j].upper()
            ext = rnd(L) + r + rnd(L)
            a = rng.randint(k, L + len(r) - k)               # the record lies at ext[L:L + len(r)]: at least k of its bases
            s = ext[a:a + L]
        else:
            if what == 6:
                a = rng.randrange(0, gap_lo - L)
            elif what == 7:
                a = rng.randrange(gap_hi, len(sc) - L)
            else:                                            # over an edge of the gap or an end of the scaffold
                x = rng.randint(0, L - k)
                a = rng.choice([gap_lo - L + x, gap_hi - x if parts["gap"] else 0, -x, len(sc) - L + x])
            ext = rnd(L) + sc + rnd(L)
            s = ext[L + a:L + a + L]
        if L >= k and what != 9:
            s = _sub(s, sub_rate, rng) if "N" not in s else s
            if rng.random() < 0.5:
                s = revcomp(s)
        if L and rng.random() < 0.08:
            s = list(s)
            for _ in range(rng.randint(1, 3)):
                s[rng.randrange(L)] = rng.choice("NnRK.")
            s = "".join(s)
        if rng.random() < 0.05:
            s = s.lower()
        out.append(s)
    return out


def many_segment_read(g, k, n_seg, seed, long_at, span=None):
    """n_seg segments of k bases from scattered places of g[:span], one of them (long_at) k + 1 long, each on a diagonal of its own, with an
    N between two segments so that no window spans them: n_seg candidates, exactly one with 2 votes (test_gpu_place.scattered_read for
    any number of segments)"""
    rng = random.Random(seed)
    spots = list(range(0, (span or len(g)) - k - 1, 2 * k + 2))
    rng.shuffle(spots)
    segs, diagonals, at = [], set(), 0
    for p in spots:
        if len(segs) == n_seg:
            break
        if p - at in diagonals:
            continue
        diagonals.add(p - at)
        segs.append(g[p:p + k + (len(segs) == long_at)])
        at += len(segs[-1]) + 1
    assert len(segs) == n_seg
    return "N".join(segs)


def bound_carry_read(parts, k, seed, below=63, above=70, wins=False):
    """-> (read, m).  One k-base window of each of `below` plain records in front of plain record m, the first k bases of m one base into
    the read -- a forward candidate on m with start -1 --, and one window of each of `above` plain records behind m, the last of them k + 1
    bases long: below + 1 + above candidates, the 64 smallest of them the `below` and m's, the winner among the rest.  wins: m's segment
    is the one of k + 1 bases instead (two windows, both with start -1), so that the winner is the largest key of the first sweep's map."""
    rng = random.Random(seed)
    plain = sorted(parts["plain"])
    at = len(plain) // 2
    m = plain[at]
    lower, upper = rng.sample(plain[:at], below), rng.sample(plain[at + 1:], above)
    seqs = parts["seqs"]
    pick = lambda j, n: (lambda p: seqs[j][p:p + n])(rng.randrange(0, len(seqs[j]) - n + 1))
    segs = ["N" + seqs[m][:k + wins]] + [pick(j, k) for j in lower + upper[:-1]] + [pick(upper[-1], k + 1 - wins)]
    order = list(range(1, len(segs)))
    rng.shuffle(order)                                       # (the first segment stays first: its place in the read is its start)
    return "N".join([segs[0]] + [segs[i] for i in order]), m


def short_record_bait(n_rec, length, seed, name="r"):
    """n_rec records of `length` random bases each (a few one base longer or shorter): the baits on either side of the counters' LDS limit"""
    rng = random.Random(seed)
    recs = [("%s%d" % (name, j), "".join(rng.choices("ACGT", k=length + (j % 7 == 3) - (j % 11 == 5)))) for j in range(n_rec)]
    return fasta(recs), [s for _, s in recs]


def short_record_reads(seqs, k, n, seed, sub_rate=0.02, lo=None, hi=None):
    """n reads over the records seqs[lo:hi] in turn and at random: the record inside random flanks, cut so that at least k of its bases
    remain; both strands, substitutions (none, few or many a read), and every tenth read random"""
    rng = random.Random(seed)
    rnd = lambda m: "".join(rng.choices("ACGT", k=m))
    idx = list(range(len(seqs)))[lo:hi]
    out = []
    for i in range(n):
        if i % 10 == 9:
            out.append(rnd(rng.randint(k, 90)))
            continue
        r = seqs[idx[i % len(idx)] if i % 2 else rng.choice(idx)]
        L = rng.randint(k + 4, len(r) + 30)
        ext = rnd(L) + r + rnd(L)
        a = rng.randint(k, L + len(r) - k)
        s = _sub(ext[a:a + L], rng.choice([0.0, sub_rate, 4 * sub_rate]), rng)
        out.append(revcomp(s) if rng.random() < 0.5 else s)
    return out
