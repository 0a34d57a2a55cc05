"""The generator of the report fuzz (tests/test_gpu_report_fuzz.py): config(seed) draws one bait, two mate sets of reads and one value of
every parameter of the report calls (assignment, depth, placement, pile-up, verification and the keep rule, banded alignment, gapped
consensus, extension, pairs with rescue).  It is pure Python and calls neither the device nor an oracle; expected(c) is the one place
where the oracles of a configuration are run, shared by the GPU test and by tests/test_report_fuzz_data.py, which holds the generator to
what it is meant to reach.

What is scheduled by the seed, so that a run of consecutive seeds covers it by construction: k (K_LIST[seed % 20]), the bait's number
of positions (seed % 8: 4096, 4097, 4095 -- the placement kernels' tile and its neighbours --, twice more than 8192, else free), one
read length for the whole set (seed % 3 == 0) and the one read of 5000 to 9000 bases (seed % 4 == 1 where the set is ragged).
Everything else is drawn from random.Random(19000 + seed); where every read has one length, the threshold is drawn from the values that
a read of that length can reach.

Junk (IUPAC codes, lower case, N, '-'; the alphabet of tests/test_gpu_fuzz.py) falls at a rate of 0 or 0.1 on the short records and the
padding; the two long records that the reads are drawn from take it at one letter in 250, at arbitrary offsets, so that at k = 63 they
still hold windows without an invalid base (up to k = 21 the second of them takes invalid letters at the full rate in half of those seeds)."""
import os
import random

K_LIST = [11, 12, 15, 16, 17, 20, 21, 27, 28, 31, 32, 33, 34, 40, 47, 48, 49, 55, 62, 63]
N_SEEDS = int(os.environ.get("MF_FUZZ_SEEDS", "24"))
JUNK = "ACGT" * 12 + "NRYacgtn-"
SPARSE_JUNK = "NRYn-acgt"
EXTEND_MAX = 4096
RESCUE_MAX = 4096
PS_TILE = 4096
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
PARAMS = ("thr", "mode", "min_depth", "max_permille", "band", "keep", "extend", "rescue_permille", "min_insert", "max_insert", "group")


def revcomp(s):
    return s[::-1].translate(_COMP)


def _dna(rng, n, junk=0.0):
    return "".join(rng.choices(JUNK if junk else "ACGT", k=n))


def _substituted(rng, s, rate):
    t = list(s)
    for i, c in enumerate(t):
        if rng.random() < rate:
            t[i] = rng.choice([b for b in "ACGT" if b != c.upper()])
    return "".join(t)


def _piece(rng, rec, lo, hi):
    """the record's letters at [lo, hi), random letters where that lies outside the record"""
    return "".join(rec[c] if 0 <= c < len(rec) else rng.choice("ACGT") for c in range(lo, hi))


# ------------------------------------------------------------------ bait
def _bait(rng, k, seed):
    """-> (records [(name, letters)], what: the features drawn, and where the reads find them)"""
    target = {0: PS_TILE, 1: PS_TILE + 1, 2: PS_TILE - 1}.get(seed % 8)
    budget = target or (rng.randint(8300, 11800) if seed % 8 in (3, 4) else rng.randint(3400, 8000))
    junk = rng.choice([0.0, 0.1])
    draw = {f: rng.random() < p for f, p in (("anonymous", 0.4), ("repeat", 0.6), ("shared", 0.6), ("homopolymer", 0.3), ("ac_repeat", 0.3),
                                             ("palindrome", 0.5), ("adjacent", 0.6))}
    draw["palindrome"] &= k % 2 == 0
    len_a = 4000 if budget >= 8300 or (budget >= 6500 and rng.random() < 0.5) else 1500
    len_b = rng.choice([200, 600, 1500])
    a, b = list(_dna(rng, len_a)), list(_dna(rng, len_b))
    what = dict(draw, junk=junk, stretches=[])
    if draw["repeat"]:                                   # a stretch repeated inside one record
        s = rng.randint(k + 10, 150)
        p = rng.randrange(0, len_a // 2 - s)
        q = rng.randrange(len_a // 2, len_a - s)
        a[q:q + s] = a[p:p + s]
        what["stretches"].append(("a", p, s))
    if draw["palindrome"]:                               # a window that is its own reverse complement
        h = _dna(rng, k // 2)
        p = rng.randrange(0, len_a - k)
        a[p:p + k] = h + revcomp(h)
    a, b = "".join(a), "".join(b)
    small = [0, 5, k - 1, k, k + 1, 16, 64]
    shorts = [_dna(rng, rng.choice(small), rng.choice([0.0, junk])) for _ in range(rng.randint(0, 2))]
    mid, shared = [], None
    if draw["homopolymer"]:
        mid.append("T" * rng.randint(k, 90))
    if draw["ac_repeat"]:
        mid.append("AC" * rng.randint(k, k + 30))
    if draw["shared"]:                                   # a stretch shared by two records, once as it is and once reverse-complemented
        s, t = rng.randint(k + 5, 120), rng.randint(k + 5, 120)
        p, q = rng.randrange(0, len_a - s), rng.randrange(0, len_b - t)
        shared = _dna(rng, 40) + a[p:p + s] + _dna(rng, 30) + revcomp(b[q:q + t]) + _dna(rng, 40)
        mid.insert(0, shared)
        shared_stretches = [("a", p, s), ("b", q, t)]
    if junk:                                             # after the copies: the shared record keeps the letters the long ones lose
        a, b = _sprinkled(rng, a), _sprinkled(rng, b)
        if k <= 21 and rng.random() < 0.5:               # (a window of 21 bases is free of it once in seven: reads of b still pass)
            b = "".join(rng.choice("NRY-") if rng.random() < 0.09 else c for c in b)
    lead = [_dna(rng, rng.choice([5, k - 1, 16, 64]), rng.choice([0.0, junk]))] if draw["anonymous"] else []
    between = [] if draw["adjacent"] else [_dna(rng, rng.choice(small), 0.0)]
    seqs = lead + shorts[:1] + [a] + between + [b] + shorts[1:]
    for m in mid:
        if len(seqs) < 6:
            seqs.append(m)
    left = budget - sum(len(s) for s in seqs)
    while left < 0:                                      # (the records after the two long ones give way to the total)
        left += len(seqs.pop())
    if shared in seqs:
        what["stretches"] += shared_stretches
    what["shared"] = shared in seqs
    if left:
        seqs.append(_dna(rng, left, rng.choice([0.0, junk])))
    ia = seqs.index(a)
    what.update(a=ia, b=seqs.index(b, ia + 1), total=sum(len(s) for s in seqs))
    names = [""] * len(lead) + ["%s_%d_%s" % (rng.choice(("ga", "gb", "gc")), i, rng.choice("xy")) for i in range(len(seqs) - len(lead))]
    return list(zip(names, seqs)), what


def _sprinkled(rng, s):
    t = list(s)
    for _ in range(max(len(t) // 250, 1)):
        t[rng.randrange(len(t))] = rng.choice(SPARSE_JUNK)
    return "".join(t)


def fasta(records):
    out = []
    for i, (name, s) in enumerate(records):
        if name or i:
            out.append(">%s drawn\n" % name)
        out.extend(s[j:j + 70] + "\n" for j in range(0, len(s), 70))
    return "".join(out)


# ------------------------------------------------------------------ reads
class _Reads:
    """one mate set's reads as (kind, letters, origin); origin is (record, strand, lo, hi) in record coordinates, or None"""

    def __init__(self, rng, k, recs, what, uniform):
        self.rng, self.k, self.recs, self.what, self.uniform = rng, k, recs, what, uniform
        self.longs = [what["a"], what["b"]]
        self.out = []

    def length(self, at_least=0, at_most=1200):
        if self.uniform:
            return self.uniform
        rng, k = self.rng, self.k
        L = rng.choice([0, 1, k - 1, k, k + 1, 63, 64, 65, 100, 150, 151, rng.randint(k, 300), rng.randint(2 * k, 300), rng.randint(2 * k, 300),
                        rng.randint(300, 1200)])
        return min(max(L, at_least), at_most)

    def add(self, kind, s, origin=None):
        if origin is not None and origin[1]:
            s = revcomp(s)
        if self.uniform:
            assert len(s) == self.uniform, (kind, len(s))
        self.out.append((kind, s, origin))

    def slice(self, kind="slice", rate=0.01, at_least=0):
        rng = self.rng
        j = rng.choice(self.longs + [self.what["a"]])
        rec = self.recs[j]
        L = self.length(at_least)
        lo = rng.randrange(0, max(len(rec) - L, 0) + 1)
        s = _substituted(rng, rec[lo:lo + L], rate)
        if len(s) < L:                                   # longer than the record: it hangs over its end
            s += _dna(rng, L - len(s))
        self.add(kind, s, (j, rng.randrange(2), lo, lo + L))
        return s

    def overhang(self):
        """a random flank over the record's begin, its end, or both (a read longer than a short record)"""
        rng, k = self.rng, self.k
        fits = [j for j, r in enumerate(self.recs) if len(r) >= k]
        j = rng.choice(fits + self.longs * 2)
        rec, L = self.recs[j], self.length(k + 2)
        side = rng.choice(("begin", "end", "both"))
        if side == "both":
            if not self.uniform:
                L = min(len(rec) + rng.randint(2, 60), 1200)
            if L < len(rec) + 2:
                side = "begin"
            else:
                lo = -rng.randint(1, L - len(rec) - 1)
        if side == "begin":
            lo = -rng.randint(1, max(min(L - k, 60), 1))
        elif side == "end":
            lo = len(rec) - L + rng.randint(1, max(min(L - k, 60), 1))
        self.add("overhang", _substituted(rng, _piece(rng, rec, lo, lo + L), 0.01), (j, rng.randrange(2), lo, lo + L))

    def junction(self):
        rng = self.rng
        left, right = self.recs[self.what["a"]], self.recs[self.what["b"]]
        L = self.length(2 * self.k, len(right) + self.k)
        n = rng.randint(1, L - 1)
        s = left[-n:] + right[:L - n]
        self.add("junction", s + _dna(rng, L - len(s)), (self.what["a"], rng.randrange(2), len(left) - n, len(left) - n + L))

    def indel(self):
        """one to three indels of 1 to 6 bases, at least k bases from either end"""
        rng, k = self.rng, self.k
        L = self.length(2 * k + 8, 600)
        if L < 2 * k + 2:
            return self.slice()
        j = rng.choice(self.longs)
        rec = self.recs[j]
        lo = rng.randrange(0, max(len(rec) - L - 20, 1))
        s = list(_piece(rng, rec, lo, lo + L + 20))
        for at in sorted((rng.randint(k, L - k) for _ in range(rng.randint(1, 3))), reverse=True):
            n = rng.randint(1, 6)
            if rng.random() < 0.5:
                s[at:at] = _dna(rng, n)
            elif at + n <= L - k:
                del s[at:at + n]
        self.add("indel", "".join(s[:L]), (j, rng.randrange(2), lo, lo + L))

    def junky(self):
        """a slice with an N, IUPAC codes or lower-case letters inside"""
        at = len(self.out)
        s = list(self.slice("junky", at_least=self.k + 4))
        kind, _, origin = self.out.pop(at)
        for _ in range(self.rng.randint(1, 3)):
            s[self.rng.randrange(len(s))] = self.rng.choice("NNRYKn-acgt")
        self.add(kind, "".join(s), origin)

    def no_anchor(self):
        """from a repeated or shared stretch only: every bait window of the read is held twice"""
        rng, k = self.rng, self.k
        if not self.what["stretches"]:
            return self.slice()
        r, p, n = rng.choice(self.what["stretches"])
        rec = self.recs[self.what[r]]
        L = self.uniform or rng.randint(k, n)
        m = min(L, n)
        at = rng.randint(0, n - m)
        s = rec[p + at:p + at + m]
        s = s + _dna(rng, L - m)
        self.add("no_anchor", revcomp(s) if rng.random() < 0.5 else s)

    def tie(self):
        """two halves of one length from two places, an N between them"""
        rng, k = self.rng, self.k
        L = self.length(2 * k + 1, 400)
        h = (L - 1) // 2
        if h < k:
            return self.slice()
        rec = self.recs[self.what["a"]]
        p, q = rng.randrange(0, len(rec) // 2 - h), rng.randrange(len(rec) // 2, len(rec) - h)
        s = rec[p:p + h] + "N" + rec[q:q + h]
        self.add("tie", s + "A" * (L - len(s)))

    def random(self):
        self.add("random", _dna(self.rng, self.length(), self.rng.choice([0.0, 0.0, 0.1])))

    def stack(self):
        """50 copies of one read and its reverse complement; the read holds a base that is not the bait's"""
        rng, k = self.rng, self.k
        j = self.what["a"]
        rec, L = self.recs[j], self.uniform or rng.randint(k + 20, 200)
        lo = rng.randrange(0, len(rec) - L)
        s = list(rec[lo:lo + L])
        s[L // 2] = "CGTA"["ACGT".index(s[L // 2].upper())] if s[L // 2].upper() in "ACGT" else "A"
        for i in range(50):
            self.add("stack", "".join(s), (j, i % 2, lo, lo + L))

    def tiling(self):
        """one read of 5000 to 9000 bases: tiles of a long record on diagonals of their own, one of them the longest"""
        rng, k = self.rng, self.k
        rec = self.recs[self.what["a"]]
        goal, tiles = rng.randint(5000, 9000), []
        big = rng.randrange(10)
        while sum(len(t) for t in tiles) < goal or len(tiles) < 80:
            n = 300 if len(tiles) == big else rng.randint(k + 1, k + 20)
            p = rng.randrange(0, len(rec) - n)
            tiles.append(rec[p:p + n])
        self.add("tiling", "".join(tiles)[:9000])


KINDS = (("slice", 30), ("overhang", 12), ("junction", 6), ("indel", 14), ("junky", 8), ("no_anchor", 6), ("tie", 4), ("random", 14))


def _read_set(rng, k, recs, what, uniform, n, tiling):
    r = _Reads(rng, k, recs, what, uniform)
    r.stack()
    if tiling:
        r.tiling()
    kinds = [(name, w) for name, w in KINDS if name != "junction" or (what["adjacent"] and (not uniform or uniform >= 2 * k))]
    names = rng.choices([name for name, _ in kinds], weights=[w for _, w in kinds], k=n - len(r.out))
    for name in names:
        getattr(r, name)()
    rng.shuffle(r.out)
    return r.out


def _mates(rng, k, recs, reads, window):
    """the second set: the mate of every read of the first, on the reverse strand of its fragment; some diverged so far that no window
    of k bases is the bait's -- by substitutions, or by invalid bases, which a rescue at 0 mismatches still takes -- (only rescue places
    those), some in another record, some random"""
    lo_ins, hi_ins = window
    gap = max(6, min(k - 1, 14))
    out = []
    for kind, s, origin in reads:
        L = len(s)
        how = rng.choices(("mate", "diverged", "elsewhere", "random"), weights=(62, 14, 10, 14))[0]
        if origin is None or L == 0 or how == "random":
            out.append(("random", _dna(rng, L)))
            continue
        j, strand, lo, hi = origin
        if how == "elsewhere":
            j2 = rng.choice([i for i, r in enumerate(recs) if len(r) >= 200])
            p = rng.randrange(0, len(recs[j2]) - min(L, 150))
            out.append((how, _piece(rng, recs[j2], p, p + L)))
            continue
        d = rng.randint(lo_ins, hi_ins) if how == "diverged" or rng.random() < 0.5 else max(int(L * rng.uniform(0.5, 3.0)), 1)
        m = revcomp(_piece(rng, recs[j], lo + d - L, lo + d)) if strand == 0 else _piece(rng, recs[j], hi - d, hi - d + L)
        if how == "diverged":                            # another letter, or an invalid one, in every window of k bases
            t, invalid = list(m), rng.random() < 0.5
            for i in range(gap - 1, L, gap):
                t[i] = "N" if invalid else "CGTA"["ACGT".index(t[i].upper())] if t[i].upper() in "ACGT" else "A"
            m = "".join(t)
        else:
            m = _substituted(rng, m, 0.01)
        out.append((how, m))
    return out


# ------------------------------------------------------------------ one seed
def config(seed):
    rng = random.Random(19000 + seed)
    k = K_LIST[seed % len(K_LIST)]
    records, what = _bait(rng, k, seed)
    recs = [s for _, s in records]
    uniform = rng.choice([L for L in (k, k + 1, 64, 100, 150) if L >= k]) if seed % 3 == 0 else 0
    tiling = seed % 4 == 1 and not uniform
    n = rng.randint(200, 600)
    reads = _read_set(rng, k, recs, what, uniform, n, tiling)
    lens = sorted(len(s) for _, s, origin in reads if origin is not None)
    width = rng.choice([8, 32, 100])
    min_insert = max(int(lens[len(lens) // 2] * rng.choice([0.8, 1.0, 1.5])), 1)
    window = (min_insert, min_insert + width - 1)
    assert window[1] - window[0] + 1 <= RESCUE_MAX
    mates = _mates(rng, k, recs, reads, window)
    c = {
        "seed": seed, "k": k, "records": records, "text": fasta(records), "what": what, "uniform": uniform,
        "seqs1": [s for _, s, _ in reads], "kinds1": [kind for kind, _, _ in reads], "seqs2": [s for _, s in mates], "kinds2": [kind for kind, _ in mates],
        "thr": rng.choice([t for t in (1, 1, 2, 3, 8) if not uniform or t <= uniform - k + 1]), "mode": rng.randrange(2), "min_depth": rng.choice([1, 2, 5]), "max_permille": rng.choice([0, 20, 60, 1000]),
        "band": rng.choice([0, 1, 4, 8, min(31, k - 1)]), "keep": rng.randrange(3), "extend": rng.choice([0, 1, 16, 64, EXTEND_MAX]),
        "rescue_permille": rng.choice([0, 100, 300]), "min_insert": window[0], "max_insert": window[1],
        "group": rng.choice([(None, 0), ("_", 1), ("_", 3)]),
    }
    c["told"] = dict({"seed": seed, "k": k, "records": [len(s) for s in recs], "n_reads": len(reads), "uniform": uniform, "tiling": tiling,
                      "junk": what["junk"]}, **{p: c[p] for p in PARAMS})
    return c


def expected(c):
    """every oracle result of one configuration, computed once: the placement oracle and its tallies of both sets, then placement,
    pile-up, verification, alignment with its insertion and extension piles, and the pairs with and without rescue"""
    from tests import extend_oracle as xo
    from tests import pair_oracle as pa
    from tests import place_oracle as po
    from tests import verify_oracle as vo
    k, s1, s2, thr, cut, band = c["k"], c["seqs1"], c["seqs2"], c["thr"], c["max_permille"], c["band"]
    o = po.PlaceOracle(c["text"], k)
    t1, t2 = o.tally(s1), o.tally(s2)
    X = xo.ExtendOracle(o)
    V = vo.VerifyOracle(o)
    P = pa.PairOracle(o)
    e = {"o": o, "t1": t1, "t2": t2, "X": X, "G": X.G, "A": X.A, "V": V, "P": P, "Pile": V.P}
    e["place"] = o.place(t1, thr)
    e["pile"] = V.P.pile(s1, e["place"][1])
    e["verify"] = V.verify(s1, t1, thr, cut)
    e["align"] = X.A.run(s1, t1, thr, cut, band)
    e["ins"] = X.G.pile(s1, e["align"], band)
    e["ext"] = X.pile(s1, e["align"], band, c["extend"]) if c["extend"] else None
    e["pairs"] = P.pairs(s1, s2, t1, t2, thr, cut, c["min_insert"], c["max_insert"], 1, c["rescue_permille"])
    e["pairs_alone"] = P.pairs(s1, s2, t1, t2, thr, cut, c["min_insert"], c["max_insert"], 0, c["rescue_permille"])
    return e
