"""The quality filter's decisions as functions (mitoflex_amd/csrc/mf_qualdecide.h; over a batch on several threads:
qual_check_cut_batch of mf_pl_stages.h), called directly by tests/native/qualdecide_check.cpp -- no reader, no thread around them, no
device -- plain, under ASan + UBSan and under TSan, and compared with a restatement written from oracle/filter_v2_ref.py."""
import random
import struct
import subprocess

import pytest

from oracle.filter_v2_ref import f32, f32_as_usize, lines_of
from tests.native_host import FLAG_IDS, FLAG_SETS, build_check, clean


# ---------------------------------------------------------------- the restatement (filter_v2_ref.run, one rule at a time)
def ref_check_cut(mates, start, end):
    """mates: per mate a list of (head, seq, qual).  -> (first record at which the reference panics, or n; the strings afterwards)"""
    n = len(mates[0])
    out = [[(s, q) for _, s, q in m] for m in mates]
    for i in range(n):
        try:
            for m in mates:
                for x in m[i]:                                       # head, seq, qual are unwrapped; the '+' line never is
                    x.decode("utf-8")
        except UnicodeDecodeError:
            return i, out
        if start and any(start > len(m[i][1]) for m in mates) or start and any(start > len(m[i][2]) for m in mates):
            return i, out                                            # drain(..start) out of range
        for k, m in enumerate(mates):
            s, q = m[i][1], m[i][2]
            if start:
                s, q = s[start:], q[start:]
            if end:
                s, q = s[:end - start], q[:end - start]
            out[k][i] = (s, q)
    return n, out


def f32_mul(a, b):
    try:
        return f32(f32(a) * b)
    except OverflowError:                                            # (struct cannot pack what rounds to an infinity)
        return float("inf") if (a > 0) == (b > 0) else float("-inf")


def ref_drop(nm, sl1, ql1, nc, bc, ns, limit):
    if nc[0] > ns or (nm == 2 and nc[1] > ns):
        return True
    cutoff = f32_as_usize(f32_mul(sl1 if nm == 2 else ql1, limit))   # PE: seq1's length; SE: the quality string's
    return bc[0] >= cutoff or (nm == 2 and bc[1] >= cutoff)


def ref_take(alive, dup, sl, trim, budget):
    keep, stop = [0] * len(sl), False
    for i in range(len(sl)):
        if (alive is not None and not alive[i]) or (dup is not None and dup[i]):
            continue
        if trim:
            budget += sl[i]
            if budget > trim:
                stop = True
                break
        keep[i] = 1
    return keep, sum(keep), stop, budget


# ---------------------------------------------------------------- the cases
def hx(b):
    return b.hex() if b else "-"


def limit_bits(x):
    """(bits as the program reads them, the f32 value)"""
    raw = struct.pack(">f", x) if isinstance(x, float) else bytes.fromhex(x)
    return raw.hex(), struct.unpack(">f", raw)[0]


BAD_UTF8 = [b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xe2\x82", b"\xf0\x9f\x92", b"\x80", b"ACGT\xbf", b"\xf5\x80\x80\x80", b"\xf4\x90\x80\x80"]
GOOD_UTF8 = [b"caf\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x92\xa9", b"\xed\x9f\xbf", b"\xf4\x8f\xbf\xbf", b"ABCDEFG\xc3\xa9", b"ABCDEFGH\xc3\xa9"]


def cut_cases():
    rec = lambda i, s=b"ACGTNACGTNAC", q=b"IIIIIIIIIIII": (b"@r%d" % i, s, q)
    cases = []
    # the cut itself: start, end, end shorter than the line, start == end, end beyond the line, no cut
    for start, end in ((0, 0), (0, 5), (3, 8), (4, 4), (0, 100), (2, 100), (12, 12), (12, 20)):
        for nm in (1, 2):
            cases.append(([[rec(0), rec(1, b"ACGTNACG", b"IIIIIIII"), rec(2)] for _ in range(nm)], start, end))
    # start beyond one string only, each of the four in turn; mate 2's quality is the last looked at
    for which in range(4):
        m1, m2 = [rec(0), list(rec(1)), rec(2)], [rec(0), list(rec(1)), rec(2)]
        (m1, m2)[which % 2][1][1 + which // 2] = b"ACGT"
        cases.append(([[tuple(r) for r in m1], [tuple(r) for r in m2]], 5, 9))
    for which in (1, 2):
        m1 = [rec(0), list(rec(1)), rec(2)]
        m1[1][which] = b""
        cases.append(([[tuple(r) for r in m1]], 1, 0))
    # invalid UTF-8 in head, sequence, quality of either mate; valid multi-byte text passes
    for bad in BAD_UTF8:
        for field in range(3):
            for mate in (0, 1):
                ms = [[rec(0), list(rec(1)), rec(2)] for _ in range(2)]
                ms[mate][1][field] = b"ACGTACGTAC" + bad
                cases.append(([[tuple(r) for r in m] for m in ms], 2, 0))
                if mate == 0:
                    cases.append(([[tuple(r) for r in ms[0]]], 0, 0))
    for good in GOOD_UTF8:
        cases.append(([[(b"@" + good, good + b"ACGT", b"IIII" + good)]], 0, 0))
    # the first record, the last record, every record bad; no record at all
    cases.append(([[rec(0, b"A"), rec(1)]], 2, 0))
    cases.append(([[rec(0), rec(1, b"A")]], 2, 0))
    cases.append(([[]], 2, 0))
    # through lines_of, as the reference meets them: CR LF endings, an invalid '+' line (never looked at), a partial record at the end
    text = b"@a\r\nACGTACGT\r\n+\xff\xfe\r\nIIIIIIII\r\n@b\nAC\n+\nII\n@c\nACGTAC\n+\nIIIIII\n@d\nAC"
    ln = lines_of(text)
    cases.append(([[(ln[i], ln[i + 1], ln[i + 3]) for i in range(0, len(ln) - 3, 4)]], 3, 6))
    return cases


def drop_cases():
    cases = []
    lim = 0.2
    # N count at the boundary: dropped at > ns, not at == ns; either mate
    for ns in (0, 3, 10):
        for n1 in (ns - 1, ns, ns + 1):
            for n2 in (ns - 1, ns, ns + 1):
                for nm in (1, 2):
                    cases.append((nm, 100, 100, (max(n1, 0), max(n2, 0)), (0, 0), ns, lim))
    # low-quality count at the boundary: dropped at >= cutoff; either mate
    for ln in (5, 100, 150, 151):
        cut = f32_as_usize(f32_mul(ln, limit_bits(lim)[1]))
        for b1 in (cut - 1, cut, cut + 1):
            for b2 in (cut - 1, cut, cut + 1):
                for nm in (1, 2):
                    cases.append((nm, ln, ln, (0, 0), (max(b1, 0), max(b2, 0)), 10, lim))
    # the length behind the cutoff: seq1's for pairs (mate 2 longer or shorter does not count), the quality string's for single end
    for sl, ql in ((100, 50), (50, 100), (0, 100), (100, 0)):
        for b in range(0, 25):
            for nm in (1, 2):
                cases.append((nm, sl, ql, (0, 0), (b, 0), 10, lim))
                cases.append((nm, sl, ql, (0, 0), (0, b), 10, lim))
    # limits: 0, negative, NaN (both signs), infinities, one that saturates as a finite f32, one whose product overflows f32, denormal
    for lm in (0.0, -0.0, -0.5, -1e30, "7fc00000", "ffc00000", "7f800000", "ff800000", 1e18, 3e38, 1e-45, 1.0, 0.999, 1e-3):
        for ln in (0, 1, 100, 150):
            for b in (0, 1, 100, 0xFFFFFFFF):
                for nm in (1, 2):
                    cases.append((nm, ln, ln, (0, 0), (b, b // 2), 10, lm))
    # limit * len just below, at and just above an integer: every length up to 400 for limits around the usual ones
    for lm in (0.05, 0.1, 0.2, 0.25, 0.3, 0.5, 0.7, 0.9, 0.99):
        for ln in range(0, 401):
            cut = f32_as_usize(f32_mul(ln, limit_bits(lm)[1]))
            for b in (max(cut - 1, 0), cut):
                cases.append((1, 7, ln, (0, 0), (b, 0), 10, lm))
                cases.append((2, ln, 7, (0, 0), (0, b), 10, lm))
    return cases


def take_cases():
    cases = []
    sl = [10, 20, 30, 40]
    one = [1, 1, 1, 1]
    for trim, budget in ((0, 0), (100, 0), (99, 0), (101, 0), (60, 0), (59, 0), (9, 0), (10, 0), (100, 95), (100, 90), (100, 100), (5, 7)):
        cases.append((trim, budget, one, None, sl))                  # met exactly (kept), overflowed by one, by the batch's first record
        cases.append((trim, budget, None, None, sl))
        cases.append((trim, budget, [1, 0, 1, 1], [0, 0, 1, 0], sl))   # the dropped and the duplicates add nothing to the budget
        cases.append((trim, budget, [0, 0, 0, 0], None, sl))
        cases.append((trim, budget, one, [1, 1, 1, 1], sl))
    cases.append((50, 0, one, None, [0, 0, 50, 0]))                  # records of length 0 behind a budget that is met are still kept
    cases.append((50, 0, None, None, []))
    rng = random.Random(7)
    for _ in range(200):
        n = rng.randrange(0, 40)
        cases.append((rng.choice([0, 1, 50, 500, 5000]), rng.randrange(0, 100), rng.choice([None, [rng.randrange(2) for _ in range(n)]]),
                      rng.choice([None, [rng.randrange(2) for _ in range(n)]]), [rng.choice([0, 1, 100, 150, 151]) for _ in range(n)]))
    return cases


def par_cases():
    cases = []
    for threads in (1, 2, 8):
        for n in (4095, 4096, 4097, 20000):
            for nm in (1, 2):
                chunk = n // min(threads, n // 4096 + 1)
                bads = [[], [0], [n - 1], [chunk - 1, chunk], [chunk + 1, n - 2], [n // 2 + 1, 7], [n - 1, chunk, 3 * n // 4]]
                for b in bads:
                    cases.append((threads, n, nm, 3, [x for x in b if 0 <= x < n]))
    return cases


@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_decisions_match_the_restatement(tmp_path, flags):
    exe = build_check(("qualdecide_check.cpp",), flags)
    cuts, drops, takes, pars = cut_cases(), drop_cases(), take_cases(), par_cases()
    lines = []
    for mates, start, end in cuts:
        lines.append("cut %d %d %d %d" % (len(mates), start, end, len(mates[0])))
        for i in range(len(mates[0])):
            lines.append(" ".join(hx(x) for m in mates for x in m[i]))
    for nm, sl, ql, nc, bc, ns, lm in drops:
        lines.append("drop %d %d %d %d %d %d %d %d %s" % (nm, sl, ql, nc[0], nc[1], bc[0], bc[1], ns, limit_bits(lm)[0]))
    for trim, budget, alive, dup, sl in takes:
        lines.append("take %d %d %d %d %d" % (trim, budget, alive is not None, dup is not None, len(sl)))
        for i in range(len(sl)):
            lines.append("%d %d %d" % (alive[i] if alive else 0, dup[i] if dup else 0, sl[i]))
    for threads, n, nm, start, bad in pars:
        lines.append("par %d %d %d %d %s" % (threads, n, nm, start, " ".join(map(str, bad))))
    cmd = tmp_path / "commands.txt"
    cmd.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(cmd)], capture_output=True)
    clean(p.stderr)
    assert p.returncode == 0
    got = p.stdout.decode().splitlines()
    assert len(got) == len(cuts) + len(drops) + len(takes) + len(pars)
    it = iter(got)
    for mates, start, end in cuts:
        bad, out = ref_check_cut(mates, start, end)
        want = "cut %d" % bad + "".join(" %s %s" % (hx(out[k][i][0]), hx(out[k][i][1])) for i in range(len(mates[0])) for k in range(len(mates)))
        assert next(it) == want, (mates, start, end)
    for c in drops:
        nm, sl, ql, nc, bc, ns, lm = c
        assert next(it) == "drop %d" % ref_drop(nm, sl, ql, nc, bc, ns, limit_bits(lm)[1]), c
    for c in takes:
        trim, budget, alive, dup, sl = c
        keep, kept, stop, b = ref_take(alive, dup, sl, trim, budget)
        assert next(it) == "take %s %d %d %d" % ("".join(map(str, keep)) or "-", kept, stop, b), c
    for c in pars:
        assert next(it) == "par %d" % min(c[4] + [c[1]]), c          # the lowest index wins, whichever chunk finds its own first
