"""The pairing of the two mates' batches (MateZip, mitoflex_amd/csrc/mf_pl_stages.h) on its own: tests/native/matezip_check.cpp feeds it
from two threads with batches of unequal sizes, plain and under the sanitizers (TSan: the channels and the pool between the threads)."""
import itertools
import random
import subprocess

import pytest

from tests.native_host import FLAG_IDS, FLAG_SETS, build_check, clean


def expected(s1, s2):
    """Pair batches end wherever a batch of either mate ends; the shorter mate bounds them.  -> [(n, first1, first2, index1, index2)]"""
    mates = [s1] if s2 is None else [s1, s2]
    ends = [list(itertools.accumulate(s)) for s in mates]
    total = min(e[-1] if e else 0 for e in ends)
    cuts = sorted({c for e in ends for c in e if 0 < c <= total} | ({total} if total else set()))
    out, a = [], 0
    for c in cuts:
        firsts = [a - max([0] + [x for x in e if x <= a]) for e in ends]          # offset into the batch of that mate which holds record a
        out.append((c - a, firsts[0], firsts[1] if s2 is not None else 0, a, a if s2 is not None else 0))
        a = c
    return out


def cases():
    rng = random.Random(3)
    c = [([5, 5, 5], [5, 5, 5]), ([7], [3, 4]), ([1, 2, 3, 4], [10]), ([4, 4, 4], [6, 6, 6]),          # equal, one against many, staggered, a mate longer
         ([3, 3], [2, 2, 2, 2, 2]), ([9, 9, 9, 9], [10]), ([10], [3]),                                # a mate that ends early, inside and at a border
         ([], [4, 4]), ([4, 4], []), ([], []),                                                        # a mate without a batch
         ([3, 0, 3], [0, 2, 0, 4, 0]), ([5, 5], None), ([], None), ([1] * 40, [40]), ([1], [1])]
    for _ in range(40):
        mk = lambda: [rng.choice([1, 2, 3, 17, 64, 700, 1500]) for _ in range(rng.randrange(0, 25))]
        c.append((mk(), rng.choice([None, mk(), mk()])))
    return c


@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_mates_are_paired_by_record_count(flags):
    exe = build_check(("matezip_check.cpp",), flags)
    for k, (s1, s2) in enumerate(cases()):
        arg = lambda s: ",".join(map(str, s))
        for seed in (0, k + 1):                                       # feeders at full speed, and with pauses
            p = subprocess.run([exe, arg(s1), "-" if s2 is None else arg(s2), str(seed)], capture_output=True, timeout=120)
            clean(p.stderr)
            got = [tuple(map(int, ln.split())) for ln in p.stdout.decode().splitlines()]
            assert p.returncode == 0 and got == expected(s1, s2), (s1, s2, seed, p.stdout[-300:])
            # records 0 .. min(n1, n2) - 1 of both mates once, in order (the program has checked the records themselves)
            assert sum(g[0] for g in got) == min(sum(s1), sum(s2) if s2 is not None else sum(s1))
