"""The quality filter's host pipeline without a GPU and under sanitizers: tests/native/qualpipe_check.cpp calls mf_qualfilter_files of
tests/native/qualfilter_stub.cpp (the real run_qualfilter_pipeline; the stub stands in for the counting and hashing kernels), linked with
the four host sources.  Output bytes and the `kept total panicked` line are compared with oracle.filter_v2_ref.run at batch sizes 1,
64, 700 and one batch; a parse segment of 997 bytes puts a border inside almost every record."""
import gzip
import os
import random
import subprocess
import threading
import time

import pytest

from oracle.filter_v2_ref import run as oracle_run
from tests.native_host import FLAG_IDS, FLAG_SETS, build_check, clean

N1, N2 = 5000, 5100
BATCHES = (1, 64, 700, 2_000_000)
PANIC_AT = 1033


def make_mate(rng, n, tag, crlf, seqs=None):
    """records with N runs, low-quality stretches, duplicates of earlier sequences, short and empty lines; -> (bytes, sequences)"""
    out, kept_seqs = [], []
    nl = b"\r\n" if crlf else b"\n"
    for i in range(n):
        L = rng.choice([150, 150, 151, 100, 40, 12, 6])
        if seqs is not None and i < len(seqs):
            L = len(seqs[i]) if rng.random() < 0.9 else L              # mate 2 mostly as long as mate 1, now and then longer or shorter
        if kept_seqs and rng.random() < 0.15:
            s = rng.choice(kept_seqs[-50:])                            # a duplicate of a recent sequence
        else:
            s = "".join(rng.choices("ACGT", k=L))
            if rng.random() < 0.3:
                k = rng.randrange(0, 14)
                p = rng.randrange(0, max(1, L - k))
                s = s[:p] + "N" * k + s[p + k:]
            s = s[:L]
        low = rng.choice([0.0, 0.05, 0.15, 0.19, 0.2, 0.21, 0.3, 0.6])
        q = "".join("+" if rng.random() < low else "I" for _ in range(len(s)))
        kept_seqs.append(s)
        head = "@r%d/%s" % (i, tag) + (" café" if i % 97 == 5 else "")
        plus = b"+\xff\xfe" if i % 211 == 17 else b"+"                 # not valid UTF-8: the reference never looks at this line
        out.append(head.encode() + nl + s.encode() + nl + plus + nl + q.encode() + nl)
    return b"".join(out), kept_seqs


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("qualpipe")
    rng = random.Random(20)
    b1, s1 = make_mate(rng, N1, "1", False)
    b2, _ = make_mate(rng, N2, "2", True, s1)
    b1 += b"@partial\nACGT\n"                                          # a partial record at the end is dropped
    lines = b1.split(b"\n")
    lines[4 * PANIC_AT + 1] = b"AC"                                    # shorter than -s 5: the reference panics at this record
    files = {"a_1.fq": b1, "a_2.fq": b2, "p_1.fq": b"\n".join(lines)}
    for name, b in files.items():
        (d / name).write_bytes(b)
        with gzip.open(d / (name + ".gz"), "wb", compresslevel=6) as g:
            g.write(b)
    return d


def read_file(path):
    if path is None or not os.path.exists(path):
        return None
    b = open(path, "rb").read()
    return gzip.decompress(b) if path.endswith(".gz") else b


def index_of(head):
    return int(head.split(b"/")[0][2:])


def oracle(fq1, fq2, opts):
    argv = ["-1", fq1] + (["-2", fq2, "-4", "o2"] if fq2 else []) + ["-3", "o1"] + opts
    rc, o1, o2 = oracle_run(argv, read_file)
    assert rc in (0, 101)
    return rc, o1, o2


def program_args(opts):
    """the CLI's options as the check program's positional arguments: START END NS QUALITY LIMIT DEDUP TRIM TRUNCATE"""
    v = {"-s": "0", "-e": "0", "-n": "10", "-q": "55", "-l": "0.2", "-t": "0"}
    it = iter(opts)
    for o in it:
        if o in v:
            v[o] = next(it)
    return [v["-s"], v["-e"], v["-n"], v["-q"], v["-l"], str(int("-d" in opts)), v["-t"], str(int("--truncate_only" in opts))]


def expected_total(fq1, fq2, opts, rc, o1, batch):
    """records the decision thread has been through: all pairs; up to the record that panics; with a -t budget that stops the run, up
    to the end of the batch that holds the record that overflowed it"""
    n = min(N1, N2) if fq2 else N1
    if rc == 101:
        return PANIC_AT
    if "-t" not in opts:
        return n
    k = opts.index("-t")
    _, all1, _ = oracle(fq1, fq2, opts[:k] + opts[k + 2:])
    kept, untrimmed = o1.split(b"\n")[0::4][:-1], all1.split(b"\n")[0::4][:-1]
    assert untrimmed[:len(kept)] == kept
    if len(kept) == len(untrimmed):
        return n
    return min(n, (index_of(untrimmed[len(kept)]) // batch + 1) * batch)


def trim_for(fq1, target):
    """a -t budget that the first kept record at or behind `target` overflows (single end, defaults)"""
    _, o1, _ = oracle(fq1, None, [])
    ln = o1.split(b"\n")
    return max(1, sum(len(ln[i + 1]) for i in range(0, len(ln) - 3, 4) if index_of(ln[i]) < target))


def run_case(exe, d, tmp, fq1, fq2, opts, batch, gz_out=False, stdout2=False, fifo_slow=None):
    f1, f2 = str(d / fq1), str(d / fq2) if fq2 else None
    rc, w1, w2 = oracle(f1, f2, opts)
    o1, o2 = str(tmp / ("o1.fq.gz" if gz_out else "o1.fq")), str(tmp / "o2.fq")
    in1, in2, feeders = f1, f2, []
    if fifo_slow is not None:
        def feed(src, dst, bursts):
            b = open(src, "rb").read()
            with open(dst, "wb", buffering=0) as w:
                step = len(b) // 5 + 1 if bursts else len(b)
                for a in range(0, len(b), step):
                    w.write(b[a:a + step])
                    if bursts:
                        time.sleep(0.12)                               # longer than the reader's idle time-out: batches are handed over early
        in1, in2 = str(tmp / "p1.fifo"), str(tmp / "p2.fifo")
        for k, (src, dst) in enumerate(((f1, in1), (f2, in2))):
            if os.path.exists(dst):
                os.unlink(dst)
            os.mkfifo(dst)
            feeders.append(threading.Thread(target=feed, args=(src, dst, fifo_slow == k)))
            feeders[-1].start()
    env = dict(os.environ, MF_BATCH_READS=str(batch), MF_PARSE_SEG="997")
    p = subprocess.run([exe, in1, in2 or "-", o1, "-" if (not fq2 or stdout2) else o2, *program_args(opts)], capture_output=True, env=env, timeout=300)
    for t in feeders:
        t.join()
    err = clean(p.stderr)
    what = (fq1, fq2, opts, batch, gz_out, stdout2, fifo_slow)
    assert p.returncode == 0, (what, err[-500:])
    g1 = gzip.decompress(open(o1, "rb").read()) if gz_out else open(o1, "rb").read()
    assert g1 == w1, what
    if fq2:
        assert (p.stdout if stdout2 else open(o2, "rb").read()) == w2, what
    kept = w1.count(b"\n") // 4
    line = err.strip().splitlines()[-1].split()
    assert line[0] == str(kept) and line[2] == str(int(rc == 101)), (what, line)
    if fifo_slow is None:                                              # (batches from a pipe are as long as the producer makes them)
        assert line[1] == str(expected_total(f1, f2, opts, rc, w1, batch)), (what, line)
    else:
        assert line[1] == str(min(N1, N2)), (what, line)
    return kept, rc


@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_quality_pipeline_matches_the_oracle(data, tmp_path, flags):
    exe = build_check(("qualpipe_check.cpp", "qualfilter_stub.cpp"), flags)
    d = data
    for batch in BATCHES:
        kept, _ = run_case(exe, d, tmp_path, "a_1.fq", "a_2.fq", ["-d"], batch)
        assert 0 < kept < min(N1, N2)
        run_case(exe, d, tmp_path, "a_1.fq", "a_2.fq", ["-s", "3", "-e", "100"], batch)
        # single end with a budget that is spent inside the second batch (the only one: in its middle)
        target = batch + batch // 2 if batch < N1 else N1 // 2
        kept, _ = run_case(exe, d, tmp_path, "a_1.fq", None, ["-t", str(trim_for(str(d / "a_1.fq"), target))], batch)
        assert kept <= target and (kept > 0 or batch == 1)
        # a record that panics (its sequence is shorter than -s) in the middle of a batch: everything before it is decided and written
        kept, rc = run_case(exe, d, tmp_path, "p_1.fq", "a_2.fq", ["-s", "5", "-e", "200"], batch)
        assert rc == 101 and kept > 0
        run_case(exe, d, tmp_path, "a_1.fq", "a_2.fq", ["-s", "2", "-e", "90", "--truncate_only"], batch)
        run_case(exe, d, tmp_path, "a_1.fq.gz", "a_2.fq.gz", ["-d", "-s", "2", "-e", "120"], batch)
        run_case(exe, d, tmp_path, "a_1.fq", None, ["-n", "3", "-l", "0.25"], batch, gz_out=True)
        run_case(exe, d, tmp_path, "a_1.fq", "a_2.fq", ["-d", "-t", "200000"], batch, stdout2=True)
        for slow in (0, 1):
            run_case(exe, d, tmp_path, "a_1.fq", "a_2.fq", [], batch, fifo_slow=slow)
