"""Which kernels a filter pass runs, on which buffer set and which streams, is decided by one pure function (mitoflex_amd/csrc/mf_passplan.h:
plan_pass), next to the one definition of a pass's tally block (TallyLayout) and the feedback a call leaves for the next (adapt_after_call).
None of it needs a device: tests/native/passplan_check.cpp reads rows of integers and prints one answer a row, under ASan + UBSan, and every
answer is compared with the rules restated here -- written from the decision table, not derived from the C++."""
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCREENED, EXACT_MAX_GRID = 0, 2048

KNOBS = {"pass": (0, 1, 2), "finish_streams": (0, 1, 2), "screen_streams": (1, 2), "split_pipe": (0, 1), "exact_co": (0, 1), "knob_s8": (-1, 0, 1)}
INPUTS = {"prot": (0, 1), "s": (0, 16), "stride": (8, 16), "kw": (1, 2), "k": (21, 31, 47, 48, 63), "set_s8": (0, 1),
          "thr": (1, 2), "mode": (0, 1), "count_all": (0, 1), "overlap": (0, 1), "more": (0, 1),
          "prefer_split": (0, 1), "finish_two": (0, 1), "split_serial": (0, 1), "flip": (0, 1), "cur": (0, 1, 2), "nsets": (2, 3, 4)}
FIELDS = list(KNOBS) + list(INPUTS)
DOMAIN = dict(KNOBS, **INPUTS)
# a pipelined threshold-1 call on the 16.5 kbp bait at k = 31, not its last pass -- and the six other ways test_other_pass_kinds_match_oracle runs it
DEFAULT = dict(zip(FIELDS, (0, 0, 2, 1, 0, -1, 0, 16, 16, 1, 31, 0, 1, SCREENED, 0, 1, 1, 0, 0, 0, 0, 0, 3)))
KINDS = {"default": {}, "split": {"pass": 1}, "serial": {"pass": 2}, "split-co": {"pass": 1, "exact_co": 1}, "split-one-stream": {"pass": 1, "split_pipe": 0},
         "one-screen-stream": {"screen_streams": 1}, "two-finish-streams": {"finish_streams": 2}}


def expected_plan(c):
    """The decision table.  Returns the driver's line: kind two_streams q q_out screen_on later_on screen wait_prev_finish screen_clears_bits
    needs_cand exact_behind_finish exact_coresident flip cur sample_pass tally_regions."""
    def line(kind, two=0, q=0, q_out=0, screen_on="MAIN", later_on="MAIN", screen=0, wait=0, clears=0, cand=0, behind=0, co=0, flip=c["flip"], cur=c["cur"], sample=0, regions=1):
        return " ".join(str(int(x) if not isinstance(x, str) else x) for x in (kind, two, q, q_out, screen_on, later_on, screen, wait, clears, cand, behind, co, flip, cur, sample, regions))
    if c["prot"]:          # one kernel on the main stream, bits and tally of the current set
        return line("PROTEIN", q_out=c["cur"])
    screened = c["mode"] == SCREENED and c["s"] > 0
    s8_finish = c["set_s8"] != 0 if c["knob_s8"] < 0 else c["knob_s8"] == 1
    if screened and c["pass"] != 1 and not c["prefer_split"] and c["thr"] == 1 and not c["count_all"] and (c["stride"] == 16 or c["pass"] == 2 or s8_finish):
        two = bool(c["overlap"]) and c["pass"] == 0
        q = (c["cur"] + 1) % (c["nsets"] if two and c["kw"] == 2 else 2)
        odd = c["flip"] ^ 1
        fin2 = c["finish_streams"] == 2 or (c["finish_streams"] == 0 and (c["finish_two"] or c["kw"] == 2))
        later = ("FINISH_B" if fin2 and odd else "FINISH_A") if two else "MAIN"
        screen_on = "SCREEN_ALT" if two and c["screen_streams"] == 2 and odd else "MAIN"
        behind = c["k"] >= 48
        # the tally regions the pass writes: the two phases of the finish kernels, and the third only with the exact kernel behind them
        return line("FINISH", two, q, q, screen_on, later, 1, two, 1, behind, behind, behind and c["more"], odd, q, 1, 3 if behind else 2)
    if screened and not c["count_all"] and c["overlap"] and c["split_pipe"] and c["pass"] != 2 and not c["split_serial"]:
        q = (c["cur"] + 1) % (c["nsets"] if c["kw"] == 2 else 2)
        odd = c["flip"] ^ 1
        screen_on = "SCREEN_ALT" if c["screen_streams"] == 2 and odd else "MAIN"
        return line("SPLIT_PIPELINED", 1, q, q, screen_on, "FINISH_A", 1, 1, 0, 1, 0, c["more"] or c["exact_co"], odd, q, 0)
    # records and candidates of set 0, bits and tally of the current set; screen and mark only when screened
    return line("ONE_STREAM", q=0, q_out=c["cur"], screen=screened, cand=screened)


def _cases():
    rng = random.Random(20261018)
    cases = [{f: rng.choice(DOMAIN[f]) for f in FIELDS} for _ in range(100_000)]
    for changes in KINDS.values():          # every single-input variation around the seven configurations
        base = dict(DEFAULT, **changes)
        cases += [dict(base, **{f: v}) for f in FIELDS for v in DOMAIN[f]]
    return cases


def _row(c):
    return " ".join(str(c[f]) for f in FIELDS)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("passplan")
    exe = str(d / "passplan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "passplan_check.cpp"), "-o", exe])

    def run(rows):
        path = str(d / "rows.txt")
        with open(path, "w") as f:
            f.write("".join(r + "\n" for r in rows))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def test_the_cases_reach_every_kind_and_every_rule():
    cases = _cases()
    assert len(cases) == 100_000 + 7 * sum(len(DOMAIN[f]) for f in FIELDS)
    plans = [expected_plan(c).split() for c in cases]
    assert {p[0] for p in plans} == {"PROTEIN", "FINISH", "SPLIT_PIPELINED", "ONE_STREAM"}
    for kind, column, values in (("FINISH", 1, "01"), ("FINISH", 2, "0123"), ("FINISH", 4, ("MAIN", "SCREEN_ALT")), ("FINISH", 5, ("MAIN", "FINISH_A", "FINISH_B")),
                                 ("FINISH", 10, "01"), ("FINISH", 11, "01"), ("SPLIT_PIPELINED", 2, "0123"), ("SPLIT_PIPELINED", 4, ("MAIN", "SCREEN_ALT")),
                                 ("SPLIT_PIPELINED", 11, "01"), ("ONE_STREAM", 3, "012"), ("ONE_STREAM", 6, "01"),
                                 ("FINISH", 15, "23"), ("SPLIT_PIPELINED", 15, "1"), ("ONE_STREAM", 15, "1"), ("PROTEIN", 15, "1")):
        assert {p[column] for p in plans if p[0] == kind} == set(values), (kind, column)
    # the seven configurations are the seven they are named for
    kinds = {name: expected_plan(dict(DEFAULT, **ch)).split() for name, ch in KINDS.items()}
    assert [kinds[n][0] for n in KINDS] == ["FINISH", "SPLIT_PIPELINED", "FINISH", "SPLIT_PIPELINED", "ONE_STREAM", "FINISH", "FINISH"]
    assert kinds["serial"][1] == "0" and kinds["split-co"][11] == "1" and kinds["one-screen-stream"][4] == "MAIN" and kinds["two-finish-streams"][5] == "FINISH_B"


def test_plan_pass_follows_the_decision_table(run):
    cases = _cases()
    got = run(["plan " + _row(c) for c in cases])
    assert len(got) == len(cases)
    wrong = [(c, g, expected_plan(c)) for c, g in zip(cases, got) if g != expected_plan(c)]
    assert not wrong, (len(wrong), wrong[:3])


def test_seven_passes_rotate_sets_and_streams(run):
    k41 = dict(DEFAULT, kw=2, k=41)
    got = run(["seq 7 " + _row(DEFAULT), "seq 7 " + _row(k41)])
    one, two = [g.split() for g in got[:7]], [g.split() for g in got[7:]]
    assert len(got) == 14 and {p[0] for p in one + two} == {"FINISH"}
    # one-word keys: two sets in turn, every other screen on the alternate stream, all finish kernels on one stream
    assert [int(p[2]) for p in one] == [1, 0, 1, 0, 1, 0, 1] == [int(p[13]) for p in one]
    assert [p[4] for p in one] == ["SCREEN_ALT", "MAIN", "SCREEN_ALT", "MAIN", "SCREEN_ALT", "MAIN", "SCREEN_ALT"]
    assert [p[5] for p in one] == ["FINISH_A"] * 7
    # two-word keys: three sets in turn, the finish kernels of consecutive passes on two streams
    assert [int(p[2]) for p in two] == [1, 2, 0, 1, 2, 0, 1] == [int(p[13]) for p in two]
    assert [p[4] for p in two] == ["SCREEN_ALT", "MAIN", "SCREEN_ALT", "MAIN", "SCREEN_ALT", "MAIN", "SCREEN_ALT"]
    assert [p[5] for p in two] == ["FINISH_B", "FINISH_A", "FINISH_B", "FINISH_A", "FINISH_B", "FINISH_A", "FINISH_B"]
    # ... and each pass is what the table says of the state the pass before it left
    for start, passes in ((DEFAULT, one), (k41, two)):
        c = dict(start)
        for p in passes:
            assert " ".join(p) == expected_plan(c)
            c.update(flip=int(p[12]), cur=int(p[13]))


def test_a_call_is_summed_over_the_regions_its_pass_wrote(run):
    """One read set, calls of different sets one after the other: nothing clears a tally block between passes, so what a pass does not write is
    what an earlier pass left.  Modelled here: every pass stamps its call's number into the regions its kernels write -- region 0 for every
    kind, region 1 too for screen + finish, region 2 only with the exact kernel behind them (k >= 48) -- of the block of its q_out; a call's
    answer reads the leading tally_regions of the last pass's block and must meet its own stamp alone.  (Summing all three regions after
    every screen + finish pass met the k = 63 stamp in a later k = 31 call: after three pipelined k = 63 passes in the very next call, with
    single passes in the third call.)"""
    k63, k31 = dict(DEFAULT, kw=2, k=63), dict(DEFAULT)
    single = {"overlap": 0, "more": 0}
    calls = [(k63, 3), (k31, 1), (k31, 1), (k31, 1),                                                 # sequence a
             (dict(k63, **single), 1), (dict(k31, **single), 1), (dict(k31, **single), 1),           # sequence b
             (dict(k31, thr=2, **single), 1), (dict(k63, **single), 1), (dict(k31, prot=1), 1), (dict(k31, **single), 1), (dict(k31, **single), 1),
             (dict(k31, k=47, kw=2), 5), (dict(k63, k=48), 5), (dict(k31, k=47, kw=2), 5), (k31, 2)]
    seen_regions, stale_met = set(), []
    for number, (c, steps) in enumerate(calls, 1):
        if number in (1, 5):          # a freshly uploaded read set: zeroed blocks
            blocks, flip, cur = [[0, 0, 0] for _ in range(3)], 0, 0
        for step in range(steps):
            row = dict(c, flip=flip, cur=cur, more=int(c["overlap"] and step + 1 < steps))
            p = run(["plan " + _row(row)])[0].split()
            assert " ".join(p) == expected_plan(row)
            writes = {"FINISH": 3 if int(p[10]) else 2}.get(p[0], 1)          # (by kind and exact_behind_finish: not read from tally_regions)
            blocks[int(p[3])][:writes] = [number] * writes
            flip, cur = int(p[12]), int(p[13])
        regions = int(p[15])
        seen_regions.add(regions)
        assert int(p[3]) == cur and blocks[cur][:regions] == [number] * regions, (number, c, blocks, regions)
        if p[0] == "FINISH" and set(blocks[cur]) - {0, number}:          # what the sum over all three regions would have met
            stale_met.append(number)
    assert seen_regions == {1, 2, 3}
    assert stale_met[:4] == [2, 3, 4, 7] and len(stale_met) >= 6, stale_met          # (sequence a: the next call on; sequence b: the third)


def test_tally_layout(run):
    got = run(["layout", "sum 1", "sum 3", "sum 0"])
    assert got[0].split() == ["12288", "98304", "0", "4096", "8192"] and 3 * EXACT_MAX_GRID * 2 == 12288
    for regions, line in ((1, got[1]), (3, got[2]), (0, got[3])):          # word i holds 3 * i + 1: pairs of (pass, candidate)
        words = [3 * i + 1 for i in range(regions * EXACT_MAX_GRID * 2)]
        assert [int(x) for x in line.split()] == [sum(words[0::2]), sum(words[1::2])], regions


def expected_feedback(prefer_split, finish_two, split_serial, sample_pass, cand, n_reads):
    if n_reads >= 100000:
        if sample_pass:          # work items per read of a screen + finish pass
            prefer_split = prefer_split or cand > n_reads
            finish_two = cand > n_reads // 20
        else:                    # candidate reads per read of a candidate-bitmap pass
            prefer_split = prefer_split and not cand < n_reads // 8
            split_serial = True if cand > n_reads // 20 else False if cand < n_reads // 40 else split_serial
    return "%d %d %d" % (prefer_split, finish_two, split_serial)


def test_adapt_after_call_thresholds(run):
    n = 200_000
    cases = [(a, b, c, sample, cand, reads) for a, b, c, sample in itertools.product((0, 1), repeat=4)
             for reads in (n, 100_000, 99_999, 100_001)
             for at in (reads, reads // 20, reads // 8, reads // 40) for cand in (at - 1, at, at + 1)]
    got = run(["adapt %d %d %d %d %d %d" % c for c in cases])
    assert got == [expected_feedback(*c) for c in cases]
    # literally, at 200 000 reads: the sample pass turns to the candidate bitmap above one work item a read and to two finish streams above 1 / 20;
    # the candidate-bitmap pass turns back below 1 / 8, goes to one stream above 1 / 20 and back to two below 1 / 40; under 100 000 reads nothing moves
    ask = [(0, 0, 0, 1, n, n), (0, 0, 0, 1, n + 1, n), (0, 1, 0, 1, n // 20, n), (0, 0, 0, 1, n // 20 + 1, n),
           (1, 0, 0, 0, n // 8, n), (1, 0, 0, 0, n // 8 - 1, n), (0, 0, 0, 0, n // 20, n), (0, 0, 0, 0, n // 20 + 1, n),
           (0, 0, 1, 0, n // 40, n), (0, 0, 1, 0, n // 40 - 1, n), (0, 0, 0, 1, 99_999 + 1, 99_999), (1, 0, 1, 0, 0, 99_999), (1, 0, 1, 0, 0, 100_000)]
    assert run(["adapt %d %d %d %d %d %d" % c for c in ask]) == ["0 1 0", "1 1 0", "0 0 0", "0 1 0", "1 0 1", "0 0 1", "0 0 0", "0 0 1",
                                                                  "0 0 1", "0 0 0", "0 0 0", "1 0 1", "0 0 0"]
