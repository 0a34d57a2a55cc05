"""mf_filter_fastq_files_aligned over batches, on both ingest paths and on two logical devices, in the manner of the file tests of
test_gpu_keep.py: two mates of 954 reads in batches of 300 (MF_BATCH_READS), so the reports add over four batches a mate and two
workers a device, the read set's work memory grows when the third batch brings a 2 000-base read and then serves shorter batches, and
on the device-ingest path the keep bits of the alignment reach the writer through amend_bits.  The written files are the selected
records of the input byte for byte, and every report equals the sum over the mates of what tests/align_oracle.py gives (band 8, cut 30;
keep bits by the rule of test_gpu_align.check, pairs by the rule of test_gpu_keep.py).  There is no tolerance anywhere.
tests/test_align_data.py holds the mates to their conditions without a device."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import align_data as ad
from tests import align_oracle as ao
from tests import pileup_oracle as pio
from tests import place_oracle as po
from tests.report_data import mf, ol  # noqa: F401  (fixtures)
from tests.test_gpu_align import ALIGN_REC, PILE_REC, PLACE_REC, align_rows, inputs, placement, table
from tests.test_gpu_keep import HOOKS_LIB, ROOT, fastq_records, md5, pair_rule
from tests.util_data import write_fastq

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)          # KEEP_PASSING, KEEP_ACCEPTED, KEEP_PLACED
MIN_DEPTH = 2
GZDEV = {"MF_GZDEV_CHUNK_BYTES": "8192", "MF_GZDEV_SLAB_CHUNKS": "5", "MF_GZDEV_TEXT_PIECE": "100000"}


@pytest.fixture(scope="module")
def mates():
    """the two mates, the long read's index, the oracle's run on each (once for every test below) and the keep bits of every mode"""
    text, parts = inputs()[:2]
    m1, m2, at = ad.align_mates(parts)
    o = placement(31)[0]
    A = ao.AlignOracle(o)
    want = [A.run(m, o.tally(m), 1, ad.FILE_CUT, ad.FILE_BAND) for m in (m1, m2)]
    bits = {keep: [ao.keep_bits(w, keep) for w in want] for keep in MODES}
    return text, (m1, m2), at, o, want, bits


def summed(o, want):
    """the reports of a file-level call from the oracle's runs on its mates: every count adds; covered and the calls come from the sums"""
    add = lambda f: sum(w[f] for w in want)
    cons, pile_rec = pio.PileupOracle(o).call(add("counts"), MIN_DEPTH)
    return {"depth": np.minimum(add("depth"), po.CLAMP), "place_rec": add("place_rec")[:, :4], "align_rec": add("align_rec"), "counts": pio.clamped(add("counts")),
            "consensus": cons, "pile_rec": pile_rec, "indels": add("indels"), "unplaced": [sum(w["unplaced"][i] for w in want) for i in (0, 1)]}


def check_reports(v, s):
    assert np.array_equal(v.base_depth.astype(np.int64), s["depth"])
    assert np.array_equal(table(v.place_records, PLACE_REC[:4]).astype(np.uint64), s["place_rec"]), (table(v.place_records, PLACE_REC[:4]), s["place_rec"])
    assert np.array_equal(align_rows(v.align_records), s["align_rec"]), (align_rows(v.align_records), s["align_rec"])
    assert np.array_equal(table(v.pileup, ("a", "c", "g", "t")), s["counts"])
    assert np.array_equal(v.consensus, s["consensus"])
    assert np.array_equal(table(v.pileup_records, PILE_REC).astype(np.uint64), s["pile_rec"])
    assert np.array_equal(table(v.indels, ("del", "ins", "ins_bases")), s["indels"])
    assert v.unplaced.tolist() == s["unplaced"]
    assert np.array_equal(v.align_records["accepted"], v.place_records["forward"] + v.place_records["reverse"])
    assert np.array_equal(v.align_records["hist"].sum(axis=1), v.align_records["accepted"] + v.align_records["rejected"])


def write_mates(tmp_path, pair, gz):
    ext = ".fq.gz" if gz else ".fq"
    fq = [str(tmp_path / ("a_%d%s" % (m + 1, ext))) for m in (0, 1)]
    plain = [str(tmp_path / ("p_%d.fq" % (m + 1))) for m in (0, 1)]
    for m, prefix in ((0, "a"), (1, "b")):
        write_fastq(fq[m], pair[m], prefix, gz=gz)
        write_fastq(plain[m], pair[m], prefix)
    return fq, [fastq_records(p) for p in plain]


@pytest.mark.parametrize("ingest", ["device-gz", "host-plain"])
def test_files_aligned_over_batches(mf, mates, tmp_path, monkeypatch, ingest):
    text, pair, at, o, want, bits = mates
    gz = ingest == "device-gz"
    monkeypatch.setenv("MF_INGEST", "device" if gz else "host")
    monkeypatch.setenv("MF_BATCH_READS", str(ad.FILE_BATCH))
    for name, value in GZDEV.items():
        monkeypatch.setenv(name, value)
    (fq1, fq2), recs = write_mates(tmp_path, pair, gz)
    n = len(pair[0])
    assert n > 3 * ad.FILE_BATCH and at // ad.FILE_BATCH == 2          # four batches a mate, the long read in the third
    ks = mf.KmerSet.from_text(text, 31)
    out = [str(tmp_path / name) for name in ("o1.fq", "o2.fq", "d1.fq", "d2.fq")]
    path = 1 if gz else 0
    both_mates = summed(o, want)
    call = lambda f2, o2, pair_mode, keep: mf.filter_fastq_files_aligned(ks, fq1, f2, out[2], o2, band=ad.FILE_BAND, pair_mode=pair_mode, min_depth=MIN_DEPTH,
                                                                          max_permille=ad.FILE_CUT, keep=keep)
    for pair_mode, both in ((mf.PAIR_EITHER, False), (mf.PAIR_BOTH, True)):
        kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, out[0], out[1], 1, pair_mode)
        assert (kept0, total0) == (int(pair_rule(bits[0], both).sum()), n)
        base = None
        for keep in MODES:
            v = call(fq2, out[3], pair_mode, keep)
            assert mf.last_ingest_stats()["path"] == path
            sel = pair_rule(bits[keep], both)
            assert (v.kept, v.total) == (int(sel.sum()), n), (pair_mode, keep)
            for m in (0, 1):
                assert open(out[2 + m], "rb").read() == b"".join(r for r, s in zip(recs[m], sel) if s), (pair_mode, keep, m)
            if keep == mf.KEEP_PASSING:
                assert md5(out[2]) == md5(out[0]) and md5(out[3]) == md5(out[1])          # the plain filter's files
            check_reports(v, both_mates)
            base = v if base is None else base
            for f in ("base_depth", "place_records", "align_records", "pileup", "consensus", "pileup_records", "indels", "unplaced"):
                assert np.array_equal(getattr(v, f), getattr(base, f)), (pair_mode, keep, f)          # no report depends on the keep mode
    # single end, mate 1 alone (it holds the long read)
    first = summed(o, want[:1])
    for keep in MODES:
        v = call(None, None, mf.PAIR_EITHER, keep)
        assert mf.last_ingest_stats()["path"] == path
        assert (v.kept, v.total) == (int(bits[keep][0].sum()), n)
        assert open(out[2], "rb").read() == b"".join(r for r, s in zip(recs[0], bits[keep][0]) if s), keep
        check_reports(v, first)
        passing = v.total - int(v.unplaced[1])
        assert v.kept == (passing, passing - int(v.align_records["rejected"].sum()), int(v.align_records["accepted"].sum()))[keep]
    ks.close()


CHILD = (
    "import hashlib, json, sys\n"
    "from mitoflex_amd import mitofilter as mf\n"
    "ks = mf.KmerSet.from_fasta(sys.argv[1], 31)\n"
    "band, cut = int(sys.argv[5]), int(sys.argv[6])\n"
    "out = {}\n"
    "for tag, devices in (('one', [0]), ('two', [0, 1])):\n"
    "    names = [sys.argv[4] + '/' + tag + m + '.fq' for m in '12']\n"
    "    v = mf.filter_fastq_files_aligned(ks, sys.argv[2], sys.argv[3], names[0], names[1], band=band, pair_mode=mf.PAIR_EITHER, devices=devices,\n"
    "                                      min_depth=2, max_permille=cut, keep=mf.KEEP_ACCEPTED)\n"
    "    st = mf.last_ingest_stats()\n"
    "    r = v.align_records\n"
    "    out[tag] = {'kept': v.kept, 'total': v.total, 'path': st['path'], 'n_dev': st['n_devices'],\n"
    "                'records': [[int(x) for x in r[f]] for f in ('accepted', 'rejected', 'compared', 'mismatches', 'insertions', 'deletions', 'gapped')],\n"
    "                'hist': r['hist'].sum(axis=0).tolist(), 'indels': [int(v.indels[f].sum()) for f in ('del', 'ins', 'ins_bases')],\n"
    "                'depth': int(v.base_depth.sum()), 'unplaced': v.unplaced.tolist(),\n"
    "                'md5': [hashlib.md5(open(p, 'rb').read()).hexdigest() for p in names]}\n"
    "print(json.dumps(out))\n")


@pytest.mark.parametrize("ingest", ["device", "host"])
def test_files_aligned_two_devices(mf, mates, tmp_path, ingest):
    """a list of two logical devices on the library with the test hooks (MF_FAKE_DEVICES), in one child process a path: what two devices
    report and write is what one does, and what the oracle gives"""
    text, pair, _, o, want, bits = mates
    gz = ingest == "device"
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    (fq1, fq2), recs = write_mates(tmp_path, pair, gz)
    env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_BATCH_READS=str(ad.FILE_BATCH), PYTHONPATH=ROOT, **GZDEV)
    p = subprocess.run([sys.executable, "-c", CHILD, bait, fq1, fq2, str(tmp_path), str(ad.FILE_BAND), str(ad.FILE_CUT)], capture_output=True, env=env,
                       cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert r["one"]["n_dev"] == 1 and r["two"]["n_dev"] == 2 and r["one"]["path"] == r["two"]["path"] == (1 if gz else 0)
    s = summed(o, want)
    sel = pair_rule(bits[1], False)
    files = [hashlib.md5(b"".join(rec for rec, keep in zip(recs[m], sel) if keep)).hexdigest() for m in (0, 1)]
    expected = {"kept": int(sel.sum()), "total": len(pair[0]), "records": s["align_rec"][:, :len(ALIGN_REC)].T.astype(np.int64).tolist(),
                "hist": s["align_rec"][:, len(ALIGN_REC):].sum(axis=0).astype(np.int64).tolist(), "indels": s["indels"].sum(axis=0).tolist(),
                "depth": int(s["depth"].sum()), "unplaced": s["unplaced"], "md5": files}
    for tag in ("one", "two"):
        got = {f: r[tag][f] for f in expected}
        assert got == expected, tag
