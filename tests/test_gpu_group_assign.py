"""Assignment of baited reads to GROUPS of bait records (mf_kmerset_group_records, mf_assign_groups, mf_filter_fastq_files_by_group,
`fastfilter bait --group-report`), for protein and nucleotide sets, against a plain-Python oracle written from the semantics in
include/mitofilter.h: a key is unique to group g when every record with a valid window holding it belongs to g; a passing read goes
to the group with the strictly largest count of its windows whose key is unique to that group, ambiguous when there is none or a
tie, unassigned when it does not pass.  Protein windows are the (frame, window) pairs that Spec P counts as hits."""
import json
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from oracle import kmer_bait_ref as kb
from oracle import prot_bait_ref as pr
from tests.clade_data import GENES, Clade, gene_dna, sample_reads
from tests.report_data import eight_record_bait, fasta, keys_nuc, keys_prot, mf, ol, upload  # noqa: F401  (mf, ol: fixtures)
from tests.util_data import bits_to_bool, make_protein_bait, make_reads, revcomp, write_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_LIB = os.path.join(ROOT, "mitoflex_amd", "libmitofilter_hip_hooks.so")
CLI = os.path.join(ROOT, "mitoflex_amd", "assemble", "fastfilter")
AMB, NONE = 0xFFFFFFFE, 0xFFFFFFFF


# ------------------------------------------------------------------ oracle
def record_names(text):
    """names in the record order of kb.read_fasta_records: header text up to the first space, tab or CR; "" for leading sequence"""
    names, opened = [], False
    for line in text.split("\n"):
        if line.startswith(">"):
            h = line[1:]
            for c in " \t\r":
                h = h.split(c)[0]
            names.append(h)
            opened = True
        elif "".join(line.split()) and not opened:
            names.append("")
            opened = True
    return names


def grouping(names, sep=None, field=0):
    """-> (group of every record, group names)"""
    if sep is None or field == 0:
        return list(range(len(names))), list(names)
    index, gnames, rg = {}, [], []
    for nm in names:
        parts = nm.split(sep)
        g = parts[field - 1] if len(parts) >= field else nm
        if g not in index:
            index[g] = len(gnames)
            gnames.append(g)
        rg.append(index[g])
    return rg, gnames


def owners_prot(text, kp, rec_group):
    own = {}
    for j, rec in enumerate(pr.protein_records(text)):
        g = rec_group[j]
        for i in range(len(rec) - kp + 1):
            v = pr.pep_code(rec[i:i + kp])
            if v is not None:
                o = own.get(v)
                own[v] = g if o is None or o == g else -1
    return own


def owners_nuc(text, k, rec_group):
    own = {}
    for j, rec in enumerate(kb.read_fasta_records(text)):
        s = kb._norm(rec)
        g = rec_group[j]
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if "N" not in w:
                c = kb.canonical_code(w)
                o = own.get(c)
                own[c] = g if o is None or o == g else -1
    return own


def oracle_assign(read_keys, own, thr, n_groups):
    """read_keys: the window keys of every read -> (passes bool[n], assign u32[n], counts u64[G + 2])"""
    passes = np.zeros(len(read_keys), bool)
    assign = np.full(len(read_keys), NONE, np.uint32)
    for i, ks in enumerate(read_keys):
        hits, u = 0, Counter()
        for v in ks:
            o = own.get(v)
            if o is None:
                continue
            hits += 1
            if o >= 0:
                u[o] += 1
        if hits < thr:
            continue
        passes[i] = True
        m = max(u.values()) if u else 0
        win = [j for j, c in u.items() if c == m]
        assign[i] = win[0] if m and len(win) == 1 else AMB
    return passes, assign, counts_of(assign, n_groups)


def counts_of(assign, n_groups):
    c = np.zeros(n_groups + 2, np.uint64)
    for a in assign:
        c[n_groups + 1 if a == NONE else n_groups if a == AMB else a] += 1
    return c


class Oracle:
    """the expected results for one set and one grouping"""

    def __init__(self, text, k, code=None, sep=None, field=0):
        self.k, self.code = k, code
        self.rec_group, self.names = grouping(record_names(text), sep, field)
        self.own = owners_prot(text, k, self.rec_group) if code else owners_nuc(text, k, self.rec_group)

    def keys(self, seqs):
        return [keys_prot(s, self.k, self.code) if self.code else keys_nuc(s, self.k) for s in seqs]

    def assign(self, seqs, thr, keys=None):
        return oracle_assign(keys if keys is not None else self.keys(seqs), self.own, thr, len(self.names))


# ------------------------------------------------------------------ data
def protein_reads(gene_fa, kp, seed, n=600):
    """reads from the gene DNA with ragged lengths, invalid bases, stop codons put in, and reads shorter than 3kp"""
    rng = random.Random(seed)
    genes = [g for g in kb.read_fasta_records(gene_fa) if len(g) > 60]
    out = []
    for i in range(n):
        g = genes[i % len(genes)]
        L = rng.choice([150, 150, 100, rng.randint(3 * kp - 2, 3 * kp + 2), rng.randint(30, 260)])
        p = rng.randrange(0, max(len(g) - L, 0) + 1)
        s = list(g[p:p + L])
        if i % 7 == 1 and s:
            s[rng.randrange(len(s))] = "N"
        if i % 5 == 2 and len(s) > 12:
            q = rng.randrange(0, len(s) - 3)
            s[q:q + 3] = rng.choice(["TAA", "TAG", "TGA"])
        s = "".join(s)
        out.append(revcomp(s) if i % 3 == 0 else s)
    rng2 = random.Random(seed + 1)
    out += ["".join(rng2.choices("ACGT", k=rng2.randint(1, 160))) for _ in range(n // 10)]
    return out


def check(mf, reads, ks, o, seqs, thr, keys=None, mode=None):
    passes, oassign, ocounts = o.assign(seqs, thr, keys)
    bits, assign, counts = mf.assign_groups(ks, reads, thr, mf.MODE_SCREENED if mode is None else mode)
    assert np.array_equal(bits_to_bool(bits, len(seqs)), passes)
    bad = np.nonzero(assign != oassign)[0]
    assert bad.size == 0, [(int(i), int(assign[i]), int(oassign[i])) for i in bad[:10]]
    assert np.array_equal(counts, ocounts), (counts, ocounts)
    assert ks.group_names == o.names
    return assign, counts


# ------------------------------------------------------------------ 1. protein sets against the oracle
@pytest.mark.parametrize("kp,code", [(4, 1), (7, 2), (9, 5), (12, 9)])
def test_protein_matches_oracle(mf, ol, kp, code):
    prot_fa, gene_fa = make_protein_bait(code=code)
    seqs = protein_reads(gene_fa, kp, seed=kp * 10 + code)
    ks = mf.KmerSet.protein_from_text(prot_fa, kp, code)
    reads = upload(mf, ol, seqs)
    for sep, field in ((None, 0), ("_", 4), ("_", 9)):          # identity; the genus (all but one record); a field no name has
        ks.group_records(sep, field)
        o = Oracle(prot_fa, kp, code, sep, field)
        keys = o.keys(seqs)
        for thr in (1, 2, 3):
            fbits, _, _ = mf.filter_reads(ks, reads, thr)
            bits, assign, counts = mf.assign_groups(ks, reads, thr)
            assert np.array_equal(bits, fbits)
            check(mf, reads, ks, o, seqs, thr, keys)
    reads.close(); ks.close()


def test_protein_names_and_groups(mf):
    text = ("MLSFIVAL\n>a_x_1 desc\r\nMLSFIVALLSS\n>b_y\tdesc\nMLSFIVA*\n>a_z_2\nMKK\n>\nMLSWWT\n>a_x_3\nPPPPMLSF\n")
    ks = mf.KmerSet.protein_from_text(text, 4, 5)
    assert ks.group_names == ["", "a_x_1", "b_y", "a_z_2", "", "a_x_3"]
    ks.group_records("_", 1)
    assert ks.group_names == ["", "a", "b"]
    ks.group_records("_", 2)
    assert ks.group_names == ["", "x", "y", "z"]
    ks.group_records("_", 3)
    assert ks.group_names == ["", "1", "b_y", "2", "3"]
    ks.group_records(None, 3)
    assert ks.group_names == ["", "a_x_1", "b_y", "a_z_2", "", "a_x_3"]
    ks.group_records("__", 2)
    assert ks.group_names == ["", "a_x_1", "b_y", "a_z_2", "a_x_3"]
    with pytest.raises(mf.MitoFilterError):
        ks.group_records("", 2)
    with pytest.raises(mf.MitoFilterError):
        ks.group_records("_", -1)
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        ks.record_names
    ks.close()


# ------------------------------------------------------------------ 2. more than 64 groups in one read, ties
def test_protein_crowded_read_sweeps(mf, ol):
    rng = random.Random(31)
    aas = pr.AA
    prots = ["".join(rng.choices(aas, k=16 + (3 if j in (77, 5) else 0))) for j in range(120)]
    text = fasta([("p%d" % j, p) for j, p in enumerate(prots)])
    drng = random.Random(32)
    bt = lambda p: pr.back_translate(p, 5, drng)
    seqs = [bt("".join(p for j, p in enumerate(prots) if j != 5)),          # unique keys of 119 groups; 77 wins (beyond 64)
            bt("".join(p for j, p in enumerate(prots) if j != 77)),         # ... 5 wins
            bt("".join(prots)),                                              # 5 and 77 tie: ambiguous
            revcomp(bt("".join(p for j, p in enumerate(prots) if j != 5))),  # 77 again, reverse strand
            bt(prots[3] + prots[4])]                                         # two records of 10 unique keys each: a tie
    ks = mf.KmerSet.protein_from_text(text, 7, 5)          # (kp = 7: the read's other frames hit no key by chance)
    reads = upload(mf, ol, seqs)
    o = Oracle(text, 7, 5)
    assign, _ = check(mf, reads, ks, o, seqs, 1)
    assert list(assign) == [77, 5, AMB, 77, AMB]
    reads.close(); ks.close()


# ------------------------------------------------------------------ 3. the point: genes of a clade
@pytest.fixture(scope="module")
def clade():
    return Clade(n_species=10)


def test_unseen_species_resolve_by_gene(mf, ol, clade):
    code, kp = 5, 9
    dna = gene_dna(clade.unseen(0.06, seed=3), code, seed=4)
    seqs, truth = sample_reads(dna, 1300, seed=5)
    ks = mf.KmerSet.protein_from_text(clade.text, kp, code)
    reads = upload(mf, ol, seqs)
    o_id = Oracle(clade.text, kp, code)
    keys = o_id.keys(seqs)
    a_id, c_id = check(mf, reads, ks, o_id, seqs, 1, keys)
    ks.group_records("_", 4)
    o_gene = Oracle(clade.text, kp, code, "_", 4)
    assert o_gene.names == GENES
    a_gene, c_gene = check(mf, reads, ks, o_gene, seqs, 1, keys)
    passing = a_id != NONE
    assert passing.sum() > 0.95 * len(seqs)
    assert (a_id[passing] == AMB).mean() > 0.6                      # record level: mostly ambiguous
    right = np.array([a == GENES.index(t) for a, t in zip(a_gene, truth)])
    assert right[passing].mean() > 0.9                              # gene level: mostly the true gene
    sampled = Counter(truth)
    for j, g in enumerate(GENES):
        assert abs(int(c_gene[j]) - sampled[g]) <= 0.12 * sampled[g], (g, int(c_gene[j]), sampled[g])
    reads.close(); ks.close()


# ------------------------------------------------------------------ 4. nucleotide sets
@pytest.mark.parametrize("k", [21, 31, 41])
def test_nucleotide_identity_equals_record_assignment(mf, ol, k):
    text = eight_record_bait()
    ks = mf.KmerSet.from_text(text, k)
    for uniform in (True, False):
        seqs = make_reads(text, 1500, seed=800 + k, uniform=uniform, mito_frac=0.5)
        seqs = [revcomp(s) if i % 3 == 0 else s for i, s in enumerate(seqs)]
        reads = upload(mf, ol, seqs)
        for thr in (1, 3):
            for mode in (mf.MODE_SCREENED, mf.MODE_EXHAUSTIVE):
                want = mf.assign_reads(ks, reads, thr, mode)
                got = mf.assign_groups(ks, reads, thr, mode)
                for w, g in zip(want, got):
                    assert np.array_equal(w, g)
        reads.close()
    assert ks.group_names == ks.record_names
    ks.close()


def test_nucleotide_crowded_identity(mf, ol):
    from tests.test_gpu_assign import crowded_bait_and_reads
    text, crowded, _ = crowded_bait_and_reads()
    ks = mf.KmerSet.from_text(text, 31)
    reads = upload(mf, ol, crowded)
    want = mf.assign_reads(ks, reads, 1)
    got = mf.assign_groups(ks, reads, 1)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    assert list(got[1]) == [77, 5, AMB, 77]
    reads.close(); ks.close()


def test_nucleotide_field_grouping_and_regrouping(mf, ol):
    text = eight_record_bait()
    k = 31
    seqs = make_reads(text, 2000, seed=61, mito_frac=0.5)
    ks = mf.KmerSet.from_text(text, k)
    reads = upload(mf, ol, seqs)
    before = mf.assign_reads(ks, reads, 1)
    keys = Oracle(text, k).keys(seqs)
    for sep, field in (("_", 1), (None, 0), ("_", 2), ("_", 1)):           # each regrouping rebuilds the group-owner table
        ks.group_records(sep, field)
        check(mf, reads, ks, Oracle(text, k, None, sep, field), seqs, 1, keys)
        after = mf.assign_reads(ks, reads, 1)                                # the record assignment does not move
        for w, g in zip(before, after):
            assert np.array_equal(w, g)
    assert ks.group_names == ["mito", "tiny", "rec2", "rand"]
    reads.close(); ks.close()


def test_protein_record_calls_still_refused(mf, clade):
    ks = mf.KmerSet.protein_from_text(clade.text, 9, 5)
    ks.group_records("_", 4)
    reads = mf.Reads.from_packed(np.zeros(16, np.uint32), np.array([0, 100], np.uint64), np.zeros(0, np.uint64))
    with pytest.raises(mf.MitoFilterError, match="nucleotide"):
        mf.assign_reads(ks, reads, 1)
    reads.close(); ks.close()


# ------------------------------------------------------------------ 5. file level
def file_counts(o, s1, s2, thr, both):
    G = len(o.names)
    p1, a1, _ = o.assign(s1, thr)
    if s2 is None:
        return int(p1.sum()), counts_of(a1[p1], G)
    n = min(len(s1), len(s2))
    p2, a2, _ = o.assign(s2[:n], thr)
    keep = (p1[:n] & p2) if both else (p1[:n] | p2)
    return int(keep.sum()), counts_of(np.concatenate([a1[:n][keep], a2[keep]]), G)


@pytest.fixture(scope="module")
def clade_files(clade):
    dna = gene_dna(clade.unseen(0.05, seed=11), 5, seed=12)
    s1, _ = sample_reads(dna, 400, seed=13)
    s2, _ = sample_reads(dna, 400, seed=14)
    rng = random.Random(15)
    noise1 = ["".join(rng.choices("ACGT", k=150)) for _ in range(1600)]
    noise2 = ["".join(rng.choices("ACGT", k=150)) for _ in range(1600)]
    mix1, mix2 = [], []
    for i in range(2000):          # pairs where one mate, both or neither come from a gene
        a, b = i % 5 == 0, i % 5 in (0, 1)
        mix1.append(s1[i // 5] if a else noise1[i % 1600])
        mix2.append(s2[i // 5] if b else noise2[i % 1600])
    return mix1, mix2


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("pe,pair", [(False, 0), (True, 0), (True, 1)])
def test_files_by_group(mf, clade, clade_files, tmp_path, monkeypatch, path, gz, pe, pair):
    monkeypatch.setenv("MF_INGEST", path)
    s1, s2 = clade_files
    s2 = s2 if pe else None
    ext = ".fq.gz" if gz else ".fq"
    fq1, fq2 = str(tmp_path / ("a_1" + ext)), (str(tmp_path / ("a_2" + ext)) if pe else None)
    write_fastq(fq1, s1, "a", gz=gz)
    if pe:
        write_fastq(fq2, s2, "b", gz=gz)
    ks = mf.KmerSet.protein_from_text(clade.text, 9, 5)
    ks.group_records("_", 4)
    o = [str(tmp_path / n) for n in ("o1.fq", "o2.fq", "g1.fq", "g2.fq")]
    kept0, total0 = mf.filter_fastq_files(ks, fq1, fq2, o[0], o[1] if pe else None, 1, pair)
    kept, total, counts = mf.filter_fastq_files_by_group(ks, fq1, fq2, o[2], o[3] if pe else None, 1, pair)
    assert mf.last_ingest_stats()["path"] == (1 if path == "device" else 0)
    assert (kept, total) == (kept0, total0)
    assert open(o[2], "rb").read() == open(o[0], "rb").read()
    if pe:
        assert open(o[3], "rb").read() == open(o[1], "rb").read()
    okept, ocounts = file_counts(Oracle(clade.text, 9, 5, "_", 4), s1, s2, 1, pair == 1)
    assert kept == okept
    assert np.array_equal(counts, ocounts), (counts, ocounts)
    assert int(counts.sum()) == kept * (2 if pe else 1)
    ks.close()


def test_files_by_group_nucleotide_identity(mf, tmp_path, monkeypatch):
    monkeypatch.setenv("MF_INGEST", "device")
    text = eight_record_bait()
    s1 = make_reads(text, 2500, seed=91, mito_frac=0.3)
    s2 = make_reads(text, 2500, seed=92, mito_frac=0.3)
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    ks = mf.KmerSet.from_text(text, 31)
    a = mf.filter_fastq_files_by_record(ks, fq1, fq2, str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq"), 1, mf.PAIR_BOTH)
    b = mf.filter_fastq_files_by_group(ks, fq1, fq2, str(tmp_path / "g1.fq"), str(tmp_path / "g2.fq"), 1, mf.PAIR_BOTH)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    ks.group_records("_", 1)
    kept, _, counts = mf.filter_fastq_files_by_group(ks, fq1, fq2, str(tmp_path / "h1.fq"), str(tmp_path / "h2.fq"), 1, mf.PAIR_BOTH)
    okept, ocounts = file_counts(Oracle(text, 31, None, "_", 1), s1, s2, 1, True)
    assert kept == okept and np.array_equal(counts, ocounts)
    ks.close()


def test_files_by_group_two_devices(clade, clade_files, tmp_path):
    """a list of two devices on the library with the test hooks (MF_FAKE_DEVICES: two logical devices on the one GPU), on both ingest
    paths; a child process, because the variable is read when the library is loaded"""
    s1, s2 = clade_files
    bait = str(tmp_path / "clade.fa")
    open(bait, "w").write(clade.text)
    okept, ocounts = file_counts(Oracle(clade.text, 9, 5, "_", 4), s1, s2, 1, False)
    for gz, ingest in ((True, "device"), (False, "host")):
        ext = ".fq.gz" if gz else ".fq"
        fq1, fq2 = str(tmp_path / ("a_1" + ext)), str(tmp_path / ("a_2" + ext))
        write_fastq(fq1, s1, "a", gz=gz)
        write_fastq(fq2, s2, "b", gz=gz)
        script = (
            "import json, sys\n"
            "from mitoflex_amd import mitofilter as mf\n"
            "ks = mf.KmerSet.protein_from_fasta(sys.argv[1], 9, 5)\n"
            "ks.group_records('_', 4)\n"
            "a = mf.filter_fastq_files(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/o1.fq', sys.argv[4] + '/o2.fq', 1, 0, devices=[0, 1])\n"
            "b = mf.filter_fastq_files_by_group(ks, sys.argv[2], sys.argv[3], sys.argv[4] + '/g1.fq', sys.argv[4] + '/g2.fq', 1, 0, devices=[0, 1])\n"
            "print(json.dumps({'a': list(a), 'kept': b[0], 'total': b[1], 'counts': [int(x) for x in b[2]], 'path': mf.last_ingest_stats()['path'],"
            " 'n_dev': mf.last_ingest_stats()['n_devices']}))\n")
        env = dict(os.environ, MITOFILTER_LIB=HOOKS_LIB, MF_FAKE_DEVICES="2", MF_INGEST=ingest, MF_GZDEV_CHUNK_BYTES="8192",
                   MF_GZDEV_SLAB_CHUNKS="5", MF_GZDEV_TEXT_PIECE="200000", MF_BATCH_READS="700", PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", script, bait, fq1, fq2, str(tmp_path)], capture_output=True, env=env, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert r["path"] == (1 if ingest == "device" else 0) and r["n_dev"] == 2
        assert r["a"] == [r["kept"], r["total"]]
        for m in ("1", "2"):
            assert open(str(tmp_path / ("g%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
        assert r["kept"] == okept and r["counts"] == [int(x) for x in ocounts]


# ------------------------------------------------------------------ 6. CLI
def _tsv(names, c):
    G = len(names)
    return ("group\tname\treads\n" + "".join("%d\t%s\t%d\n" % (j, n, c[j]) for j, n in enumerate(names))
            + "-\t*ambiguous*\t%d\n-\t*unassigned*\t%d\n" % (c[G], c[G + 1]))


def test_cli_group_report_protein(mf, clade, clade_files, tmp_path):
    s1, s2 = clade_files
    fq1, fq2 = str(tmp_path / "a_1.fq.gz"), str(tmp_path / "a_2.fq.gz")
    write_fastq(fq1, s1, "a", gz=True)
    write_fastq(fq2, s2, "b", gz=True)
    bait = str(tmp_path / "Clade.fa")
    open(bait, "w").write(clade.text)
    base = [CLI, "bait", "--protein", "--bait", bait, "--code", "5", "--fq1", fq1, "--fq2", fq2]
    p0 = subprocess.run(base + ["--out1", str(tmp_path / "o1.fq"), "--out2", str(tmp_path / "o2.fq")], capture_output=True, timeout=300)
    assert p0.returncode == 0, p0.stderr.decode()[-2000:]
    rep = str(tmp_path / "genes.tsv")
    p1 = subprocess.run(base + ["--out1", str(tmp_path / "g1.fq"), "--out2", str(tmp_path / "g2.fq"), "--group-report", rep, "--group-field", "4"],
                        capture_output=True, timeout=300)
    assert p1.returncode == 0, p1.stderr.decode()[-2000:]
    assert p1.stdout == p0.stdout
    for m in ("1", "2"):
        assert open(str(tmp_path / ("g%s.fq" % m)), "rb").read() == open(str(tmp_path / ("o%s.fq" % m)), "rb").read()
    okept, oc = file_counts(Oracle(clade.text, 9, 5, "_", 4), s1, s2, 1, False)
    assert int(p1.stdout.decode()) == okept
    assert open(rep).read() == _tsv(GENES, oc)
    # records as groups (no --group-field), and an explicit separator
    p2 = subprocess.run(base + ["--out1", str(tmp_path / "h1.fq"), "--out2", str(tmp_path / "h2.fq"), "--group-report", rep], capture_output=True, timeout=300)
    assert p2.returncode == 0, p2.stderr.decode()[-2000:]
    o = Oracle(clade.text, 9, 5)
    _, oc = file_counts(o, s1, s2, 1, False)
    assert open(rep).read() == _tsv(o.names, oc)
    p3 = subprocess.run(base + ["--out1", str(tmp_path / "h1.fq"), "--out2", str(tmp_path / "h2.fq"), "--group-report", rep,
                                "--group-field", "5", "--group-sep", "_"], capture_output=True, timeout=300)
    assert p3.returncode == 0, p3.stderr.decode()[-2000:]
    o = Oracle(clade.text, 9, 5, "_", 5)
    _, oc = file_counts(o, s1, s2, 1, False)
    assert open(rep).read() == _tsv(o.names, oc)


def test_cli_group_report_nucleotide(mf, tmp_path):
    text = eight_record_bait()
    s1 = make_reads(text, 2000, seed=95)
    fq1 = str(tmp_path / "a_1.fq")
    write_fastq(fq1, s1, "a")
    bait = str(tmp_path / "bait.fa")
    open(bait, "w").write(text)
    rep = str(tmp_path / "r.tsv")
    p = subprocess.run([CLI, "bait", "--bait", bait, "-k", "31", "--fq1", fq1, "--out1", str(tmp_path / "o1.fq"), "--group-report", rep,
                        "--group-field", "1"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    o = Oracle(text, 31, None, "_", 1)
    okept, oc = file_counts(o, s1, None, 1, False)
    assert int(p.stdout.decode()) == okept
    assert open(rep).read() == _tsv(["mito", "tiny", "rec2", "rand"], oc)
