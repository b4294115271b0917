"""The k-mer QV counts (NTEDIT_HIP_APPLY_QV, `ntedit --qv`): per entry the k-mer starts and the absent k-mers, before
and after the polish, against a CPU model -- numpy for the k-mer starts, the oracle's screening for the absent ones, on
the draft and on the oracle's edited sequences.  All counts are integers and must be equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from test_gpu_reads_cascade import case as cascade_case  # noqa: F401  (the small read set of that file, built once here)

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
FIELDS = ("len_before", "len_after", "kmers_before", "absent_before", "kmers_after", "absent_after")


def _hip_params(**kw):
    import ntedit_amd
    return ntedit_amd.default_params(**kw)


def model_counts(seqs, bf, k, p=1):
    """[(kmers, absent)] per sequence: runs of ACGTacgt of length L >= k hold L - k + 1 starts; absent = the set bits of
    the oracle's screening of the batch among the sequence's own starts"""
    blob, offs, lens, _ = H.pack_batch([(b"s", s) for s in seqs])
    bits = np.unpackbits(H.oracle_screen(blob, bf, min_threshold=p).view(np.uint8), bitorder="little")
    table = np.zeros(256, dtype=bool)
    table[list(b"ACGTacgt")] = True
    out = []
    for s, o, l in zip(seqs, offs, lens):
        good = np.concatenate(([False], table[np.frombuffer(s, dtype=np.uint8)], [False]))
        edges = np.flatnonzero(good[1:] != good[:-1])
        runs = edges[1::2] - edges[0::2]
        kmers = int(np.maximum(runs - k + 1, 0).sum())
        n_starts = max(int(l) - k + 1, 0)
        out.append((kmers, int(bits[int(o):int(o) + n_starts].sum())))
    return out


def check_counts(tmp, recs, bf_path, rep=None, **par_kw):
    """Result.qv() of recs against the model on the draft and on the oracle's edited sequences; returns (rows, names)"""
    import ntedit_amd
    hp = H.default_params(**par_kw)
    draft = os.path.join(str(tmp), "qv_draft.fa")
    H.write_fasta(draft, recs)
    H.run_oracle(draft, bf_path, hp, os.path.join(str(tmp), "qv_o"), rep)
    bf = H.load_bf(bf_path)
    k, p = bf["k"], (hp.min_threshold if bf["counting"] else 1)
    kept = [(n, s) for n, s in recs if len(s) >= hp.min_contig_len]
    edited = [s for _, s in H.read_fasta(os.path.join(str(tmp), "qv_o_edited.fa"))]
    assert len(edited) == len(kept)
    before = model_counts([s for _, s in kept], bf, k, p)
    after = model_counts(edited, bf, k, p)
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(bf_path, 0)
        if rep:
            pol.load_filter_file(rep, 1)
        pol.set_params(_hip_params(**par_kw))
        pol.set_apply(ntedit_amd.APPLY_QV)
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, hp.min_contig_len)
        res = pol.polish_batch(blob, offs, lens)
        rows = res.qv(len(names))
        st = res.stats()
        with pytest.raises(ntedit_amd.NtEditHipError):
            res.edited(len(names))  # (APPLY_QV alone keeps no edited bases)
        res.free()
    finally:
        pol.close()
    want = np.array([(len(s), len(e), b[0], b[1], a[0], a[1]) for (_, s), e, b, a in zip(kept, edited, before, after)],
                    dtype=np.uint64).reshape(-1, 6)
    got = np.stack([rows[f] for f in FIELDS], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "entry %d (%s): got %s, want %s (%d entries differ)" % (
        bad[0], names[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist(), bad.size)
    assert (got.sum(axis=0) == want.sum(axis=0)).all()
    if not hp.snv:  # (with -s 1 step 1 marks every k-mer; the QV counts are those of the plain screening)
        assert int(rows["absent_before"].sum()) == st.absent_kmers  # (the batch's own count of step 1)
    return rows, names


def test_counts_make_case(tmp_path, oracle_build):
    case = H.make_case(str(tmp_path), 32001, flavor="N lower")
    rows, _ = check_counts(tmp_path, H.read_fasta(case["draft"]), case["bf"])
    # sanity on truth: the polish removes absent k-mers
    assert rows["absent_after"].sum() < rows["absent_before"].sum()


def test_counts_many_contigs(tmp_path, oracle_build):
    case = H.make_many_case(str(tmp_path))
    rows, _ = check_counts(tmp_path, H.read_fasta(case["draft"]), case["bf"])
    assert rows.size >= 2900


@pytest.mark.parametrize("name", ["counting_p2", "snv_mode"])
def test_counts_golden(tmp_path, oracle_build, name):
    import test_golden as TG
    d = os.path.join(H.GOLDEN, "cases", name)
    hp = TG.params_from_file(os.path.join(d, "params.txt"))
    kw = {f[0]: getattr(hp, f[0]) for f in hp._fields_}
    if name == "counting_p2":
        assert hp.min_threshold == 2 and H.load_bf(os.path.join(d, "filter.bf"))["counting"]
    check_counts(tmp_path, H.read_fasta(os.path.join(d, "draft.fa")), os.path.join(d, "filter.bf"), **kw)


def test_counts_tiny_contigs_sharing_bitmap_words(tmp_path, oracle_build):
    """every contig shorter than 64 bases (-z k - 1), so that every contig shares its first bitmap word with its
    neighbour: N runs, lower-case stretches, contigs of k - 1, k and 2k - 1 bases"""
    k = 25
    rng = np.random.default_rng(5150)
    truth = H.random_genome(rng, 50000)
    H.write_fasta(os.path.join(str(tmp_path), "truth.fa"), [(b"t", truth)])
    bf = os.path.join(str(tmp_path), "t.bf")
    H.mkbf([os.path.join(str(tmp_path), "truth.fa")], bf, k=k, hashes=3, nbytes=1 << 17)
    recs = []
    for i in range(400):
        L = (k - 1, k, 2 * k - 1)[i % 3] if i % 4 == 0 else int(rng.integers(k - 1, 64))
        st = int(rng.integers(0, len(truth) - L))
        d = bytearray(truth[st:st + L])
        if i % 2:
            q = int(rng.integers(0, L))
            d[q] = b"ACGT"[(b"ACGT".index(d[q]) + 1) % 4]
        if i % 5 == 0:
            q, r = int(rng.integers(0, L - 3)), int(rng.integers(1, 4))
            d[q:q + r] = b"N" * r
        if i % 7 == 0:
            q = int(rng.integers(0, L - 10))
            d[q:q + 10] = bytes(d[q:q + 10]).lower()
        recs.append((b"tiny%d" % i, bytes(d)))
    assert all(len(s) < 64 for _, s in recs) and {k - 1, k, 2 * k - 1} <= {len(s) for _, s in recs}
    rows, _ = check_counts(tmp_path, recs, bf, min_contig_len=k - 1)
    assert rows.size == len(recs)
    assert (rows["kmers_before"][[i for i, (_, s) in enumerate(recs) if len(s) == k - 1]] == 0).all()


def test_truth_has_no_absent_kmer(tmp_path, oracle_build):
    """a draft equal to the sequence the filter was built from: all four absent counts are 0, the QV prints inf"""
    import ntedit_amd
    case = H.make_case(str(tmp_path), 32002)
    recs = H.read_fasta(case["truth"])
    rows, names = check_counts(tmp_path, recs, case["bf"])
    assert rows["absent_before"].sum() == 0 and rows["absent_after"].sum() == 0
    assert (rows["kmers_before"] == rows["len_before"] - 24).all()
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(case["bf"], 0)
        pol.write_qv_table(str(tmp_path / "t_qv.tsv"), names, rows)
    finally:
        pol.close()
    lines = open(str(tmp_path / "t_qv.tsv")).read().splitlines()
    assert lines[-1].startswith("#total\t") and len(lines) == len(names) + 2
    for line in lines[1:]:
        cols = line.split("\t")
        assert cols[5] == "inf" and cols[8] == "inf"


# ---------------------------------------------------------------------------------------------------------- CLI
def _run(cmd, cwd=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _table(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["name", "len_before", "len_after", "kmers_before", "absent_before", "qv_before",
                                    "kmers_after", "absent_after", "qv_after"]
    return [l.split("\t") for l in lines[1:]]


def _strip_times(text):
    """standard output without the wall-clock stamps behind the stage lines"""
    return [l.split(" : ")[0] if l.startswith("----------") else l for l in text.splitlines()]


def test_cli_qv(tmp_path, oracle_build):
    import ntedit_amd
    case = H.make_case(str(tmp_path), 32003, flavor="N lower")
    plain = _run([NTEDIT, "-f", case["draft"], "-r", case["bf"], "-b", tmp_path / "plain"])
    with_qv = _run([NTEDIT, "-f", case["draft"], "-r", case["bf"], "-b", tmp_path / "qv", "--qv"])
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert open(str(tmp_path / ("plain" + suffix)), "rb").read() == open(str(tmp_path / ("qv" + suffix)), "rb").read()
    assert not os.path.exists(str(tmp_path / "plain_qv.tsv"))
    a, b = _strip_times(plain.stdout.replace(str(tmp_path / "plain"), "P")), _strip_times(with_qv.stdout.replace(str(tmp_path / "qv"), "P"))
    extra = [l for l in b if l not in a]
    assert len(b) == len(a) + 1 and len(extra) == 1, (a, b)
    assert extra[0].startswith("k-mer QV (k=25): before ") and "undercount" in extra[0] and "false-positive rate" in extra[0]
    # the rows equal the ABI's
    recs = H.read_fasta(case["draft"])
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(case["bf"], 0)
        pol.set_params(_hip_params())
        pol.polish_records(recs, str(tmp_path / "py"), qv=True)
        pol.set_apply(ntedit_amd.APPLY_QV)
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, pol.params.min_contig_len)
        res = pol.polish_batch(blob, offs, lens)
        rows = res.qv(len(names))
        res.free()
        qv_of = pol.qv_value
        table = _table(str(tmp_path / "qv_qv.tsv"))
        assert open(str(tmp_path / "py_qv.tsv")).read() == open(str(tmp_path / "qv_qv.tsv")).read()
        assert [r[0].encode() for r in table[:-1]] == names and table[-1][0] == "#total"
        for r, row in zip(table[:-1], rows):
            assert [int(r[i]) for i in (1, 2, 3, 4, 6, 7)] == [int(row[f]) for f in FIELDS]
            for col, (ab, km) in ((5, (row["absent_before"], row["kmers_before"])), (8, (row["absent_after"], row["kmers_after"]))):
                q = qv_of(ab, km, 25)
                assert r[col] == ("NA" if q != q else "inf" if q == float("inf") else "%.2f" % q)
        total = table[-1]
        for i in (1, 2, 3, 4, 6, 7):
            assert int(total[i]) == sum(int(r[i]) for r in table[:-1])
        assert total[5] == "%.2f" % qv_of(int(total[4]), int(total[3]), 25)
    finally:
        pol.close()


def test_cli_qv_cascade(tmp_path, cascade_case):
    """`--reads -k 31,25 --qv`: a table per round, under that round's prefix, against that round's filter"""
    prefix = tmp_path / "casc"
    r = _run([NTEDIT, "-f", cascade_case["draft"], "--reads", *cascade_case["files"]["plain"], "-k", "31,25", "--cutoff", 2,
              "--bf", 1 << 20, "-b", prefix, "--qv"])
    first, last = _table(str(prefix) + "_k31_qv.tsv"), _table(str(prefix) + "_qv.tsv")
    assert first[-1][0] == "#total" and last[-1][0] == "#total" and len(first) == len(last)
    # round 2 polishes round 1's _edited.fa: its lengths before are round 1's lengths after
    assert [row[1] for row in last[:-1]] == [row[2] for row in first[:-1]]
    assert r.stdout.count("k-mer QV (k=31)") == 1 and r.stdout.count("k-mer QV (k=25)") == 1
