"""ntedit-make-reads-bf on the GPU: the sketch and both outputs against a count-min model computed here, anchors against
the oracle (mkbf, mkbf -C) and ntedit-make-genome-bf, input forms and batching, polishing with the filter it builds,
and one run over 3 Gbp of reads."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import reads_model
from reads_model import (M64, blob_of, model_bf, model_counts, model_estimates, model_occ, model_sketch,  # noqa: F401
                         rounded, simulate_reads)

pytestmark = pytest.mark.gpu

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
GENOME_TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-genome-bf")
NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
K, HASHES = 25, 3


# ------------------------------------------------------------------ the model (reads_model.py) at this k and h
def kmer_hashes(blob, k=K, h=HASHES):
    return reads_model.kmer_hashes(blob, k, h)


def test_model_hashes_match_the_oracle():
    import ctypes
    lib = H.oracle_lib()
    lib.ora_extend_hashes.argtypes = [ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint64)]
    lib.ora_extend_hashes.restype = None
    rng = np.random.default_rng(3)
    seq = bytearray(H.random_genome(rng, 400))
    for i in rng.integers(0, 400, 40):
        seq[i] |= 0x20  # lowercase hashes like uppercase
    seq = bytes(seq)
    hv = kmer_hashes(seq)
    assert len(hv) == 400 - K + 1
    up = seq.upper()
    fh = lib.ora_base_forward_hash(up, K)
    rh = lib.ora_base_reverse_hash(up, K)
    buf = (ctypes.c_uint64 * HASHES)()
    for p in range(len(hv)):
        if p:
            fh = lib.ora_next_forward_hash(fh, K, up[p - 1], up[p + K - 1])
            rh = lib.ora_next_reverse_hash(rh, K, up[p - 1], up[p + K - 1])
        lib.ora_extend_hashes((fh + rh) & M64, K, HASHES, buf)
        assert list(hv[p]) == list(buf), p


# ------------------------------------------------------------------ fixtures
def awkward_reads(seed=17, genome_len=40000, err=0.01):
    return reads_model.awkward_reads(K, seed=seed, genome_len=genome_len, err=err)


def write_fasta(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))


def write_fastq(path, reads, opener=open):
    with opener(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def run_tool(reads_files, out, cmin=2, bf=1 << 16, sketch=None, counts=False, extra=(), timeout=600):
    cmd = [TOOL, "--reads"] + [str(x) for x in reads_files] + ["-k", str(K), "-c", str(cmin), "--bf", str(bf),
                                                               "-o", str(out)]
    if sketch:
        cmd += ["--sketch_bytes", str(sketch)]
    if counts:
        cmd += ["--counts"]
    cmd += list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.fixture(scope="module")
def awkward(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    reads = awkward_reads()
    fa = d / "reads.fa"
    write_fasta(fa, reads)
    hv = kmer_hashes(blob_of(reads))
    assert 5e5 < len(hv) < 2e6
    return dict(dir=d, reads=reads, fa=fa, hv=hv)


# ------------------------------------------------------------------ 1. model equality, with collisions
@pytest.mark.parametrize("sketch", [1000003, 1 << 20])  # non-power-of-two and power-of-two sizes
def test_sketch_and_outputs_equal_the_count_min_model(awkward, sketch):
    d, hv = awkward["dir"], awkward["hv"]
    bf = 1 << 15
    sk_model = model_sketch(hv, rounded(sketch))
    est = model_estimates(hv, sk_model)
    # saturated counters (the read repeated 300 times), >= 100k counters shared by distinct k-mers, and cmin 2 / 3
    # keeping fewer distinct k-mers than cmin 1 (the error k-mers) but more than cmin 5
    shared = np.bincount((np.unique(hv, axis=0) % np.uint64(rounded(sketch))).ravel().astype(np.int64))
    assert (sk_model == 255).any() and (shared >= 2).sum() > 100000
    kept = [len(np.unique(hv[est >= c, 0])) for c in (1, 2, 3, 5)]
    assert kept[0] > 3 * kept[1] and kept[1] > kept[2] > kept[3], kept
    for cmin in (1, 2, 3, 5):
        out = d / ("o%d_%d.bf" % (sketch, cmin))
        sk_path = d / ("s%d_%d.bf" % (sketch, cmin))
        run_tool([awkward["fa"]], out, cmin=cmin, bf=bf, sketch=sketch, extra=["--save_sketch", str(sk_path)])
        sk = H.load_bf(str(sk_path))
        assert sk["counting"] and sk["bytes"] == rounded(sketch) and sk["hash_num"] == HASHES and sk["k"] == K
        assert np.array_equal(sk["data"], sk_model)
        got = H.load_bf(str(out))
        assert not got["counting"] and got["bytes"] == bf
        assert np.array_equal(got["data"], model_bf(hv, est, cmin, bf)), cmin
    cbf = 100003
    out = d / ("c%d.bf" % sketch)
    run_tool([awkward["fa"]], out, cmin=2, bf=cbf, sketch=sketch, counts=True)
    got = H.load_bf(str(out))
    assert got["counting"] and got["bytes"] == rounded(cbf)
    want = model_counts(hv, est, 2, rounded(cbf))
    assert np.array_equal(got["data"], want)
    # every solid k-mer's counters are >= its estimate
    keep = est >= 2
    assert (got["data"][(hv[keep] % np.uint64(rounded(cbf))).astype(np.int64)].min(axis=1) >= est[keep]).all()


# ------------------------------------------------------------------ 2. oracle anchors
def test_cmin_1_equals_mkbf_and_the_genome_tool(awkward):
    d = awkward["dir"]
    bf = 1 << 17
    run_tool([awkward["fa"]], d / "c1.bf", cmin=1, bf=bf, sketch=1 << 20)
    H.mkbf([str(awkward["fa"])], str(d / "mk.bf"), k=K, hashes=HASHES, nbytes=bf)
    r = subprocess.run([GENOME_TOOL, "--genome", str(awkward["fa"]), "-k", str(K), "--bf", str(bf), "-o",
                        str(d / "g.bf")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a = open(d / "c1.bf", "rb").read()
    assert a == open(d / "mk.bf", "rb").read()
    assert a == open(d / "g.bf", "rb").read()


def test_collision_free_sketch_equals_conservative_counting(tmp_path):
    # a read set small enough (~1500 distinct k-mers) for 64 Mi counters to hold without any shared counter
    reads = awkward_reads(seed=29, genome_len=600, err=0.002)
    fa = tmp_path / "small.fa"
    write_fasta(fa, reads)
    hv = kmer_hashes(blob_of(reads))
    sketch = (1 << 26) + 40
    distinct = np.unique(hv % np.uint64(rounded(sketch)), axis=0)
    # collision-free: no counter is shared by two distinct k-mers (nor twice by one)
    assert len(np.unique(distinct.ravel())) == distinct.size
    sk_model = model_sketch(hv, rounded(sketch))
    assert (sk_model == 255).any() and (sk_model == 1).any()
    run_tool([fa], tmp_path / "x.bf", cmin=2, bf=1 << 12, sketch=sketch, extra=["--save_sketch", str(tmp_path / "xs.bf")])
    H.mkbf([str(fa)], str(tmp_path / "cons.bf"), k=K, hashes=HASHES, nbytes=sketch, counting=True)
    assert open(tmp_path / "xs.bf", "rb").read() == open(tmp_path / "cons.bf", "rb").read()


def test_small_sketch_dominates_conservative_counting(awkward):
    d = awkward["dir"]
    sketch = 50000
    run_tool([awkward["fa"]], d / "y.bf", cmin=2, bf=1 << 12, sketch=sketch, extra=["--save_sketch", str(d / "ys.bf")])
    H.mkbf([str(awkward["fa"])], str(d / "cons_s.bf"), k=K, hashes=HASHES, nbytes=sketch, counting=True)
    cm, cons = H.load_bf(str(d / "ys.bf"))["data"], H.load_bf(str(d / "cons_s.bf"))["data"]
    assert (cm >= cons).all() and (cm > cons).any()


# ------------------------------------------------------------------ 3. input forms and batching
def test_input_forms_and_batching_give_identical_bytes(awkward):
    d, reads = awkward["dir"], awkward["reads"]
    write_fastq(d / "r.fq", reads)
    write_fastq(d / "r.fq.gz", reads, opener=gzip.open)
    third = len(reads) // 3
    parts = [reads[:third], reads[third:2 * third], reads[2 * third:]]
    for i, p in enumerate(parts):
        write_fastq(d / ("p%d.fq" % i), p)
    for counts in (False, True):
        runs = {
            "fa": [awkward["fa"]], "fq": [d / "r.fq"], "gz": [d / "r.fq.gz"],
            "split": [d / ("p%d.fq" % i) for i in range(3)],
        }
        outs = {}
        for tag, files in runs.items():
            out = d / ("f_%s_%d.bf" % (tag, counts))
            run_tool(files, out, cmin=3, bf=50000, sketch=70000, counts=counts)
            outs[tag] = open(out, "rb").read()
        out = d / ("f_small_%d.bf" % counts)
        run_tool([d / "r.fq.gz"], out, cmin=3, bf=50000, sketch=70000, counts=counts, extra=["--batch_bytes", "4096"])
        outs["small batches"] = open(out, "rb").read()
        run_tool([awkward["fa"]], d / "again.bf", cmin=3, bf=50000, sketch=70000, counts=counts)
        outs["again"] = open(d / "again.bf", "rb").read()
        for tag, b in outs.items():
            assert b == outs["fa"], (tag, counts)


# ------------------------------------------------------------------ 4. end to end: polish with the reads filter
def _missing_kmers(truth, seq, k=K):
    t = {truth[i:i + k] for i in range(len(truth) - k + 1)}
    s = {seq[i:i + k] for i in range(len(seq) - k + 1)}
    return len(t - s)


@pytest.mark.parametrize("counts", [False, True])
def test_polish_with_the_reads_filter_matches_the_oracle(tmp_path, counts):
    rng = np.random.default_rng(23)
    truth = H.random_genome(rng, 200000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft)], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    write_fastq(tmp_path / "reads.fq.gz", reads, opener=gzip.open)
    run_tool([tmp_path / "reads.fq.gz"], tmp_path / "reads.bf", cmin=2, bf=1 << 20, sketch=1 << 24, counts=counts)
    args, params = [], H.default_params()
    if counts:
        args, params = ["-p", "2"], H.default_params(min_threshold=2)
    r = subprocess.run([NTEDIT, "-f", str(tmp_path / "draft.fa"), "-r", str(tmp_path / "reads.bf"), "-b",
                        str(tmp_path / "g")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    H.run_oracle(str(tmp_path / "draft.fa"), str(tmp_path / "reads.bf"), params, str(tmp_path / "o"))
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert open(tmp_path / ("g" + suffix), "rb").read() == open(tmp_path / ("o" + suffix), "rb").read(), suffix
    edited = H.read_fasta(str(tmp_path / "g_edited.fa"))[0][1].upper()
    before, after = _missing_kmers(truth, draft), _missing_kmers(truth, edited)
    # (measured: 12355 truth k-mers missing from the draft; -p 2 on the counting filter leaves 5325 of them, the plain
    # filter fewer: the oracle, given the same filter, makes exactly the same edits in both cases)
    assert before > 1000 and after < (0.5 if counts else 0.3) * before, (before, after)


# ------------------------------------------------------------------ 5. one larger run: 100 Mbp genome at 30x
def write_large_reads(path, genome_len=100_000_000, coverage=30, length=150, seed=5, chunk=1_000_000):
    """3 Gbp of 150-bp reads with 1 % errors as FASTA; returns (genome, number of reads)"""
    rng = np.random.default_rng(seed)
    genome = H.random_genome(rng, genome_len)
    g = np.frombuffer(genome, dtype=np.uint8)
    n = genome_len * coverage // length
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        done = 0
        while done < n:
            m = min(chunk, n - done)
            starts = rng.integers(0, genome_len - length, m)
            rows = np.empty((m, length + 4), dtype=np.uint8)
            rows[:, 0], rows[:, 1], rows[:, 2] = ord(">"), ord("r"), ord("\n")
            rows[:, 3:3 + length] = g[starts[:, None] + np.arange(length)]
            e = rng.random((m, length)) < 0.01
            body = rows[:, 3:3 + length]
            body[e] = acgt[rng.integers(0, 4, int(e.sum()))]
            rows[:, -1] = ord("\n")
            f.write(rows.tobytes())
            done += m
    return genome, n


def test_large_run_against_the_model_on_a_sample(tmp_path):
    fa = tmp_path / "large.fa"
    _, n_reads = write_large_reads(fa)
    sketch, bf, cmin = 1 << 32, 200_000_000, 3
    r = run_tool([fa], tmp_path / "large.bf", cmin=cmin, bf=bf, sketch=sketch,
                 extra=["--save_sketch", str(tmp_path / "sk.bf")], timeout=1800)
    rates = re.findall(r"Pass (\d) \([^)]*\): (\d+) bases, ([\d.]+) ms, ([\d.]+) Gbases/s \(GPU calls ([\d.]+) ms, ([\d.]+)", r.stderr)
    assert len(rates) == 2 and all(int(x[1]) == n_reads * 150 for x in rates), r.stderr
    print(json.dumps({"reads_bases": n_reads * 150, "passes": [
        dict(pass_=int(p), ms=float(ms), gbases_per_s=float(g), gpu_ms=float(gms), gpu_gbases_per_s=float(gg))
        for p, _, ms, g, gms, gg in rates]}))
    sk = H.load_bf(str(tmp_path / "sk.bf"))["data"]
    n_kmers = n_reads * (150 - K + 1)
    total = int(sk.sum(dtype=np.uint64))
    saturated = int((sk == 255).sum())
    # every occurrence adds 1 to each of its h counters: exact unless a counter saturated
    if saturated == 0:
        assert total == HASHES * n_kmers
    else:
        assert total < HASHES * n_kmers
    # a sample of reads through the model: solid k-mers have all their bits in the output
    out = H.load_bf(str(tmp_path / "large.bf"))["data"]
    sample = []
    with open(fa, "rb") as f:
        for i, line in enumerate(f):
            if i % 2 and (i // 2) % 1000 == 0:
                sample.append(line.rstrip(b"\n"))
    hv = kmer_hashes(blob_of(sample))
    est = sk[(hv % np.uint64(len(sk))).astype(np.int64)].min(axis=1)
    assert (est >= 1).all()
    slots = (hv % np.uint64(bf * 8)).astype(np.int64)
    bits = (out[slots >> 3] >> (slots & 7).astype(np.uint8)) & 1
    assert bits[est >= cmin].all()
    assert (est >= cmin).mean() > 0.5
