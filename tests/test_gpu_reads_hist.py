"""The k-mer histogram of ntedit-make-reads-bf on the GPU: the histogram against the count-min model of
tests/test_gpu_reads_bf.py (batching, host and device batches, the --hist file), the --solid cutoff and the filters it
gives, sizing from the histogram, polishing with a --solid filter, and one run over 3 Gbp of reads."""
import ctypes
import gzip
import json
import math
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from test_gpu_reads_bf import (HASHES, K, NTEDIT, TOOL, _missing_kmers, awkward, blob_of, kmer_hashes,
                               model_bf, model_counts, model_estimates, model_occ, model_sketch, rounded,
                               simulate_reads, write_fastq, write_large_reads)

pytestmark = pytest.mark.gpu

_ = awkward  # the module-scoped fixture, shared


# ------------------------------------------------------------------ the histogram model (and reads_model.model_occ)
def model_summary(occ):
    c = np.arange(1, 256, dtype=np.uint64)
    f = np.zeros(256, dtype=np.uint64)
    f[1:] = (occ[1:] + c // np.uint64(2)) // c
    return f, int(f.sum()), int(occ.sum())


def model_cutoff(f):
    for c in range(1, 254):
        if f[c + 1] > f[c]:
            return c
    return None


def render_hist(occ):
    f, F0, F1 = model_summary(occ)
    lines = ["F1\t%d" % F1, "F0\t%d" % F0] + ["%d\t%d" % (c, f[c]) for c in range(1, 256)]
    return ("\n".join(lines) + "\n").encode()


def get_bf_size(n, hashes=HASHES, fpr=0.01):
    """the tool's --num_elements -> bytes (the genome tool's formula)"""
    r = -hashes / math.log(1.0 - math.exp(math.log(fpr) / hashes))
    return int(math.ceil(n * r) / 8)


def run(args, timeout=600):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def logged_cutoff(r):
    m = re.findall(r"--solid: minimum k-mer count (\d+)", r.stderr)
    assert len(m) == 1, r.stderr
    return int(m[0])


# ------------------------------------------------------------------ 1. the histogram through the C ABI
def _batches(reads, nbytes):
    """reads joined by '\\n' into batches of at most nbytes (a read longer than that alone); None: one batch"""
    if nbytes is None:
        return [blob_of(reads)]
    out, cur, size = [], [], 0
    for r in reads:
        if cur and size + len(r) + 1 > nbytes:
            out.append(blob_of(cur))
            cur, size = [], 0
        cur.append(r)
        size += len(r) + 1
    if cur:
        out.append(blob_of(cur))
    return out


def lib_histogram(reads, sketch, batch_bytes, on_device):
    """pass 1 + the histogram pass through the library: (occ, sketch bytes)"""
    import torch
    import ntedit_amd
    lib = ntedit_amd._lib.load()
    pol = ntedit_amd.Polisher(0)
    h = pol._h
    err = lambda: lib.ntedit_hip_reads_last_error(h).decode()
    try:
        assert lib.ntedit_hip_sketch_alloc(h, sketch, HASHES, K) == 0, err()
        batches = _batches(reads, batch_bytes)
        for b in batches:
            assert lib.ntedit_hip_sketch_count(h, b, len(b), 0) == 0, err()
        for b in batches:
            if on_device:
                d = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                assert d.data_ptr() % 16 == 0
                rc = lib.ntedit_hip_sketch_histogram(h, ctypes.c_void_p(d.data_ptr()), len(b), 1)
                del d
            else:
                rc = lib.ntedit_hip_sketch_histogram(h, b, len(b), 0)
            assert rc == 0, err()
        occ = np.zeros(256, dtype=np.uint64)
        assert lib.ntedit_hip_sketch_histogram_download(h, occ.ctypes.data_as(ctypes.c_void_p)) == 0, err()
        sk = np.zeros(rounded(sketch), dtype=np.uint8)
        assert lib.ntedit_hip_sketch_download(h, sk.ctypes.data_as(ctypes.c_void_p)) == 0, err()
    finally:
        lib.ntedit_hip_sketch_free(h)
        pol.close()
    return occ, sk


@pytest.mark.parametrize("sketch", [1000003, 1 << 13])  # non-power-of-two; power-of-two and saturating
def test_histogram_equals_the_model_for_any_batching(awkward, sketch):
    hv = awkward["hv"]
    sk_model = model_sketch(hv, rounded(sketch))
    want = model_occ(hv, sk_model)
    assert want[0] == 0 and int(want.sum()) == len(hv)
    if sketch == 1 << 13:
        assert want[255] > 0.5 * len(hv)  # most estimates saturated
    else:
        assert want[255] > 0 and want[1] > 0 and (want[2:255] > 0).sum() > 30
    for batch_bytes in (None, 4096, 77777):
        for on_device in (0, 1):
            occ, sk = lib_histogram(awkward["reads"], sketch, batch_bytes, on_device)
            assert np.array_equal(sk, sk_model), (batch_bytes, on_device)
            assert np.array_equal(occ, want), (batch_bytes, on_device)


def test_histogram_accumulates_and_alloc_zeroes_it(awkward):
    # two histogram passes add up; a new sketch starts from zero (ntedit_hip_sketch_alloc)
    import ntedit_amd
    lib = ntedit_amd._lib.load()
    pol = ntedit_amd.Polisher(0)
    h = pol._h
    b = blob_of(awkward["reads"])
    occ = np.zeros(256, dtype=np.uint64)
    ptr = occ.ctypes.data_as(ctypes.c_void_p)
    try:
        for _ in range(2):
            assert lib.ntedit_hip_sketch_alloc(h, 1000003, HASHES, K) == 0
            assert lib.ntedit_hip_sketch_count(h, b, len(b), 0) == 0
            assert lib.ntedit_hip_sketch_histogram(h, b, len(b), 0) == 0
            assert lib.ntedit_hip_sketch_histogram(h, b, len(b), 0) == 0
            assert lib.ntedit_hip_sketch_histogram_download(h, ptr) == 0
            want = 2 * model_occ(awkward["hv"], model_sketch(awkward["hv"], rounded(1000003)))
            assert np.array_equal(occ, want)
        # an unaligned device batch is refused
        assert lib.ntedit_hip_sketch_histogram(h, ctypes.c_void_p(17), 64, 1) != 0
    finally:
        lib.ntedit_hip_sketch_free(h)
        pol.close()


# ------------------------------------------------------------------ 2. the --hist file
def test_hist_file_equals_the_model_rendering(awkward):
    d, hv = awkward["dir"], awkward["hv"]
    sketch = 1000003
    want = render_hist(model_occ(hv, model_sketch(hv, rounded(sketch))))
    write_fastq(d / "h.fq.gz", awkward["reads"], opener=gzip.open)
    for files, bb in (([awkward["fa"]], None), ([awkward["fa"]], 4096), ([d / "h.fq.gz"], 100000)):
        hist = d / "h.txt"
        extra = ["--batch_bytes", bb] if bb else []
        r = run(["--reads"] + files + ["-k", K, "-c", 2, "--bf", 1 << 15, "--sketch_bytes", sketch, "--hist", hist,
                                       "-o", d / "h.bf"] + extra)
        assert open(hist, "rb").read() == want, (files, bb)
        assert "Pass H (histogram)" in r.stderr
    lines = want.decode().splitlines()
    assert len(lines) == 257 and lines[0].startswith("F1\t") and lines[1].startswith("F0\t")


# ------------------------------------------------------------------ 3. --solid on reads with a clear valley
@pytest.fixture(scope="module")
def valley(tmp_path_factory):
    d = tmp_path_factory.mktemp("valley")
    rng = np.random.default_rng(41)
    genome = H.random_genome(rng, 200000)
    reads = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    fq = d / "reads.fq"
    write_fastq(fq, reads)
    hv = kmer_hashes(blob_of(reads))
    return dict(dir=d, reads=reads, fq=fq, hv=hv)


@pytest.mark.parametrize("counts", [False, True])
def test_solid_picks_the_model_cutoff_and_its_filter(valley, counts):
    d, hv = valley["dir"], valley["hv"]
    sketch, bf = 1 << 24, 1 << 20
    sk_model = model_sketch(hv, rounded(sketch))
    est = model_estimates(hv, sk_model)
    occ = model_occ(hv, sk_model)
    f, _, _ = model_summary(occ)
    cut = model_cutoff(f)
    assert cut is not None and 2 <= cut <= 10, f[:40]
    # a clear valley: many error k-mers below it, a coverage peak above it
    assert f[1] > 10 * f[cut] and f[cut + 1:].max() > 10 * f[cut]
    flags = ["--counts"] if counts else []
    common = ["--reads", valley["fq"], "-k", K, "--bf", bf, "--sketch_bytes", sketch] + flags
    r = run(common + ["--solid", "-o", d / "s.bf", "--hist", d / "s.txt"])
    assert logged_cutoff(r) == cut
    assert open(d / "s.txt", "rb").read() == render_hist(occ)
    run(common + ["-c", cut, "-o", d / "c.bf"])
    got = H.load_bf(str(d / "s.bf"))
    if counts:
        assert got["counting"] and np.array_equal(got["data"], model_counts(hv, est, cut, rounded(bf)))
    else:
        assert not got["counting"] and np.array_equal(got["data"], model_bf(hv, est, cut, bf))
    assert open(d / "s.bf", "rb").read() == open(d / "c.bf", "rb").read()


# ------------------------------------------------------------------ 4. sizing from the histogram
def test_solid_without_a_size_sizes_from_the_histogram(tmp_path):
    rng = np.random.default_rng(43)
    genome = H.random_genome(rng, 300000)
    reads = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    gz = tmp_path / "reads.fq.gz"
    write_fastq(gz, reads, opener=lambda p, m: gzip.open(p, m, compresslevel=0))  # stored: 4 x its size > 64 MiB
    sketch = rounded(4 * gz.stat().st_size)
    assert sketch > 64 << 20
    hv = kmer_hashes(blob_of(reads))
    sk_model = model_sketch(hv, sketch)
    f, _, _ = model_summary(model_occ(hv, sk_model))
    cut = model_cutoff(f)
    assert cut is not None and 2 <= cut <= 10
    n = int(f[cut:].sum())
    r = run(["--reads", gz, "-k", K, "--solid", "-o", tmp_path / "auto.bf", "--save_sketch", tmp_path / "sk.bf"])
    assert logged_cutoff(r) == cut
    assert "--num_elements %d " % n in r.stderr
    sk = H.load_bf(str(tmp_path / "sk.bf"))
    assert sk["bytes"] == sketch and np.array_equal(sk["data"], sk_model)
    run(["--reads", gz, "-k", K, "-c", cut, "--num_elements", n, "--sketch_bytes", sketch, "-o", tmp_path / "n.bf"])
    auto = open(tmp_path / "auto.bf", "rb").read()
    assert auto == open(tmp_path / "n.bf", "rb").read()
    got = H.load_bf(str(tmp_path / "auto.bf"))
    assert got["bytes"] == rounded(get_bf_size(n))  # (whole 64-bit words, as btllib)
    est = model_estimates(hv, sk_model)
    assert np.array_equal(got["data"], model_bf(hv, est, cut, rounded(get_bf_size(n))))


# ------------------------------------------------------------------ 5. polish with a --solid filter
@pytest.mark.parametrize("counts", [False, True])
def test_polish_with_the_solid_filter_matches_the_oracle(tmp_path, counts):
    rng = np.random.default_rng(23)
    truth = H.random_genome(rng, 200000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft)], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    write_fastq(tmp_path / "reads.fq.gz", reads, opener=gzip.open)
    # (a counting filter sized by the bits formula is mostly full: it gets the existing test's size instead)
    r = run(["--reads", tmp_path / "reads.fq.gz", "-k", K, "--solid", "-o", tmp_path / "reads.bf"] +
            (["--counts", "--bf", 1 << 20] if counts else []))
    cut = logged_cutoff(r)
    assert 2 <= cut <= 10
    args, params = [], H.default_params()
    if counts:
        args, params = ["-p", "2"], H.default_params(min_threshold=2)
    p = subprocess.run([NTEDIT, "-f", str(tmp_path / "draft.fa"), "-r", str(tmp_path / "reads.bf"), "-b",
                        str(tmp_path / "g")] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    H.run_oracle(str(tmp_path / "draft.fa"), str(tmp_path / "reads.bf"), params, str(tmp_path / "o"))
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert open(tmp_path / ("g" + suffix), "rb").read() == open(tmp_path / ("o" + suffix), "rb").read(), suffix
    edited = H.read_fasta(str(tmp_path / "g_edited.fa"))[0][1].upper()
    before, after = _missing_kmers(truth, draft), _missing_kmers(truth, edited)
    assert before > 1000 and after < (0.5 if counts else 0.3) * before, (before, after)


# ------------------------------------------------------------------ 6. full size: 100 Mbp genome at 30x
def test_large_solid_hist_run(tmp_path):
    fa = tmp_path / "large.fa"
    _, n_reads = write_large_reads(fa)
    hist = tmp_path / "large.hist"
    r = run(["--reads", fa, "-k", K, "--solid", "--hist", hist, "-o", tmp_path / "large.bf", "--save_sketch",
             tmp_path / "sk.bf"], timeout=1800)
    rates = re.findall(r"Pass ([12H]) \([^)]*\): (\d+) bases, ([\d.]+) ms, ([\d.]+) Gbases/s \(GPU calls ([\d.]+) ms, "
                       r"([\d.]+)", r.stderr)
    assert [x[0] for x in rates] == ["1", "H", "2"], r.stderr
    assert all(int(x[1]) == n_reads * 150 for x in rates), r.stderr
    cut = logged_cutoff(r)
    assert 2 <= cut <= 10, r.stderr
    text = open(hist).read().splitlines()
    head = dict(line.split("\t") for line in text[:2])
    f = np.array([0] + [int(line.split("\t")[1]) for line in text[2:]], dtype=np.uint64)
    assert int(head["F1"]) == n_reads * (150 - K + 1)
    assert model_cutoff(f) == cut
    n = int(f[cut:].sum())
    out = H.load_bf(str(tmp_path / "large.bf"))
    assert out["bytes"] == rounded(get_bf_size(n))
    sk = H.load_bf(str(tmp_path / "sk.bf"))
    assert sk["bytes"] == rounded(fa.stat().st_size)  # one counter per input byte
    print(json.dumps({"reads_bases": n_reads * 150, "cutoff": cut, "num_elements": n, "passes": [
        dict(pass_=p, ms=float(ms), gbases_per_s=float(g), gpu_ms=float(gms), gpu_gbases_per_s=float(gg))
        for p, _, ms, g, gms, gg in rates]}))
    # a sample of reads through the model: solid k-mers have all their bits in the output
    sample = []
    with open(fa, "rb") as fh:
        for i, line in enumerate(fh):
            if i % 2 and (i // 2) % 1000 == 0:
                sample.append(line.rstrip(b"\n"))
    hv = kmer_hashes(blob_of(sample))
    est = model_estimates(hv, sk["data"])
    assert (est >= 1).all()
    bits_n = out["bytes"] * 8
    slots = (hv % np.uint64(bits_n)).astype(np.int64)
    bits = (out["data"][slots >> 3] >> (slots & 7).astype(np.uint8)) & 1
    assert bits[est >= cut].all()
    assert (est >= cut).mean() > 0.5
