"""The reads kernels at every k, number of hashes and filter size the tool accepts, against the count-min model of
tests/reads_model.py, byte for byte through the C ABI:

1. every instantiation k_count<H, POW2>, k_hist<H, POW2>, k_solid<H, POW2, COUNTS> (H = 1..8) on reads with
   collisions, saturated counters and a cmin that keeps some k-mers and drops others;
2. tile and halo edges (RD_TILE = 16384 k-mer starts + a k - 1 byte halo per tile) at k = 12, 17, 200, as host and
   device batches and as one batch;
3. a sketch and both outputs past 2^32 slots (filter_slot's magic32 form), checked on the device;
4. the occupancy calls (k_nonzero, k_popcount on a counting filter), saturation at 255 and cmin 255;
5. the tool, the polisher and the sharded driver at k and h other than 25 and 3."""
import ctypes
import subprocess

import numpy as np
import pytest

import helpers as H
from reads_model import (awkward_reads, blob_of, kmer_hashes, model_bf, model_counts, model_estimates, model_occ,
                         model_sketch, rounded, simulate_reads)
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq
from test_gpu_reads_multi import _binary, _driver

pytestmark = pytest.mark.gpu

RD_TILE = 16384  # k-mer starts per block of the reads kernels (nte_reads.hip)
ALL_K = [12, 17, 25, 33, 64, 65, 128, 193, 200]


# ------------------------------------------------------------------ the C ABI
class Reads:
    """one Polisher context, its sketch and its filter slot 0, through the C ABI"""

    def __init__(self):
        import ntedit_amd
        self.lib = ntedit_amd._lib.load()
        self.pol = ntedit_amd.Polisher(0)
        self.h = self.pol._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.ntedit_hip_sketch_free(self.h)
        self.pol.close()

    def ok(self, rc, what):
        assert rc == 0, "%s: %s" % (what, self.lib.ntedit_hip_reads_last_error(self.h).decode())

    def alloc(self, counters, h, k):
        self.ok(self.lib.ntedit_hip_sketch_alloc(self.h, counters, h, k), "sketch_alloc")

    def adopt(self, t, h, k):
        self.ok(self.lib.ntedit_hip_sketch_set_device(self.h, t.data_ptr(), t.numel(), h, k), "sketch_set_device")

    def count(self, batches):
        for ptr, n, dev in batches:
            self.ok(self.lib.ntedit_hip_sketch_count(self.h, ptr, n, dev), "sketch_count")

    def hist(self, batches):
        for ptr, n, dev in batches:
            self.ok(self.lib.ntedit_hip_sketch_histogram(self.h, ptr, n, dev), "sketch_histogram")
        occ = np.zeros(256, dtype=np.uint64)
        self.ok(self.lib.ntedit_hip_sketch_histogram_download(self.h, occ.ctypes.data_as(ctypes.c_void_p)),
                "sketch_histogram_download")
        return occ

    def solid(self, batches, cmin):
        for ptr, n, dev in batches:
            self.ok(self.lib.ntedit_hip_filter_insert_solid(self.h, 0, ptr, n, dev, cmin), "filter_insert_solid")

    def sketch(self, counters):
        sk = np.zeros(counters, dtype=np.uint8)
        self.ok(self.lib.ntedit_hip_sketch_download(self.h, sk.ctypes.data_as(ctypes.c_void_p)), "sketch_download")
        return sk

    def sketch_occupancy(self):
        nz, n = ctypes.c_uint64(), ctypes.c_uint64()
        self.ok(self.lib.ntedit_hip_sketch_occupancy(self.h, ctypes.byref(nz), ctypes.byref(n)), "sketch_occupancy")
        return nz.value, n.value

    def plain(self, nbytes, h, k):
        self.pol.filter_alloc(nbytes, h, k)

    def counting(self, nbytes, h, k):
        self.ok(self.lib.ntedit_hip_filter_alloc_counting(self.h, 0, nbytes, h, k), "filter_alloc_counting")


def host_batches(blobs):
    return [(b, len(b), 0) for b in blobs]


def device_batches(blobs, keep):
    """the blobs as 16-byte aligned device buffers of exactly their length (tensors kept alive in `keep`)"""
    import torch
    out = []
    for b in blobs:
        t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        assert t.data_ptr() % 16 == 0
        keep.append(t)
        out.append((ctypes.c_void_p(t.data_ptr()), len(b), 1))
    torch.cuda.synchronize()
    return out


def run_passes(blobs, counters, h, k, cmin, plain_bytes, count_bytes, on_device):
    """pass 1, the histogram pass and pass 2 into a plain and a counting slot, in one context:
    (sketch, occ, plain, counts, sketch occupancy, counting-filter occupancy)"""
    keep = []
    with Reads() as r:
        batches = device_batches(blobs, keep) if on_device else host_batches(blobs)
        r.alloc(counters, h, k)
        r.count(batches)
        sk = r.sketch(rounded(counters))
        sk_occ = r.sketch_occupancy()
        occ = r.hist(batches)
        r.plain(plain_bytes, h, k)
        r.solid(batches, cmin)
        plain = r.pol.filter_download(0)
        r.counting(count_bytes, h, k)
        r.solid(batches, cmin)
        counts = r.pol.filter_download(0)
        c_occ = r.pol.filter_occupancy(0)
    return sk, occ, plain, counts, sk_occ, c_occ


def check_passes(got, hv, counters, cmin, plain_bytes, count_bytes):
    sk, occ, plain, counts, sk_occ, c_occ = got
    want_sk = model_sketch(hv, rounded(counters))
    est = model_estimates(hv, want_sk)
    assert np.array_equal(sk, want_sk), "sketch"
    assert sk_occ == (np.count_nonzero(want_sk), rounded(counters)), "sketch occupancy"
    assert np.array_equal(occ, model_occ(hv, want_sk)), "histogram"
    assert np.array_equal(plain, model_bf(hv, est, cmin, rounded(plain_bytes))), "plain output"
    want_counts = model_counts(hv, est, cmin, rounded(count_bytes))
    assert np.array_equal(counts, want_counts), "counting output"
    assert c_occ == (np.count_nonzero(want_counts), rounded(count_bytes)), "counting occupancy"


# ------------------------------------------------------------------ 1. every instantiation against the model
def _matrix_cases():
    cases = []
    for h in range(1, 9):
        for pow2 in (True, False):
            i = len(cases)
            k = ALL_K[i % len(ALL_K)]
            p = int(pow2)
            tid = "k_count<%d,%d>+k_hist<%d,%d>+k_solid<%d,%d,0>+k_solid<%d,%d,1>-k%d" % (h, p, h, p, h, p, h, p, k)
            cases.append(pytest.param(i, h, pow2, k, id=tid))
    return cases


MATRIX = _matrix_cases()


def matrix_data(i, h, pow2, k):
    """reads with errors, N runs, short reads and one read 300 times; a sketch of about 1.5 h counters per distinct
    k-mer (power of two or not) and two output sizes: 2^14 bytes and 100,003 bytes (rounded to whole words)"""
    # (long k-mers: fewer errors and longer reads, so that the genome's k-mers still reach cmin)
    reads = awkward_reads(k, seed=100 + i, genome_len=8000, err=0.01 if k < 100 else 0.002, length=max(150, k + 100))
    third = len(reads) // 3
    blobs = [blob_of(reads[:third]), blob_of(reads[third:2 * third]), blob_of(reads[2 * third:])]
    hv = kmer_hashes(b"".join(blobs), k, h)
    distinct = len(np.unique(hv[:, 0]))
    want = int(1.5 * h * distinct)
    counters = 1 << (want.bit_length() - 1) if pow2 else want | 1
    assert (counters & (counters - 1) == 0) == pow2 and (rounded(counters) & (rounded(counters) - 1) == 0) == pow2
    plain_bytes, count_bytes = (1 << 14, 100003) if i % 2 == 0 else (100003, 1 << 14)
    return blobs, hv, counters, plain_bytes, count_bytes


@pytest.mark.parametrize("i,h,pow2,k", MATRIX)
def test_every_instantiation_equals_the_model(i, h, pow2, k):
    blobs, hv, counters, plain_bytes, count_bytes = matrix_data(i, h, pow2, k)
    cmin = 4
    sk = model_sketch(hv, rounded(counters))
    est = model_estimates(hv, sk)
    # collisions: counters shared by distinct k-mers, saturated counters, and a cmin that keeps some distinct k-mers
    # and drops others
    u = np.unique(hv, axis=0)
    shared = np.bincount((u % np.uint64(rounded(counters))).ravel().astype(np.int64))
    assert (shared >= 2).sum() > 1000 and (sk == 255).any()
    kept = np.unique(hv[est >= cmin, 0])
    assert 0.05 * len(u) < len(kept) < 0.95 * len(u), (len(kept), len(u))
    got = run_passes(blobs, counters, h, k, cmin, plain_bytes, count_bytes, on_device=h % 2 == 0)
    check_passes(got, hv, counters, cmin, plain_bytes, count_bytes)


def test_the_matrix_covers_every_instantiation_and_k():
    triples = set()
    for p in MATRIX:
        _, h, pow2, _ = p.values
        triples |= {(h, pow2, pass_) for pass_ in ("count", "hist", "solid", "solid_counts")}
    assert len(triples) == 64
    assert {p.values[3] for p in MATRIX} == set(ALL_K)


# ------------------------------------------------------------------ 2. tile and halo edges
def _acgt(rng, n):
    r = bytearray(H.random_genome(rng, n))
    for i in rng.integers(0, max(n, 1), n // 8):
        r[i] |= 0x20
    return bytes(r)


def edge_blobs(k, seed):
    """batches that cut k-mers at every tile boundary, batch lengths around k and RD_TILE (+ the halo), breaks at
    RD_TILE - 1 and RD_TILE, break runs of 1, k - 1 and k bytes across boundaries, and reads of k - 1, k, k + 1 bytes.
    A batch ends a record (no trailing newline: its last k-mer ends at its last byte)."""
    rng = np.random.default_rng(seed)
    T = RD_TILE
    blobs = []
    long = _acgt(rng, 3 * T + 1000)  # one record, no breaks, over four tiles
    blobs.append(long)
    for n in (k - 1, k, k + 1, T - 1, T, T + 1, T + k - 1, T + k, 2 * T + 15):
        blobs.append(_acgt(rng, n))
    for at in (T - 1, T):
        b = bytearray(_acgt(rng, 2 * T + 100))
        b[at] = ord("N")
        blobs.append(bytes(b))
    b = bytearray(_acgt(rng, 3 * T + 500))
    b[T - 1] = ord("\r")  # a run of 1, and runs of k - 1 and k across the second and third tile boundaries
    b[2 * T - k // 2:2 * T - k // 2 + k - 1] = b"N" * (k - 1)
    b[3 * T - k // 2:3 * T - k // 2 + k] = b"n" * k
    blobs.append(bytes(b))
    blobs.append(blob_of([_acgt(rng, n) for n in (k - 1, k, k + 1) for _ in range(40)]))
    blobs.append(long)  # twice: its k-mers are solid at cmin 2
    return blobs


EDGES = [(12, 2, 1 << 20), (17, 7, (1 << 21) + 40), (200, 4, 3000017)]  # (k, h, sketch counters)


@pytest.mark.parametrize("k,h,counters", EDGES, ids=["k%d-h%d" % (k, h) for k, h, _ in EDGES])
def test_tile_and_halo_edges_for_every_batching(k, h, counters):
    blobs = edge_blobs(k, seed=k)
    assert {len(b) % 16 for b in blobs} - {0}  # device batches with a byte-by-byte tail
    joined = b"\n".join(blobs)
    hv = kmer_hashes(joined, k, h)
    # every batching cuts at record ends, so every one has the k-mers of the joined bytes
    assert sum(len(kmer_hashes(b, k, h)) for b in blobs) == len(hv)
    cmin, plain_bytes, count_bytes = 2, 1 << 17, 100003
    sk = model_sketch(hv, rounded(counters))
    est = model_estimates(hv, sk)
    assert (est >= cmin).any() and (est < cmin).any()
    for tag, bl, dev in (("host", blobs, False), ("device", blobs, True), ("one batch", [joined], False)):
        got = run_passes(bl, counters, h, k, cmin, plain_bytes, count_bytes, on_device=dev)
        try:
            check_passes(got, hv, counters, cmin, plain_bytes, count_bytes)
        except AssertionError as e:
            raise AssertionError("%s batches: %s" % (tag, e)) from None


# ------------------------------------------------------------------ 3. past 2^32 slots
def _nonzero(t):
    """count_nonzero of a device tensor, through 1 GiB views"""
    import torch
    step = 1 << 30
    return sum(int(torch.count_nonzero(t[i:i + step])) for i in range(0, t.numel(), step))


def _at(t, slots):
    import torch
    return t[torch.from_numpy(slots.astype(np.int64)).cuda()].cpu().numpy()


def test_sketch_and_outputs_past_2_32_slots():
    """a 2^32 + 8 counter sketch (adopted), a 600,000,008-byte plain output (4.8e9 bits) and a 2^32 + 8 byte counting
    output (adopted): none a power of two, all in filter_slot's magic32 range.  Sketch and counting output are checked
    on the device: the model's counters at its slots, and no other non-zero byte."""
    import torch
    k, h, cmin = 31, 4, 2
    reads = awkward_reads(k, seed=61)
    blob = blob_of(reads)
    hv = kmer_hashes(blob, k, h)
    assert 5e5 < len(hv) < 2e6
    counters = (1 << 32) + 8
    slots = hv % np.uint64(counters)
    u, inv, c = np.unique(slots.ravel(), return_inverse=True, return_counts=True)
    want_u = np.minimum(c, 255).astype(np.uint8)
    # (only 8 counters lie past 2^32: what this size tests is the magic32 arithmetic, at every slot)
    assert (want_u == 255).any() and (want_u == 1).any()
    est = want_u[inv.reshape(slots.shape)].min(axis=1)
    assert (est >= cmin).any() and (est < cmin).any()
    keep = est >= cmin
    with Reads() as r:
        sk = torch.zeros(counters, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.adopt(sk, h, k)
        r.count(host_batches([blob]))
        assert np.array_equal(_at(sk, u), want_u)
        assert _nonzero(sk) == len(u)
        assert r.sketch_occupancy() == (len(u), counters)
        occ = r.hist(host_batches([blob]))
        assert np.array_equal(occ, np.bincount(est, minlength=256).astype(np.uint64))
        # plain output: 4.8e9 bits
        nbytes = 600_000_008
        r.plain(nbytes, h, k)
        r.solid(host_batches([blob]), cmin)
        got = r.pol.filter_download(0)
        bits = (hv[keep] % np.uint64(nbytes * 8)).ravel()
        assert bits.max() >= 1 << 32
        want = np.zeros(nbytes, dtype=np.uint8)
        np.bitwise_or.at(want, (bits >> np.uint64(3)).astype(np.int64), (1 << (bits & np.uint64(7))).astype(np.uint8))
        assert np.array_equal(got, want)
        del got, want
        # counting output: 2^32 + 8 counters (slot 0's plain filter is freed when the tensor replaces it)
        cbytes = (1 << 32) + 8
        out = torch.zeros(cbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.pol.set_filter_device(out.data_ptr(), cbytes, h, k, slot=0, counting=True)
        r.solid(host_batches([blob]), cmin)
        cs = (hv[keep] % np.uint64(cbytes)).ravel()
        ce = np.repeat(est[keep], h)
        order = np.lexsort((ce, cs))  # by slot, then estimate: the last of each slot is its max
        cs, ce = cs[order], ce[order]
        last = np.r_[cs[1:] != cs[:-1], True]
        assert np.array_equal(_at(out, cs[last]), ce[last])
        assert _nonzero(out) == int(last.sum())
        assert r.pol.filter_occupancy(0) == (int(last.sum()), cbytes)
        r.lib.ntedit_hip_sketch_free(r.h)
        del out, sk
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. occupancy, saturation and cmin edges
@pytest.mark.parametrize("adopted", [False, True])
def test_sketch_occupancy_counts_every_nonzero_counter(adopted):
    import torch
    k, h = 25, 2
    counters = 100_008  # not a multiple of 64 (k_nonzero reads 64-bit words)
    assert counters % 64 and counters % 8 == 0
    reads = awkward_reads(k, seed=71, genome_len=2000)
    blob = blob_of(reads)
    want = model_sketch(kmer_hashes(blob, k, h), counters)
    # empty counters, saturated ones, and non-zero counters with a zero low nibble (16, 32, ...)
    assert (want == 0).any() and (want == 255).any() and ((want != 0) & (want & 0x0F == 0)).any()
    with Reads() as r:
        t = None
        if adopted:
            t = torch.zeros(counters, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.adopt(t, h, k)
        else:
            r.alloc(counters, h, k)
        r.count(host_batches([blob]))
        sk = r.sketch(counters)
        assert np.array_equal(sk, want)
        assert r.sketch_occupancy() == (np.count_nonzero(sk), counters)
        if adopted:
            assert int(torch.count_nonzero(t)) == np.count_nonzero(sk)
        # and the counting output's occupancy (k_popcount on counters)
        est = model_estimates(kmer_hashes(blob, k, h), want)
        r.counting(50_001, h, k)
        r.solid(host_batches([blob]), 2)
        c = r.pol.filter_download(0)
        assert np.array_equal(c, model_counts(kmer_hashes(blob, k, h), est, 2, rounded(50_001)))
        assert ((c != 0) & (c & 0x0F == 0)).any()
        assert r.pol.filter_occupancy(0) == (np.count_nonzero(c), rounded(50_001))


def _three_kmers(k, seed):
    rng = np.random.default_rng(seed)
    return [H.random_genome(rng, k) for _ in range(3)]


@pytest.mark.parametrize("k,h", [(33, 3), (128, 8)])
def test_estimates_254_255_256_and_cmin_255(k, h):
    """three k-mers that occur exactly 254, 255 and 256 times, each a read of k bytes, in a collision-free sketch"""
    a, b, c = _three_kmers(k, seed=k)
    blob = blob_of([a] * 254 + [b] * 255 + [c] * 256)
    hv = kmer_hashes(blob, k, h)
    assert len(hv) == 765
    counters = 1 << 20
    u = np.unique(hv, axis=0)
    assert len(u) == 3 and len(np.unique(u % np.uint64(counters))) == 3 * h  # collision-free
    sk = model_sketch(hv, counters)
    est = model_estimates(hv, sk)
    assert sorted(set(est.tolist())) == [254, 255]
    occ = model_occ(hv, sk)
    assert occ[254] == 254 and occ[255] == 511 and occ.sum() == 765
    for cmin in (254, 255):
        got = run_passes([blob], counters, h, k, cmin, 1 << 12, 4099, on_device=False)
        check_passes(got, hv, counters, cmin, 1 << 12, 4099)
        plain = got[2]
        kept = np.unique(hv[est >= cmin], axis=0)
        assert len(kept) == (3 if cmin == 254 else 2)
        n_bits = int(np.unpackbits(plain).sum())
        assert 0 < n_bits <= len(kept) * h


@pytest.mark.parametrize("k,h", [(33, 3), (200, 8)])
def test_eight_counter_sketch_makes_every_kmer_solid_at_255(k, h):
    reads = awkward_reads(k, seed=80 + k, genome_len=3000, length=max(150, k + 60))
    reads += [blob_of(_three_kmers(k, seed=k))[:-1]]
    blob = blob_of(reads)
    hv = kmer_hashes(blob, k, h)
    sk = model_sketch(hv, 8)
    assert (sk == 255).all()
    est = model_estimates(hv, sk)
    assert (est == 255).all()
    got = run_passes([blob], 8, h, k, 255, 1 << 14, 100003, on_device=True)
    check_passes(got, hv, 8, 255, 1 << 14, 100003)
    assert got[4] == (8, 8)


# ------------------------------------------------------------------ 5. the tool and its consumers at other k and h
def _tool(args, timeout=600):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("k,h", [(12, 1), (64, 5), (200, 8)])
def test_tool_at_cmin_1_equals_mkbf(tmp_path, k, h):
    reads = awkward_reads(k, seed=90 + k, genome_len=20000, length=max(150, k + 60))
    fa = tmp_path / "r.fa"
    write_fasta(fa, reads)
    bf = 100003
    _tool(["--reads", fa, "-k", k, "--hashes", h, "-c", 1, "--bf", bf, "--sketch_bytes", 1 << 20, "-o",
           tmp_path / "t.bf"])
    H.mkbf([str(fa)], str(tmp_path / "mk.bf"), k=k, hashes=h, nbytes=bf)
    got = (tmp_path / "t.bf").read_bytes()
    assert got == (tmp_path / "mk.bf").read_bytes()
    meta = H.load_bf(str(tmp_path / "t.bf"))
    assert (meta["k"], meta["hash_num"], meta["bytes"]) == (k, h, rounded(bf))
    hv = kmer_hashes(blob_of(reads), k, h)
    assert np.array_equal(meta["data"], model_bf(hv, np.ones(len(hv), dtype=np.uint8), 1, rounded(bf)))


def test_polish_with_a_k40_h5_reads_filter_matches_the_oracle(tmp_path):
    k, h = 40, 5
    rng = np.random.default_rng(31)
    truth = H.random_genome(rng, 100000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft)], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    write_fastq(tmp_path / "reads.fq", reads)
    _tool(["--reads", tmp_path / "reads.fq", "-k", k, "--hashes", h, "-c", 2, "--bf", 1 << 19, "--sketch_bytes",
           1 << 23, "-o", tmp_path / "reads.bf"])
    meta = H.load_bf(str(tmp_path / "reads.bf"))
    assert (meta["k"], meta["hash_num"]) == (k, h)
    p = subprocess.run([NTEDIT, "-f", str(tmp_path / "draft.fa"), "-r", str(tmp_path / "reads.bf"), "-b",
                        str(tmp_path / "g")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    H.run_oracle(str(tmp_path / "draft.fa"), str(tmp_path / "reads.bf"), H.default_params(), str(tmp_path / "o"))
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert (tmp_path / ("g" + suffix)).read_bytes() == (tmp_path / ("o" + suffix)).read_bytes(), suffix
    edits = (tmp_path / "g_changes.tsv").read_text().splitlines()
    assert len(edits) > 20, len(edits)


def test_sharded_driver_at_k64_h5_equals_the_binary(tmp_path):
    rng = np.random.default_rng(37)
    genome = H.random_genome(rng, 60000)
    reads = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    for i in range(0, len(reads), 29):
        reads[i] = reads[i][:70].lower() + b"NN" + reads[i][72:]
    half = len(reads) // 2
    fq, fa = tmp_path / "a.fq", tmp_path / "b.fa"
    write_fastq(fq, reads[:half] + [reads[5]] * 300)
    write_fasta(fa, reads[half:])
    args = ["--reads", str(fq), str(fa), "-k", "64", "--hashes", "5", "-c", "3", "--bf", str(100003),
            "--sketch_bytes", str(1000003)]
    for counts in ([], ["--counts"]):
        ref, out = tmp_path / "ref.bf", tmp_path / "drv.bf"
        r = _binary(args + counts + ["-o", str(ref)])
        assert r.returncode == 0, r.stderr
        r = _driver(2, args + counts + ["-o", str(out)], "gloo")
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
        assert r.stderr.count("Pass 1 (count)") == 2
        assert out.read_bytes() == ref.read_bytes(), counts
        meta = H.load_bf(str(ref))
        assert (meta["k"], meta["hash_num"], meta["counting"]) == (64, 5, bool(counts))
