"""The sharded reads filter build on the GPU: k_merge against numpy, shards counted in separate contexts and merged
against one context and the count-min model, and the driver (python -m ntedit_amd.make_reads) byte for byte against
ntedit-make-reads-bf at world 1 over RCCL and at worlds 2 and 3 over gloo on one GPU.  Every subprocess runs under a
timeout; the driver runs start at most 3 processes that hold the GPU."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from test_gpu_reads_bf import (HASHES, K, TOOL, awkward, blob_of, kmer_hashes, model_bf, model_counts, model_estimates,
                               model_sketch, rounded, simulate_reads, write_fasta, write_fastq)

pytestmark = pytest.mark.gpu

_ = awkward  # the module-scoped fixture, shared
SAT, OR, MAX = 0, 1, 2


# ------------------------------------------------------------------ 1. k_merge
def _numpy_merge(chunks, op):
    if op == SAT:
        return np.minimum(chunks.astype(np.int64).sum(axis=0), 255).astype(np.uint8)
    return np.bitwise_or.reduce(chunks, axis=0) if op == OR else chunks.max(axis=0)


@pytest.mark.parametrize("op", [SAT, OR, MAX])
def test_merge_against_numpy(op):
    import torch
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    lib, h = pol._lib, pol._h
    rng = np.random.default_rng(7 + op)
    try:
        for n in (1, 15, 16, 17, 2 << 20, (3 << 20) + 3):
            for n_src in range(1, 8):
                if op == SAT:  # dense near the top: most sums saturate, some do not
                    chunks = rng.integers(200, 256, (n_src, n), dtype=np.uint8)
                    chunks[:, ::7] = rng.integers(0, 40, chunks[:, ::7].shape, dtype=np.uint8)
                else:
                    chunks = rng.integers(0, 256, (n_src, n), dtype=np.uint8)
                srcs = torch.from_numpy(chunks.reshape(-1).copy()).cuda()
                dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert lib.ntedit_hip_merge_bytes(h, dst.data_ptr(), srcs.data_ptr(), n_src, n, op) == 0, \
                    lib.ntedit_hip_reads_last_error(h)
                got = dst.cpu().numpy()
                assert np.array_equal(got[:n], _numpy_merge(chunks, op)), (n, n_src)
                assert (got[n:] == 0xA5).all(), (n, n_src)  # nothing past n
                # in place, into the first chunk
                assert lib.ntedit_hip_merge_bytes(h, srcs.data_ptr(), srcs.data_ptr(), n_src, n, op) == 0
                assert np.array_equal(srcs.cpu().numpy()[:n], _numpy_merge(chunks, op)), (n, n_src)
                if n_src > 1:
                    assert np.array_equal(srcs.cpu().numpy()[n:], chunks[1:].reshape(-1))
    finally:
        pol.close()


def test_merge_refuses_bad_arguments():
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    try:
        lib, h = pol._lib, pol._h
        assert lib.ntedit_hip_merge_bytes(h, None, None, 1, 16, 0) != 0
        assert lib.ntedit_hip_merge_bytes(None, None, None, 1, 16, 0) != 0
        host = (ctypes.c_uint8 * 32)()
        assert lib.ntedit_hip_merge_bytes(h, ctypes.addressof(host), ctypes.addressof(host), 1, 16, 3) != 0
    finally:
        pol.close()


# ------------------------------------------------------------------ 2. shards in separate contexts = one context
def _ctx_with_sketch(torch, counters, lib):
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    t = torch.zeros(counters, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.ntedit_hip_sketch_set_device(pol._h, t.data_ptr(), counters, HASHES, K) == 0, \
        lib.ntedit_hip_reads_last_error(pol._h)
    return pol, t


def _occ(lib, h):
    occ = np.zeros(256, dtype=np.uint64)
    assert lib.ntedit_hip_sketch_histogram_download(h, occ.ctypes.data_as(ctypes.c_void_p)) == 0
    return occ


@pytest.mark.parametrize("sketch", [1000003, 1 << 14])  # collisions; most counters saturate in every shard
def test_shards_merged_equal_one_context_and_the_model(awkward, sketch):
    import torch
    import ntedit_amd
    lib = ntedit_amd._lib.load()
    reads = awkward["reads"] + [awkward["reads"][3]] * 600  # 900 copies of one read: 300 per shard, past 255
    shards = [blob_of(reads[i::3]) for i in range(3)]
    whole = blob_of(reads)
    hv = kmer_hashes(whole)
    counters = rounded(sketch)
    bf = 1 << 15
    one = ntedit_amd.Polisher(0)
    parts = [_ctx_with_sketch(torch, counters, lib) for _ in range(3)]
    try:
        h1 = one._h
        assert lib.ntedit_hip_sketch_alloc(h1, sketch, HASHES, K) == 0
        assert lib.ntedit_hip_sketch_count(h1, whole, len(whole), 0) == 0
        for (pol, _), b in zip(parts, shards):
            assert lib.ntedit_hip_sketch_count(pol._h, b, len(b), 0) == 0, lib.ntedit_hip_reads_last_error(pol._h)
        got = np.zeros(counters, dtype=np.uint8)
        assert lib.ntedit_hip_sketch_download(h1, got.ctypes.data_as(ctypes.c_void_p)) == 0
        per_shard = [t.cpu().numpy() for _, t in parts]
        assert min(int((s == 255).sum()) for s in per_shard) > 0
        stacked = torch.cat([t for _, t in parts])
        merged = torch.zeros(counters, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.ntedit_hip_merge_bytes(h1, merged.data_ptr(), stacked.data_ptr(), 3, counters, SAT) == 0
        model = model_sketch(hv, counters)
        assert np.array_equal(merged.cpu().numpy(), got)
        assert np.array_equal(got, model)
        # the histogram pass of each shard against the merged sketch sums to the one-context histogram
        assert lib.ntedit_hip_sketch_histogram(h1, whole, len(whole), 0) == 0
        occ = np.zeros(256, dtype=np.uint64)
        for (pol, t), b in zip(parts, shards):
            t.copy_(merged)
            torch.cuda.synchronize()
            assert lib.ntedit_hip_sketch_histogram(pol._h, b, len(b), 0) == 0
            occ += _occ(lib, pol._h)
        assert np.array_equal(occ, _occ(lib, h1))
        # pass 2: OR / max of the shards' filters (adopted slots) = the one-context filters
        est = model_estimates(hv, model)
        for counts, op in ((False, OR), (True, MAX)):
            outs = []
            for (pol, _), b in zip(parts, shards):
                ft = torch.zeros(bf, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                pol.set_filter_device(ft.data_ptr(), bf, HASHES, K, slot=0, counting=counts)
                assert lib.ntedit_hip_filter_insert_solid(pol._h, 0, b, len(b), 0, 2) == 0, \
                    lib.ntedit_hip_reads_last_error(pol._h)
                outs.append(ft)
            if counts:
                assert lib.ntedit_hip_filter_alloc_counting(h1, 0, bf, HASHES, K) == 0
            else:
                one.filter_alloc(bf, HASHES, K)
            assert lib.ntedit_hip_filter_insert_solid(h1, 0, whole, len(whole), 0, 2) == 0
            ref = one.filter_download(0)
            flat = torch.cat(outs)
            m = torch.zeros(bf, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert lib.ntedit_hip_merge_bytes(h1, m.data_ptr(), flat.data_ptr(), 3, bf, op) == 0
            assert np.array_equal(m.cpu().numpy(), ref), counts
            want = model_counts(hv, est, 2, bf) if counts else model_bf(hv, est, 2, bf)
            assert np.array_equal(ref, want), counts
    finally:
        for pol, _ in parts:
            lib.ntedit_hip_sketch_free(pol._h)  # (adopted memory: freed by torch, not by the library)
            pol.close()
        lib.ntedit_hip_sketch_free(one._h)
        one.close()


def test_sketch_info_and_set_device_checks(tmp_path):
    import torch
    import ntedit_amd
    lib = ntedit_amd._lib.load()
    pol = ntedit_amd.Polisher(0)
    try:
        t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        assert lib.ntedit_hip_sketch_set_device(pol._h, t.data_ptr(), 4095, HASHES, K) != 0  # not a multiple of 8
        assert lib.ntedit_hip_sketch_set_device(pol._h, t.data_ptr() + 8, 4000, HASHES, K) != 0  # not 16-aligned
        assert lib.ntedit_hip_sketch_set_device(pol._h, t.data_ptr(), 4096, HASHES, K) == 0
        c, hn, k = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.ntedit_hip_sketch_info(pol._h, ctypes.byref(c), ctypes.byref(hn), ctypes.byref(k)) == 0
        assert (c.value, hn.value, k.value) == (4096, HASHES, K)
        lib.ntedit_hip_sketch_free(pol._h)
        assert lib.ntedit_hip_sketch_info(pol._h, None, None, None) != 0
        t.fill_(3)  # the adopted memory is still the caller's
        torch.cuda.synchronize()
        assert int(t.sum()) == 3 * 4096
    finally:
        pol.close()


# ------------------------------------------------------------------ 3. the driver against the binary
def _driver(world, args, backend, timeout=300):
    if world == 1 and backend == "nccl":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29531"]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(world),
               "--master-port", str(29531 + world)]
    cmd += ["-m", "ntedit_amd.make_reads", "--backend", backend] + list(args)
    env = dict(os.environ, PYTHONPATH=H.ROOT, OMP_NUM_THREADS="4")
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=H.ROOT, env=env)


def _binary(args, timeout=300):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """30x reads of a 100 kbp genome in three files: gzip FASTQ, plain FASTQ (the one the driver cuts), FASTA with
    lowercase runs and N"""
    d = tmp_path_factory.mktemp("mixed")
    rng = np.random.default_rng(29)
    genome = H.random_genome(rng, 100000)
    reads = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    for i in range(0, len(reads), 41):
        reads[i] = reads[i][:50].lower() + b"NNN" + reads[i][53:]
    third = len(reads) // 3
    gz, fq, fa = d / "a.fq.gz", d / "b.fq", d / "c.fa"
    write_fastq(gz, reads[:third], opener=gzip.open)
    write_fastq(fq, reads[third:2 * third] + [reads[7]] * 300)
    write_fasta(fa, reads[2 * third:])
    return dict(dir=d, files=[str(gz), str(fq), str(fa)])


MODES = {
    "c2": ["-c", "2", "--bf", str(1 << 16), "--sketch_bytes", "1000003"],
    "counts": ["-c", "2", "--bf", str(1 << 16), "--sketch_bytes", "1000003", "--counts"],
    "solid": ["--solid", "--hist", "{hist}"],
}


def _compare(mixed, world, backend, mode, extra=()):
    d = mixed["dir"]
    tag = "%s_%d_%s" % (backend, world, mode)
    ref_bf, ref_hist = d / ("ref_%s.bf" % mode), d / ("ref_%s.hist" % mode)
    args = [x.replace("{hist}", str(ref_hist)) for x in MODES[mode]]
    if not ref_bf.exists():
        r = _binary(["--reads"] + mixed["files"] + ["-k", str(K), "-o", str(ref_bf)] + args)
        assert r.returncode == 0, r.stderr
    out, hist = d / ("%s.bf" % tag), d / ("%s.hist" % tag)
    args = [x.replace("{hist}", str(hist)) for x in MODES[mode]]
    r = _driver(world, ["--reads"] + mixed["files"] + ["-k", str(K), "-o", str(out)] + args + list(extra), backend)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert out.read_bytes() == ref_bf.read_bytes(), tag
    if mode == "solid":
        assert hist.read_bytes() == ref_hist.read_bytes(), tag
    return r


def test_the_plain_fastq_is_cut_and_the_gzip_kept_whole(mixed):
    from ntedit_amd import _lib
    from ntedit_amd.make_reads import WHOLE, file_facts, plan
    lib = _lib.load()
    for world in (2, 3):
        units, owner = plan(mixed["files"], file_facts(lib, mixed["files"]), world)
        assert [(u.begin, u.end) for u in units if u.file == 0] == [(0, WHOLE)]
        assert len([u for u in units if u.file == 1]) > 1
        assert len(set(owner)) == world


@pytest.mark.parametrize("mode", sorted(MODES))
def test_driver_world_1_rccl_equals_the_binary(mixed, mode):
    _compare(mixed, 1, "nccl", mode)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_driver_gloo_rehearsal_equals_the_binary(mixed, world, mode):
    r = _compare(mixed, world, "gloo", mode)
    assert r.stderr.count("Pass 1 (count)") == world


def _multiline_fastq(path, reads, width=60):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            q = bytes(b"@+I5"[(i + j) % 4] for j in range(len(r)))  # quality lines that start with '@' or '+'
            f.write(b"@m%d\n" % i)
            for j in range(0, len(r), width):
                f.write(r[j:j + width] + b"\n")
            f.write(b"+\n")
            for j in range(0, len(q), width):
                f.write(q[j:j + width] + b"\n")


def test_multiline_fastq_is_identical_or_refused(mixed):
    d = mixed["dir"]
    rng = np.random.default_rng(5)
    genome = H.random_genome(rng, 30000)
    reads = [bytes(r) for r in simulate_reads(rng, genome, 20, length=151)]
    ml = d / "multi.fq"
    _multiline_fastq(ml, reads)
    ref = d / "ml_ref.bf"
    args = ["--reads", str(ml), "-k", str(K), "-c", "2", "--bf", str(1 << 15)]
    r = _binary(args + ["-o", str(ref)])
    assert r.returncode == 0, r.stderr
    out = d / "ml_nosplit.bf"
    r = _driver(2, args + ["-o", str(out), "--no-split"], "gloo")
    assert r.returncode == 0, r.stderr[-5000:]
    assert out.read_bytes() == ref.read_bytes()
    out = d / "ml_split.bf"
    r = _driver(3, args + ["-o", str(out)], "gloo")
    if r.returncode == 0:
        assert out.read_bytes() == ref.read_bytes()
    else:
        assert "--no-split" in r.stderr, r.stderr[-5000:]
        assert not out.exists()
