"""The count-min model of tests/reads_model.py against the oracle at every k and number of hashes the reads tool
accepts: ntHash k-mer by k-mer (rolling, lowercase, breaks), which bytes continue a k-mer (all 256), and the model's
cmin-1 filter against mkbf's file body.  No GPU: the GPU tests of the reads kernels compare with this model."""
import ctypes

import numpy as np
import pytest

import helpers as H
from reads_model import M64, awkward_reads, blob_of, kmer_hashes, model_bf, rounded

KS = [12, 13, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 193, 199, 200]
ACGT = set(b"ACGTacgt")


def _oracle():
    lib = H.oracle_lib()
    lib.ora_extend_hashes.argtypes = [ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint64)]
    lib.ora_extend_hashes.restype = None
    return lib


def _oracle_run_bases(lib, run, k):
    """fh + rh of every k-mer of one run of ACGTacgt, rolled as the reference does (upper case)"""
    up = run.upper()
    out = []
    fh = rh = 0
    for p in range(len(up) - k + 1):
        if p == 0:
            fh = lib.ora_base_forward_hash(up, k)
            rh = lib.ora_base_reverse_hash(up, k)
        else:
            fh = lib.ora_next_forward_hash(fh, k, up[p - 1], up[p + k - 1])
            rh = lib.ora_next_reverse_hash(rh, k, up[p - 1], up[p + k - 1])
        out.append((fh + rh) & M64)
    return out


def _oracle_hashes(lib, runs, k, h):
    """(n_kmers, h) of the k-mers of every run, in order"""
    buf = (ctypes.c_uint64 * h)()
    rows = []
    for run in runs:
        for base in _oracle_run_bases(lib, run, k):
            lib.ora_extend_hashes(base, k, h, buf)
            rows.append(list(buf))
    return np.array(rows, dtype=np.uint64).reshape(-1, h)


def _mixed_case_runs(rng, k):
    """runs of ACGT with lowercase letters, of lengths around k (shorter than k, exactly k, k + 1) and ~300 k-mers"""
    lengths = [k - 1, k, k + 1, 2 * k - 1, k + 300]
    runs = []
    for n in lengths:
        r = bytearray(H.random_genome(rng, n))
        for i in rng.integers(0, n, n // 4):
            r[i] |= 0x20
        runs.append(bytes(r))
    return runs


@pytest.mark.parametrize("k", KS)
def test_hashes_equal_the_oracle_at_every_k_and_h(k):
    lib = _oracle()
    rng = np.random.default_rng(1000 + k)
    runs = _mixed_case_runs(rng, k)
    # breaks of one and several bytes, and a record end
    seps = [b"N", b"n\n", b"RYK", b"\r\n", b"\x00", b"-" * (k - 1)]
    blob = b"".join(r + seps[i % len(seps)] for i, r in enumerate(runs))
    n_want = sum(max(0, len(r) - k + 1) for r in runs)
    assert n_want > 300
    for h in range(1, 9):
        got = kmer_hashes(blob, k, h)
        want = _oracle_hashes(lib, runs, k, h)
        assert got.shape == (n_want, h), (k, h)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (k, h, bad[:10])


@pytest.mark.parametrize("k", [12, 17, 33, 200])
def test_only_acgt_continues_a_kmer(k):
    """every byte value 0..255 once as a one-byte separator between two ACGT runs"""
    lib = _oracle()
    rng = np.random.default_rng(7 + k)
    h = 2
    pieces, runs, cur = [], [], b""
    for b in range(256):
        a = H.random_genome(rng, k // 2 + 3)
        pieces += [a, bytes([b])]
        cur += a
        if b in ACGT:
            cur += bytes([b])
        else:
            runs.append(cur)
            cur = b""
    tail = H.random_genome(rng, k + 2)
    pieces.append(tail)
    runs.append(cur + tail)
    blob = b"".join(pieces)
    got = kmer_hashes(blob, k, h)
    want = _oracle_hashes(lib, runs, k, h)
    # the 8 continuing letters make runs of about 2 (k / 2 + 3) + 1 bytes: each gives k-mers
    assert len(want) >= 8 * 6, len(want)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the model's LUT is exactly ACGTacgt
    from reads_model import LUT
    assert sorted(np.nonzero(LUT <= 3)[0].tolist()) == sorted(ACGT)


@pytest.mark.parametrize("k,h", [(12, 1), (17, 8), (33, 2), (64, 5), (128, 3), (200, 8)])
def test_model_filter_at_cmin_1_equals_mkbf(tmp_path, k, h):
    reads = awkward_reads(k, seed=50 + k, genome_len=3000, length=max(150, k + 60))
    fa = tmp_path / "r.fa"
    with open(fa, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))
    hv = kmer_hashes(blob_of(reads), k, h)
    assert len(hv) > 10000
    for nbytes in (1 << 12, 100003):
        out = tmp_path / ("mk%d.bf" % nbytes)
        H.mkbf([str(fa)], str(out), k=k, hashes=h, nbytes=nbytes)
        mk = H.load_bf(str(out))
        assert (mk["k"], mk["hash_num"], mk["bytes"]) == (k, h, rounded(nbytes))
        ones = np.ones(len(hv), dtype=np.uint8)  # at cmin 1 every k-mer that occurs is solid
        assert np.array_equal(model_bf(hv, ones, 1, rounded(nbytes)), mk["data"]), (k, h, nbytes)
