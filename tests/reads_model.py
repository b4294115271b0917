"""The numpy count-min model of ntedit-make-reads-bf, for any k and number of hashes: ntHash of every k-mer of
ACGTacgt (checked against the oracle in tests/test_reads_model_cpu.py), the sketch, the estimates, both outputs and
the k-mer histogram, and the read sets the reads tests feed it.  A plain module shared by the reads tests."""
import numpy as np

import helpers as H

M64 = (1 << 64) - 1


def _sroln(x, d):
    lo, hi = x & 0x1FFFFFFFF, x >> 33
    dl, dh = d % 33, d % 31
    if dl:
        lo = ((lo << dl) | (lo >> (33 - dl))) & 0x1FFFFFFFF
    if dh:
        hi = ((hi << dh) | (hi >> (31 - dh))) & 0x7FFFFFFF
    return (hi << 33) | lo


SEEDS = [0x3c8bfbb395c60474, 0x3193c18562a02b4c, 0x20323ed082572324, 0x295549f54be24456]  # A C G T
MULTISEED, MULTISHIFT = 0x90b45d39fb6da1fa, 27
# a k-mer is a run of k bytes of ACGTacgt; every other byte ends it (the kernels' LUT: char_code(c) <= 3)
LUT = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    LUT[_c] = LUT[_c | 0x20] = _i


def kmer_hashes(blob, k, h):
    """the h hash values of every k-mer of ACGTacgt in `blob` (a k-mer ends at any other byte): (n_kmers, h) uint64"""
    codes = LUT[np.frombuffer(blob, dtype=np.uint8)]
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros((0, h), dtype=np.uint64)
    starts = np.nonzero(bad[k:k + n] - bad[:n] == 0)[0]
    fh = np.zeros(len(starts), dtype=np.uint64)
    rh = np.zeros(len(starts), dtype=np.uint64)
    for i in range(k):
        c = codes[starts + i]
        tf = np.array([_sroln(SEEDS[x], k - 1 - i) for x in range(4)], dtype=np.uint64)
        tr = np.array([_sroln(SEEDS[3 - x], i) for x in range(4)], dtype=np.uint64)
        fh ^= tf[c]
        rh ^= tr[c]
    base = fh + rh
    out = np.empty((len(starts), h), dtype=np.uint64)
    out[:, 0] = base
    for i in range(1, h):
        t = base * np.uint64(i ^ ((k * MULTISEED) & M64))
        out[:, i] = t ^ (t >> np.uint64(MULTISHIFT))
    return out


def rounded(nbytes):
    return (nbytes + 7) // 8 * 8


def model_sketch(hv, counters):
    slots = (hv % np.uint64(counters)).ravel()
    return np.minimum(np.bincount(slots.astype(np.int64), minlength=counters), 255).astype(np.uint8)


def model_estimates(hv, sketch):
    return sketch[(hv % np.uint64(len(sketch))).astype(np.int64)].min(axis=1)


def model_bf(hv, est, cmin, nbytes):
    bits = np.zeros(nbytes * 8, dtype=bool)
    bits[(hv[est >= cmin] % np.uint64(nbytes * 8)).ravel().astype(np.int64)] = True
    return np.packbits(bits, bitorder="little")


def model_counts(hv, est, cmin, nbytes):
    out = np.zeros(nbytes, dtype=np.uint8)
    keep = est >= cmin
    slots = (hv[keep] % np.uint64(nbytes)).astype(np.int64)
    np.maximum.at(out, slots.ravel(), np.repeat(est[keep], hv.shape[1]).astype(np.uint8))
    return out


def model_occ(hv, sketch):
    """the 256-bin histogram of est(x) over every k-mer occurrence"""
    return np.bincount(model_estimates(hv, sketch), minlength=256).astype(np.uint64)


def blob_of(reads):
    return b"\n".join(reads) + b"\n"


def simulate_reads(rng, genome, coverage, length=150, err=0.01):
    n = int(len(genome) * coverage / length)
    g = np.frombuffer(genome, dtype=np.uint8)
    starts = rng.integers(0, len(genome) - length, n)
    reads = g[starts[:, None] + np.arange(length)].copy()
    e = rng.random(reads.shape) < err
    reads[e] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(e.sum()))]
    return reads


def awkward_reads(k, seed=17, genome_len=40000, err=0.01, length=150):
    """(by default ~1e6 k-mers) 30x reads with errors, N runs, lowercase, reads shorter than k, one read 300 times"""
    rng = np.random.default_rng(seed)
    genome = H.random_genome(rng, genome_len)
    arr = simulate_reads(rng, genome, 30, length=length, err=err)
    reads = [bytes(r) for r in arr]
    for i in range(0, len(reads), 37):
        r = bytearray(reads[i])
        p, n_run = int(rng.integers(0, length - 10)), int(rng.integers(1, 10))
        r[p:p + n_run] = b"N" * n_run
        reads[i] = bytes(r)
    for i in range(5, len(reads), 23):
        reads[i] = reads[i][:60].lower() + reads[i][60:]
    for i in range(11, len(reads), 101):
        reads[i] = reads[i][:int(rng.integers(1, k))]
    reads += [reads[3]] * 300
    return reads
