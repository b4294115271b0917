"""The numpy restatement of the k-mer spectrum split by assembly copy number (include/ntedit_hip.h), on
reads_model.kmer_hashes / model_sketch / model_estimates and spectrum_model.multiplicities.

One SIDE is a list of batches, a batch a list of entries (bytes).  The sketch has `counters` 8-bit counters, a power of two,
and takes the filter's h hash values: S = RM.model_sketch(hv of every k-mer occurrence of the side, counters);
cn = min_i S[hv_i & (counters - 1)], the class c = min(cn, 5); occ[c - 1][m] counts occurrences, w5[m] sums RECIP[cn] over
class 5, a row per entry holds kmers and the five class counts.  A plain module shared by the copy-number tests."""
import numpy as np

import reads_model as RM
import spectrum_model as SM

ROW_DTYPE = np.dtype([("kmers", "<u8"), ("cn1", "<u8"), ("cn2", "<u8"), ("cn3", "<u8"), ("cn4", "<u8"), ("cn5plus", "<u8")])
RECIP = np.array([0] * 5 + [((1 << 32) + cn // 2) // cn for cn in range(5, 256)], dtype=np.uint64)


def entries(batches):
    return [e for b in batches for e in b]


def side_sketch(batches, k, h, counters):
    assert counters & (counters - 1) == 0
    hv = [RM.kmer_hashes(bytes(e), k, h) for e in entries(batches)]
    hv = np.concatenate(hv + [np.zeros((0, h), dtype=np.uint64)])
    return RM.model_sketch(hv, counters)


def copy_numbers(seq, sketch, k, h):
    """cn of every k-mer of one sequence, in order of position"""
    hv = RM.kmer_hashes(bytes(seq), k, h)
    if hv.shape[0] == 0:
        return np.zeros(0, dtype=np.uint8)
    return RM.model_estimates(hv, sketch)


def side(batches, data, k, h, counters):
    """(occ uint64[5][256], w5 uint64[256], rows ROW_DTYPE[entries], nonzero counters) of one side"""
    data = np.asarray(data, dtype=np.uint8)
    sketch = side_sketch(batches, k, h, counters)
    occ = np.zeros((5, 256), dtype=np.uint64)
    w5 = np.zeros(256, dtype=np.uint64)
    es = entries(batches)
    rows = np.zeros(len(es), dtype=ROW_DTYPE)
    for i, e in enumerate(es):
        cn = copy_numbers(e, sketch, k, h).astype(np.int64)
        m = SM.multiplicities(e, data, k, h).astype(np.int64)
        assert cn.size == m.size and (cn.size == 0 or cn.min() >= 1)
        cls = np.minimum(cn, 5)
        np.add.at(occ, (cls - 1, m), np.uint64(1))
        np.add.at(w5, m[cls == 5], RECIP[cn[cls == 5]])
        rows[i] = (cn.size,) + tuple(int((cls == c).sum()) for c in range(1, 6))
    return occ, w5, rows, int(np.count_nonzero(sketch))


def distinct(occ, w5):
    """uint64[5][256]: (occ[c - 1][m] + c // 2) // c for c = 1 .. 4, (w5[m] + 2^31) >> 32 for class 5"""
    out = np.zeros((5, 256), dtype=np.uint64)
    for c in range(1, 5):
        out[c - 1] = (occ[c - 1] + np.uint64(c // 2)) // np.uint64(c)
    out[4] = (w5 + np.uint64(1 << 31)) >> np.uint64(32)
    return out


_CODE = {c: i for i, c in enumerate(b"ACGT")}
_CODE.update({c | 0x20: i for c, i in list(_CODE.items())})


def canonical(w):
    """the canonical form of a k-mer of ACGTacgt: the smaller of the upper-case word and its reverse complement"""
    fwd = bytes(b"ACGT"[_CODE[c]] for c in w)
    rev = bytes(b"ACGT"[3 - _CODE[c]] for c in reversed(w))
    return min(fwd, rev)


def exact_counts(batches, k):
    """the definition without a sketch: a dictionary of canonical k-mers over the whole side, in Python integers; returns
    (counts dict, per entry the list of its k-mers' canonical forms in order of position)"""
    counts, per_entry = {}, []
    for e in entries(batches):
        words = []
        for p in range(len(e) - k + 1):
            w = e[p:p + k]
            if all(c in _CODE for c in w):
                cw = canonical(w)
                counts[cw] = counts.get(cw, 0) + 1
                words.append(cw)
        per_entry.append(words)
    return counts, per_entry


def brute_force(batches, data, k, h):
    """(occ list[5][256], w5 list[256], rows list of 6-tuples) with the exact copy number min(count, 255) of the
    dictionary instead of the sketch's, one k-mer at a time in Python integers"""
    counts, per_entry = exact_counts(batches, k)
    occ = [[0] * 256 for _ in range(5)]
    w5 = [0] * 256
    rows = []
    for e, words in zip(entries(batches), per_entry):
        m = SM.multiplicities(e, np.asarray(data, dtype=np.uint8), k, h)
        assert len(m) == len(words)
        row = [len(words), 0, 0, 0, 0, 0]
        for cw, mm in zip(words, m.tolist()):
            cn = min(counts[cw], 255)
            c = min(cn, 5)
            occ[c - 1][mm] += 1
            row[c] += 1
            if c == 5:
                w5[mm] += ((1 << 32) + cn // 2) // cn
        rows.append(tuple(row))
    return occ, w5, rows


def revcomp(s):
    return bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


FIXTURE_SEED, FIXTURE_K = 20261020, 25


def fixture_draft():
    """The nine contigs of the copy-number tests, from numpy.random.default_rng(FIXTURE_SEED) and helpers.random_genome.
    Four segments of 500 bases are drawn first, for the copy numbers 2, 3, 4 and 6.  Contig i of six is 5,000 random bases,
    then every segment c with i < c -- reverse-complemented on odd i --, each followed by 700 random bases: segment c is
    held c times, on both strands.  Then 300 random bases, A x 400, 300 random bases (A^25 occurs 376 times: 255 in the
    sketch); a contig with an N and an n; a contig of 24 bases (no k-mer at k = 25)."""
    import helpers as H
    rng = np.random.default_rng(FIXTURE_SEED)
    seg = {c: H.random_genome(rng, 500) for c in (2, 3, 4, 6)}
    contigs = []
    for i in range(6):
        s = H.random_genome(rng, 5000)
        for c in (2, 3, 4, 6):
            if i < c:
                s += (revcomp(seg[c]) if i % 2 else seg[c]) + H.random_genome(rng, 700)
        contigs.append(s)
    contigs.append(H.random_genome(rng, 300) + b"A" * 400 + H.random_genome(rng, 300))
    n = bytearray(H.random_genome(rng, 426))
    n[100], n[300] = ord("N"), ord("n")
    contigs.append(bytes(n))
    contigs.append(H.random_genome(rng, 24))
    return contigs, seg
