"""Every kernel that walks a batch through nte_tile.h, at the four residues of k % 4 (the four-start reader's funnel has
one code path per residue): k = 12, 13, 14, 15 with h = 3, a filter of 2^17 slots once and one whose slot count is no
power of two once (100,003 counters; a plain filter, whose bits come in bytes, has 100,003 x 8 bytes as in its own
suites).  One batch per k: three entries that abut -- 16384 - (k - 1) bases, k - 1 bases (no k-mer; it ends exactly at
the tile's end) and k + 40 bases -- and a newline; an N at 16380 and lower case across 16384.  Every comparison is exact
equality of integers against the model the kernel's own suite uses."""
import functools

import numpy as np
import pytest

import cn_model as CM
import helpers as H
import spectrum_model as SM
from reads_model import kmer_hashes, model_sketch, rounded
from test_gpu_reads_matrix import Reads, host_batches
from test_gpu_shared import filter_bits, model_marks

pytestmark = pytest.mark.gpu

TILE = 16384
HASHES = 3
KS = [12, 13, 14, 15]
SLOTS = [1 << 17, 100003]

cases = pytest.mark.parametrize("k,slots", [(k, s) for k in KS for s in SLOTS])


@functools.lru_cache(maxsize=None)
def batch(k):
    """(blob, offs, lens, entries, genome): the entries are the genome's bytes with a substitution every 701 bases, the N
    and the lower case; the models are checked here, so that no comparison below is vacuous"""
    rng = np.random.default_rng(1600 + k)
    n = TILE + k + 40
    genome = H.random_genome(rng, n)
    d = bytearray(genome)
    for q in range(350, n, 701):
        d[q] = b"ACGT"[(b"ACGT".index(d[q]) + 1) % 4]
    d[TILE - 4] = ord("N")
    d[TILE - 8:TILE - 4] = bytes(d[TILE - 8:TILE - 4]).lower()
    d[TILE - 3:TILE + 9] = bytes(d[TILE - 3:TILE + 9]).lower()
    lens = np.array([TILE - (k - 1), k - 1, k + 40], dtype=np.uint32)
    offs = np.array([0, lens[0], TILE], dtype=np.uint64)
    assert int(offs[1] + lens[1]) == TILE and int(offs[2] + lens[2]) == n and d[16380] == ord("N")
    blob = bytes(d) + b"\n"
    entries = SM.entries_of(blob, offs, lens)
    kmers = [len(kmer_hashes(e, k, HASHES)) for e in entries]
    assert kmers[0] > 16000 and kmers[1] == 0 and kmers[2] == 41
    return blob, offs, lens, entries, genome


def spread(i):
    """counts of a counting filter's k-mers by index: a third not entered, the rest over 1..60"""
    return np.where(i % 3 == 0, 0, 1 + (i * 7) % 60)


@functools.lru_cache(maxsize=None)
def counting_filter(k, slots):
    return SM.counting_filter(batch(k)[3], k, HASHES, slots, spread)


@functools.lru_cache(maxsize=None)
def plain_filter(k, slots):
    """the genome's k-mers in a plain filter of 2^17 bits, or of 100,003 x 8 bytes"""
    nbytes = slots // 8 if slots & (slots - 1) == 0 else slots * 8
    hv = kmer_hashes(batch(k)[4], k, HASHES)
    bits = np.zeros(nbytes * 8, dtype=bool)
    bits[(hv % np.uint64(nbytes * 8)).ravel().astype(np.int64)] = True
    return np.packbits(bits, bitorder="little")


@pytest.fixture(scope="module")
def pol():
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    p.set_params(ntedit_amd.default_params())
    yield p
    p.close()


@cases
def test_spectrum(pol, k, slots):
    blob, offs, lens, entries, _ = batch(k)
    data = counting_filter(k, slots)
    want_bins, want_rows = SM.spectrum(entries, data, k, HASHES)
    assert want_bins[0] > 0 and int((want_bins[1:] > 0).sum()) >= 5
    assert want_rows["kmers"][0] > 0 and want_rows["kmers"][1] == 0 and want_rows["kmers"][2] > 0
    pol.set_filter(data, HASHES, k, counting=True)
    bins, rows = pol.spectrum_count(blob, offs, lens)
    assert np.array_equal(np.asarray(bins), want_bins)
    assert np.array_equal(np.asarray(rows).astype(SM.ROW_DTYPE), want_rows)


@cases
def test_copy_numbers(pol, k, slots):
    blob, offs, lens, entries, _ = batch(k)
    data = counting_filter(k, slots)
    counters = 1 << 16
    occ, w5, want_rows, nonzero = CM.side([entries], data, k, HASHES, counters)
    assert want_rows["kmers"][0] > 0 and want_rows["kmers"][1] == 0 and want_rows["kmers"][2] > 0
    assert int(occ.sum()) == int(want_rows["kmers"].sum()) and int(occ[1:].sum()) > 0  # (collisions: classes above 1)
    pol.set_filter(data, HASHES, k, counting=True)
    pol.set_cn(True, 1 << 30)
    try:
        pol.cn_append(0, blob, offs, lens)
        pol.cn_finish(counters)
        got_occ, got_w5 = pol.cn_table(0)
        got_rows = np.asarray(pol.cn_rows(0, 3)).astype(CM.ROW_DTYPE)
        assert pol.cn_info().nonzero[0] == nonzero
    finally:
        pol.set_cn(False, 0)
    assert np.array_equal(got_occ, occ) and np.array_equal(got_w5, w5) and np.array_equal(got_rows, want_rows)


@cases
def test_marks(pol, k, slots):
    blob = batch(k)[0]
    data = plain_filter(k, slots)
    want = model_marks([blob], filter_bits(data), k, HASHES)
    assert 0 < int(np.unpackbits(want).sum()) < len(kmer_hashes(blob, k, HASHES))  # (some k-mers present, some absent)
    pol.set_filter(data, HASHES, k)
    pol.shared_begin()
    pol.shared_reset()
    pol.shared_mark(blob, 0)
    assert np.array_equal(pol.shared_download(0), want)


@cases
def test_screen(pol, k, slots, oracle_build):
    blob = batch(k)[0]
    data = plain_filter(k, slots)
    want = H.oracle_screen(blob, dict(data=data, bytes=data.size, hash_num=HASHES, k=k, counting=False))
    absent = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 0 < absent < TILE // 2
    pol.set_filter(data, HASHES, k)
    got = pol.screen(blob)
    assert got.shape == want.shape and np.array_equal(got, want)


@cases
def test_filter_insert(pol, k, slots, tmp_path, oracle_build):
    blob = batch(k)[0]
    nbytes = plain_filter(k, slots).size
    H.write_fasta(str(tmp_path / "b.fa"), [(b"b", blob[:-1])])
    H.mkbf([str(tmp_path / "b.fa")], str(tmp_path / "b.bf"), k=k, hashes=HASHES, nbytes=nbytes)
    want = H.load_bf(str(tmp_path / "b.bf"))["data"]
    assert 0 < int(np.unpackbits(want).sum()) < nbytes * 8
    pol.filter_alloc(nbytes, HASHES, k)
    pol.filter_insert(blob)
    assert np.array_equal(pol.filter_download(), want)


@cases
def test_reads_sketch(k, slots):
    blob = batch(k)[0]
    counters = rounded(slots)
    want = model_sketch(kmer_hashes(blob, k, HASHES), counters)
    assert want.max() >= 2 and (want == 0).any()
    with Reads() as r:
        r.alloc(slots, HASHES, k)
        r.count(host_batches([blob]))
        assert np.array_equal(r.sketch(counters), want)
