"""The completeness marks (k_mark, NTEDIT_HIP_APPLY_SHARED, `ntedit --qv --completeness`) against a numpy model: the
k-mers of ACGTacgt of a batch (reads_model.kmer_hashes) whose h slots are all set in the filter set bit hv0 % bits of a
zero array.  Every comparison of arrays and popcounts is exact; only the estimate against the true number of distinct
k-mers has a bound, the estimator's own standard deviation."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from reads_model import kmer_hashes
from test_gpu_reads_cascade import case as cascade_case  # noqa: F401  (the small read set of that file, built once here)

from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
E_ARG, E_UNSUPPORTED = -1, -6
TILE = 16384
HASHES = 3


def _amd():
    import ntedit_amd
    return ntedit_amd


def filter_bits(data):
    return np.unpackbits(np.asarray(data, dtype=np.uint8), bitorder="little").astype(bool)


def present_hashes(blob, r_bits, k, h):
    """the hash rows of the blob's k-mers whose h slots are all set in the filter"""
    hv = kmer_hashes(blob, k, h)
    if not len(hv):
        return hv
    slots = (hv % np.uint64(len(r_bits))).astype(np.int64)
    return hv[r_bits[slots].all(axis=1)]


def model_marks(blobs, r_bits, k, h):
    """the mark array of the union of the blobs' present k-mers, as the filter's bytes"""
    m = np.zeros(len(r_bits), dtype=bool)
    for blob in blobs:
        hv = present_hashes(blob, r_bits, k, h)
        m[(hv[:, 0] % np.uint64(len(r_bits))).astype(np.int64)] = True
    return np.packbits(m, bitorder="little")


def popcount(a):
    return int(np.unpackbits(a).sum())


def card(set_bits, slots, h):
    return -(slots / h) * math.log1p(-set_bits / slots)


# ------------------------------------------------------------------ 1. the kernel's edges, through shared_mark
GENOME_LEN = 2 * TILE + 1024


@functools.lru_cache(maxsize=None)
def edge_data():
    """(genome, draft): the draft is the genome with a substitution every ~700 bases (absent k-mers), N runs -- one
    across the first tile's edge --, lower-case stretches, an R and a '-'; its first 300 bases are clean"""
    rng = np.random.default_rng(9100)
    genome = H.random_genome(rng, GENOME_LEN)
    d = bytearray(genome)
    for q in range(350, len(d), 701):
        d[q] = b"ACGT"[(b"ACGT".index(d[q]) + 1) % 4]
    d[1000:1005] = b"NNNNN"
    d[TILE - 3:TILE + 4] = b"N" * 7
    d[20000:20002] = b"NN"
    d[5000:5400] = bytes(d[5000:5400]).lower()
    d[25000:25100] = bytes(d[25000:25100]).lower()
    d[9000] = ord("R")
    d[12000] = ord("-")
    return genome, bytes(d)


@functools.lru_cache(maxsize=None)
def genome_filter(k, nbytes):
    """the plain filter of the genome's k-mers: bytes, as np.uint8"""
    hv = kmer_hashes(edge_data()[0], k, HASHES)
    bits = np.zeros(nbytes * 8, dtype=bool)
    bits[(hv % np.uint64(nbytes * 8)).ravel().astype(np.int64)] = True
    return np.packbits(bits, bitorder="little")


def edge_blob(n, k):
    """a batch of n bytes: up to k bytes one entry without a separator, else two entries, a separator behind each"""
    d = edge_data()[1]
    if n <= k:
        return d[:n]
    e1 = n // 2 + 7
    return d[:e1] + b"\n" + d[e1 + 1:n - 1] + b"\n"


@pytest.fixture(scope="module")
def polisher():
    pol = _amd().Polisher(0)
    yield pol
    pol.close()


@pytest.mark.parametrize("nbytes", [1 << 17, 100003 * 8], ids=["pow2", "not_pow2"])
@pytest.mark.parametrize("k", [12, 25, 64, 65, 200])
def test_mark_equals_the_model_at_the_tile_edges(polisher, k, nbytes):
    pol = polisher
    data = genome_filter(k, nbytes)
    r_bits = filter_bits(data)
    pol.set_filter(data, HASHES, k)
    pol.set_params(_amd().default_params())
    with pytest.raises(_amd().NtEditHipError):
        pol.shared_counts()  # (a new filter: no marks until the next begin)
    pol.shared_begin()
    assert pol.shared_download(0).size == nbytes
    some_absent = some_present = False
    for i, n in enumerate((k - 1, k, TILE - 1, TILE, TILE + 1, 2 * TILE + k - 2)):
        blob = edge_blob(n, k)
        assert len(blob) == n
        which = i & 1
        pol.shared_reset()
        pol.shared_mark(blob, which)
        want = model_marks([blob], r_bits, k, HASHES)
        got = pol.shared_download(which)
        assert np.array_equal(got, want), (n, popcount(got), popcount(want))
        assert not pol.shared_download(1 - which).any()
        st = pol.shared_counts()
        assert (st.bits, st.hash_num, st.k) == (nbytes * 8, HASHES, k)
        assert st.filter_set == popcount(data) and st.shared_set[which] == popcount(want) and st.shared_set[1 - which] == 0
        assert st.marked_calls == 1
        n_kmers = len(kmer_hashes(blob, k, HASHES))
        assert n_kmers == (0 if n < k else 1) or n > k
        some_present |= popcount(want) > 0
        some_absent |= len(present_hashes(blob, r_bits, k, HASHES)) < n_kmers
        assert not (want & ~data).any()  # (every marked bit is a bit of the filter)
    assert some_present and some_absent
    pol.shared_free()
    with pytest.raises(_amd().NtEditHipError):
        pol.shared_download(0)


# ------------------------------------------------------------------ 2. repeats, idempotence, accumulation, lifetime
def test_repeats_and_idempotence(polisher):
    pol, k, nbytes = polisher, 25, 1 << 17
    genome = edge_data()[0]
    hv = kmer_hashes(genome + b"\n" + b"A" * 5000, k, HASHES)
    bits = np.zeros(nbytes * 8, dtype=bool)
    bits[(hv % np.uint64(nbytes * 8)).ravel().astype(np.int64)] = True
    data = np.packbits(bits, bitorder="little")
    entry = edge_data()[1][300:1300]
    blob = (entry + b"\n") * 50 + b"A" * 5000 + b"\n"
    pol.set_filter(data, HASHES, k)
    pol.set_params(_amd().default_params())
    pol.shared_begin()
    pol.shared_begin()  # (idempotent: the marks stay)
    pol.shared_mark(blob, 0)
    once = pol.shared_download(0)
    want = model_marks([blob], bits, k, HASHES)
    assert np.array_equal(once, want)
    assert popcount(want) == len(np.unique(present_hashes(blob, bits, k, HASHES)[:, 0] % np.uint64(nbytes * 8)))
    pol.shared_mark(blob, 0)
    pol.shared_begin()
    assert np.array_equal(pol.shared_download(0), once)
    assert pol.shared_counts().marked_calls == 2


def test_accumulation_reset_and_release(polisher):
    pol, k, nbytes = polisher, 25, 100003 * 8
    data = genome_filter(k, nbytes)
    r_bits = filter_bits(data)
    d = edge_data()[1]
    blobs = [d[:9000] + b"\n", d[8000:21000] + b"\n" + d[21000:22000] + b"\n", d[30000:] + b"\n"]
    pol.set_filter(data, HASHES, k)
    pol.set_params(_amd().default_params())
    pol.shared_begin()
    for b in blobs:
        pol.shared_mark(b, 0)
    pol.shared_mark(b"".join(blobs), 1)
    one_by_one, at_once = pol.shared_download(0), pol.shared_download(1)
    assert np.array_equal(one_by_one, at_once)
    assert np.array_equal(one_by_one, model_marks(blobs, r_bits, k, HASHES))
    st = pol.shared_counts()
    assert st.marked_calls == 4 and st.shared_set[0] == st.shared_set[1] == popcount(at_once) > 0
    pol.shared_reset()
    assert not pol.shared_download(0).any() and not pol.shared_download(1).any()
    st = pol.shared_counts()
    assert (st.shared_set[0], st.shared_set[1], st.marked_calls, st.ms_mark[0], st.ms_mark[1]) == (0, 0, 0, 0.0, 0.0)
    # the marks belong to the filter: a new PRIMARY filter releases them
    pol.set_filter(genome_filter(k, 1 << 17), HASHES, k)
    stats = _lib.SharedStats()
    assert pol._lib.ntedit_hip_shared_counts(pol._h, ctypes.byref(stats)) == E_ARG
    assert pol._lib.ntedit_hip_shared_reset(pol._h) == E_ARG
    pol.shared_begin()
    assert pol.shared_counts().bits == (1 << 17) * 8 and not pol.shared_download(0).any()
    # a secondary filter plays no part
    pol.set_filter(genome_filter(k, 1 << 17), HASHES, k, slot=1)
    assert pol.shared_counts().bits == (1 << 17) * 8


# ------------------------------------------------------------------ 3. through polish_batch
def _polish(pol, recs, flags, min_len):
    amd = _amd()
    pol.set_apply(flags)
    blob, offs, lens, names = amd.pack_batch(recs, min_len)
    res = pol.polish_batch(blob, offs, lens)
    return res, names, blob


def check_polish(tmp, recs, bf_path, edited, **par_kw):
    """M[0] / M[1] of one polish_batch call against the model of the draft / of the edited sequences; the QV rows against
    APPLY_QV alone; the same records in two batches.  Returns (stats, exact number of distinct present k-mers before)"""
    amd = _amd()
    hp = H.default_params(**par_kw)
    bf = H.load_bf(bf_path)
    k, h = bf["k"], bf["hash_num"]
    r_bits = filter_bits(bf["data"])
    kept = [(n, s) for n, s in recs if len(s) >= hp.min_contig_len]
    assert len(edited) == len(kept)
    draft_blob = H.pack_batch(kept)[0]
    want = [model_marks([draft_blob], r_bits, k, h), model_marks([H.pack_batch([(b"e", s) for s in edited])[0]], r_bits, k, h)]
    pol = amd.Polisher(0)
    try:
        pol.load_filter_file(bf_path, 0)
        pol.set_params(amd.default_params(**par_kw))
        res, names, blob = _polish(pol, recs, amd.APPLY_QV, hp.min_contig_len)
        assert blob == draft_blob
        qv_alone = res.qv(len(names)).copy()
        res.free()
        with pytest.raises(amd.NtEditHipError):
            pol.shared_counts()  # (APPLY_QV alone begins no marks)
        res, names, _ = _polish(pol, recs, amd.APPLY_QV | amd.APPLY_SHARED, hp.min_contig_len)
        assert np.array_equal(res.qv(len(names)), qv_alone)
        res.free()
        got = [pol.shared_download(0), pol.shared_download(1)]
        for w in (0, 1):
            assert np.array_equal(got[w], want[w]), (w, popcount(got[w]), popcount(want[w]))
        st = pol.shared_counts()
        assert st.marked_calls == 2 and st.shared_set[0] == popcount(want[0]) and st.shared_set[1] == popcount(want[1])
        assert st.filter_set == popcount(bf["data"])
        # the same records in two batches
        pol.shared_reset()
        half = (len(kept) + 1) // 2
        parts = [p for p in (kept[:half], kept[half:]) if p]
        for part in parts:
            _polish(pol, part, amd.APPLY_QV | amd.APPLY_SHARED, hp.min_contig_len)[0].free()
        assert pol.shared_counts().marked_calls == 2 * len(parts)
        for w in (0, 1):
            assert np.array_equal(pol.shared_download(w), want[w]), w
        # APPLY_SHARED alone: the same marks, and the QV rows are not handed out
        pol.shared_reset()
        res, names, _ = _polish(pol, recs, amd.APPLY_SHARED, hp.min_contig_len)
        with pytest.raises(amd.NtEditHipError):
            res.qv(len(names))
        res.free()
        for w in (0, 1):
            assert np.array_equal(pol.shared_download(w), want[w]), w
    finally:
        pol.close()
    n_distinct = len(np.unique(present_hashes(draft_blob, r_bits, k, h)[:, 0]))
    return st, n_distinct


def test_polish_make_case_and_the_estimate(tmp_path, oracle_build):
    case = H.make_case(str(tmp_path), 32001, flavor="N lower")
    H.run_oracle(case["draft"], case["bf"], H.default_params(), os.path.join(str(tmp_path), "o"))
    edited = [s for _, s in H.read_fasta(os.path.join(str(tmp_path), "o_edited.fa"))]
    st, n = check_polish(tmp_path, H.read_fasta(case["draft"]), case["bf"], edited)
    # the estimate against truth: within 6 standard deviations of linear counting (+ 1 for the rounding of a count)
    bits = st.bits
    lib = _lib.load()
    est = lib.ntedit_hip_bloom_cardinality(st.shared_set[0], bits, 1)
    t = n / bits
    sd = math.sqrt(bits * (math.exp(t) - t - 1))
    print("distinct present k-mers %d, estimate %.1f, sd %.1f" % (n, est, sd))
    assert abs(est - n) <= 6 * sd + 1
    filter_kmers = lib.ntedit_hip_bloom_cardinality(st.filter_set, bits, st.hash_num)
    before, after = est / filter_kmers, lib.ntedit_hip_bloom_cardinality(st.shared_set[1], bits, 1) / filter_kmers
    print("completeness before %.6f after %.6f" % (before, after))
    assert after > before


def test_polish_many_contigs(tmp_path, oracle_build):
    case = H.make_many_case(str(tmp_path))
    H.run_oracle(case["draft"], case["bf"], H.default_params(), os.path.join(str(tmp_path), "o"))
    edited = [s for _, s in H.read_fasta(os.path.join(str(tmp_path), "o_edited.fa"))]
    assert len(edited) >= 2900
    check_polish(tmp_path, H.read_fasta(case["draft"]), case["bf"], edited)


def _golden(name):
    import test_golden as TG
    d = os.path.join(H.GOLDEN, "cases", name)
    hp = TG.params_from_file(os.path.join(d, "params.txt"))
    return d, hp, {f[0]: getattr(hp, f[0]) for f in hp._fields_}


def test_polish_snv_mode_marks_the_plain_screening(tmp_path):
    """-s 1: step 1's bitmap holds every k-mer, both screenings run again into ONE second bitmap -- the before-mark is
    queued in front of the screening of the edited bases"""
    d, hp, kw = _golden("snv_mode")
    assert hp.snv == 1
    edited = [s for _, s in H.read_fasta(os.path.join(d, "expected_edited.fa"))]
    check_polish(tmp_path, H.read_fasta(os.path.join(d, "draft.fa")), os.path.join(d, "filter.bf"), edited, **kw)


def test_counting_filter_is_refused():
    amd = _amd()
    d, hp, kw = _golden("counting_p2")
    assert H.load_bf(os.path.join(d, "filter.bf"))["counting"]
    recs = H.read_fasta(os.path.join(d, "draft.fa"))
    pol = amd.Polisher(0)
    try:
        pol.load_filter_file(os.path.join(d, "filter.bf"), 0)
        pol.set_params(amd.default_params(**kw))
        pol.set_apply(amd.APPLY_QV | amd.APPLY_SHARED)
        blob, offs, lens, names = amd.pack_batch(recs, hp.min_contig_len)
        with pytest.raises(amd.NtEditHipError, match=r"\(-6\).*counting"):
            pol.polish_batch(blob, offs, lens)
        assert pol._lib.ntedit_hip_shared_begin(pol._h) == E_UNSUPPORTED
        assert pol._lib.ntedit_hip_shared_mark(pol._h, 0, blob, len(blob), 0) == E_UNSUPPORTED
        assert len(pol._lib.ntedit_hip_last_error(pol._h).decode().splitlines()) == 1
        pol.set_apply(amd.APPLY_QV)
        pol.polish_batch(blob, offs, lens).free()  # (the QV counts take a counting filter as before)
    finally:
        pol.close()
    pol = amd.Polisher(0)
    try:
        assert pol._lib.ntedit_hip_shared_begin(pol._h) == E_ARG  # (no PRIMARY filter)
        assert pol._lib.ntedit_hip_shared_mark(pol._h, 0, b"ACGT", 4, 0) == E_ARG
    finally:
        pol.close()


# ------------------------------------------------------------------ 4. the CLI
def _run(cmd, cwd=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(path):
    with open(str(path), "rb") as f:
        return f.read()


def test_cli_completeness(tmp_path, oracle_build):
    case = H.make_case(str(tmp_path), 32001, flavor="N lower")
    with_qv = _run([NTEDIT, "-f", case["draft"], "-r", case["bf"], "-b", tmp_path / "qv", "--qv"])
    both = _run([NTEDIT, "-f", case["draft"], "-r", case["bf"], "-b", tmp_path / "cp", "--qv", "--completeness", "--report"])
    for suffix in ("_edited.fa", "_changes.tsv", "_qv.tsv"):
        assert _read(tmp_path / ("qv" + suffix)) == _read(tmp_path / ("cp" + suffix)), suffix
    assert not os.path.exists(str(tmp_path / "qv_completeness.tsv"))
    assert "k-mer completeness" not in with_qv.stdout
    lines = [l for l in both.stdout.splitlines() if l.startswith("k-mer completeness (k=25): before ")]
    assert len(lines) == 1 and "false positives" in lines[0] and lines[0].endswith("table: %s" % (tmp_path / "cp_completeness.tsv"))
    assert both.stdout.count('{"completeness": {') == 1
    # the rows: the formatter fed the model's popcounts
    bf = H.load_bf(case["bf"])
    r_bits = filter_bits(bf["data"])
    hp = H.default_params()
    kept = [(n, s) for n, s in H.read_fasta(case["draft"]) if len(s) >= hp.min_contig_len]
    edited = [(n, s) for n, s in H.read_fasta(str(tmp_path / "cp_edited.fa"))]
    st = _lib.SharedStats()
    st.bits, st.hash_num, st.k, st.filter_set = bf["bytes"] * 8, bf["hash_num"], bf["k"], popcount(bf["data"])
    st.shared_set[0] = popcount(model_marks([H.pack_batch(kept)[0]], r_bits, bf["k"], bf["hash_num"]))
    st.shared_set[1] = popcount(model_marks([H.pack_batch(edited)[0]], r_bits, bf["k"], bf["hash_num"]))
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    want = lib.ntedit_hip_completeness_header()
    for which, stage in ((0, b"before"), (1, b"after")):
        assert lib.ntedit_hip_completeness_format_row(stage, ctypes.byref(st), which, buf, len(buf)) == 0
        want += buf.value
    assert _read(tmp_path / "cp_completeness.tsv") == want
    rows = [l.split("\t") for l in want.decode().splitlines()[1:]]
    assert float(rows[1][6]) > float(rows[0][6]) > 0.9


def test_cli_counting_filter_is_refused_before_any_output(tmp_path):
    d, hp, kw = _golden("counting_p2")
    r = subprocess.run([NTEDIT, "-f", os.path.join(d, "draft.fa"), "-r", os.path.join(d, "filter.bf"), "-b", str(tmp_path / "o"),
                        "--qv", "--completeness"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--completeness" in lines[0] and "counting" in lines[0], r.stderr
    assert not list(tmp_path.glob("o*"))


def test_cli_completeness_cascade(tmp_path, cascade_case):
    """`--reads -k 31,25 --qv --completeness`: a table per round under that round's prefix, equal to the stand-alone run
    at that k fed the previous _edited.fa"""
    common = ["--cutoff", 2, "--bf", 1 << 20, "--qv", "--completeness"]
    reads = ["--reads", *cascade_case["files"]["plain"]]
    r = _run([NTEDIT, "-f", cascade_case["draft"]] + reads + ["-k", "31,25"] + common + ["-b", tmp_path / "o"])
    assert r.stdout.count("k-mer completeness (k=31)") == 1 and r.stdout.count("k-mer completeness (k=25)") == 1
    _run([NTEDIT, "-f", cascade_case["draft"]] + reads + ["-k", 31] + common + ["-b", tmp_path / "s31"])
    _run([NTEDIT, "-f", tmp_path / "s31_edited.fa"] + reads + ["-k", 25] + common + ["-b", tmp_path / "s25"])
    assert _read(tmp_path / "o_k31_edited.fa") == _read(tmp_path / "s31_edited.fa")
    first, last = _read(tmp_path / "o_k31_completeness.tsv"), _read(tmp_path / "o_completeness.tsv")
    assert first == _read(tmp_path / "s31_completeness.tsv")
    assert last == _read(tmp_path / "s25_completeness.tsv")
    assert first != last and len(first.splitlines()) == 3 and len(last.splitlines()) == 3
    assert [l.split(b"\t")[0] for l in last.splitlines()] == [b"stage", b"before", b"after"]
