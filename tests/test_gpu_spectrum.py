"""The k-mer multiplicity spectrum (ntedit_hip_set_spectrum, ntedit_hip_spectrum_count, `ntedit --spectrum`) against
tests/spectrum_model.py, the numpy restatement of the definition.  Every comparison is exact equality of integers.  The
counting filters are made in numpy, so that the tests control the multiplicities; each is checked on the model first (bins
at 0, at 255 and at five or more values in between), so that a degenerate filter cannot let a test pass vacuously."""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import spectrum_model as SM
from test_gpu_reads_cascade import case as cascade_case  # noqa: F401  (the small read set of that file, built once here)

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
TILE = 16384
E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def pol():
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    p.set_params(ntedit_amd.default_params())
    yield p
    p.close()


def spread(i):
    """counts for the k-mers of a test filter by index: a third not entered, the rest over 1..60"""
    return np.where(i % 3 == 0, 0, 1 + (i * 7) % 60)


def same(got_bins, got_rows, want_bins, want_rows):
    bad = np.flatnonzero(np.asarray(got_bins) != want_bins)
    assert bad.size == 0, "bin %d: got %d, want %d (%d differ)" % (bad[0], got_bins[bad[0]], want_bins[bad[0]], bad.size)
    if got_rows is not None:
        got = np.asarray(got_rows).astype(SM.ROW_DTYPE)
        assert got.shape == want_rows.shape
        bad = np.flatnonzero(got != want_rows)
        assert bad.size == 0, "entry %d: got %s, want %s (%d differ)" % (bad[0], got[bad[0]], want_rows[bad[0]], bad.size)


def identities(bins, rows):
    assert int(bins.sum()) == int(rows["kmers"].sum())
    assert int((np.arange(256, dtype=np.uint64) * bins).sum()) == int(rows["sum"].sum())
    assert int(bins[255]) == int(rows["saturated"].sum())


def count_and_check(pol, blob, offs, lens, data, k, h):
    """the stand-alone call on host bytes against the model; returns (bins, rows)"""
    want = SM.spectrum(SM.entries_of(blob, offs, lens), data, k, h)
    got = pol.spectrum_count(blob, offs, lens)
    same(*got, *want)
    identities(*got)
    st = pol.spectrum_info()
    assert (st.kmers[0], st.kmers[1], st.ms[1]) == (int(want[0].sum()), 0, 0.0)
    return got


# ------------------------------------------------------------------------------- 1. tile and stream edges
@pytest.fixture(scope="module")
def edges():
    """k = 25, h = 3, 2^17 counters; an entry of 40,000 bases: an N-run across 16,384, lower case across 32,768, one R, a
    k-mer 400 times in a row (counted 255 times or more), and C^k at 37"""
    k, h, counters = 25, 3, 1 << 17
    rng = np.random.default_rng(1301)
    e = bytearray(H.random_genome(rng, 40000))
    e[TILE - 9:TILE + 14] = b"N" * 23
    e[2 * TILE - 300:2 * TILE + 500] = bytes(e[2 * TILE - 300:2 * TILE + 500]).lower()
    e[5000] = ord("R")
    sat = b"T" * (400 + k - 1)
    e[22000:22000 + len(sat)] = sat
    e = bytes(e)
    data = SM.counting_filter([e], k, h, counters, spread, pinned=[(sat, 255), (b"C" * k, 37)])  # (A^k is T^k's reverse complement)
    bins, _ = SM.spectrum([e], data, k, h)
    SM.check_not_degenerate(bins)
    assert bins[255] >= 400
    return dict(k=k, h=h, data=data, entry=e)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_tile_and_stream_edges(pol, edges, shift):
    """the entry alone, and 1..3 bytes further on behind a short first entry: the 64-start streams and the 16-byte staging
    chunks fall differently"""
    k, h, e = edges["k"], edges["h"], edges["entry"]
    pol.set_filter(edges["data"], h, k, counting=True)
    if shift == 0:
        blob, offs, lens = e + b"\n", [0], [len(e)]
    else:
        first = e[100:100 + 30 + shift - 1]  # (with its separator: 30 + shift bytes in front)
        blob, offs, lens = first + b"\n" + e + b"\n", [0, len(first) + 1], [len(first), len(e)]
        assert offs[1] % 16 == (30 + shift) % 16
    bins, rows = count_and_check(pol, blob, offs, lens, edges["data"], k, h)
    assert rows["kmers"][-1] == len(e) - k + 1 - (23 + k - 1) - k and bins[255] >= 400


# ------------------------------------------------------------------------------- 2. per-entry rows on shared words
def test_rows_of_tiny_and_abutting_entries(pol):
    """the 400 contigs of test_counts_tiny_contigs_sharing_bitmap_words (k - 1, k, 2k - 1 and random lengths below 64, N
    runs, lower case), then two entries that abut without a separator"""
    k, h = 25, 3
    rng = np.random.default_rng(5150)
    truth = H.random_genome(rng, 50000)
    seqs = []
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
        seqs.append(bytes(d))
    assert all(len(s) < 64 for s in seqs) and {k - 1, k, 2 * k - 1} <= {len(s) for s in seqs}
    blob, offs, lens, _ = H.pack_batch([(b"s", s) for s in seqs])
    # two abutting entries: the window that spans their border is no k-mer of either
    a, b = truth[1000:1060], truth[1060:1100]
    offs = np.concatenate((offs, [len(blob), len(blob) + len(a)])).astype(np.uint64)
    lens = np.concatenate((lens, [len(a), len(b)])).astype(np.uint32)
    blob = blob + a + b
    assert offs[-1] == offs[-2] + lens[-2] and len(blob) % 16 != 0
    sat = truth[200:200 + k]
    data = SM.counting_filter([truth], k, h, 1 << 18, spread, pinned=[(sat, 255)])
    seqs += [a, b, sat]
    blob, offs, lens = blob + b"\n" + sat, np.append(offs, len(blob) + 1), np.append(lens, len(sat)).astype(np.uint32)
    SM.check_not_degenerate(SM.spectrum(seqs, data, k, h)[0])
    pol.set_filter(data, h, k, counting=True)
    bins, rows = count_and_check(pol, blob, offs, lens, data, k, h)
    short = [i for i, s in enumerate(seqs) if len(s) == k - 1]
    assert len(short) > 20 and not rows[short]["kmers"].any() and not rows[short]["sum"].any()
    assert (rows["kmers"][400], rows["kmers"][401]) == (len(a) - k + 1, len(b) - k + 1)


# ------------------------------------------------------------------------------- 3. parameter matrix
@pytest.fixture(scope="module")
def matrix_batch():
    """20,000 bases in two entries, with an N run, lower case and a run of 300 T; the length is no multiple of 16 and the
    batch ends without a separator"""
    rng = np.random.default_rng(1303)
    g = bytearray(H.random_genome(rng, 20000))
    g[3000:3010] = b"N" * 10
    g[9000:9500] = bytes(g[9000:9500]).lower()
    g[15000:15300] = b"T" * 300
    a, b = bytes(g[:7003]), bytes(g[7003:])
    blob = a + b"\n" + b
    assert len(a) + len(b) == 20000 and len(blob) % 16 != 0 and not blob.endswith(b"\n")
    return blob, np.array([0, len(a) + 1], dtype=np.uint64), np.array([len(a), len(b)], dtype=np.uint32)


@pytest.mark.parametrize("counters", [1 << 17, 100003])
@pytest.mark.parametrize("k", [12, 25, 64, 200])
@pytest.mark.parametrize("h", [1, 3, 8])
def test_matrix(pol, matrix_batch, h, k, counters):
    import torch
    blob, offs, lens = matrix_batch
    seqs = SM.entries_of(blob, offs, lens)
    data = SM.counting_filter(seqs, k, h, counters, spread, pinned=[(b"T" * 300, 255)])
    want = SM.spectrum(seqs, data, k, h)
    SM.check_not_degenerate(want[0])
    pol.set_filter(data, h, k, counting=True)
    same(*pol.spectrum_count(blob, offs, lens), *want)
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    got = pol.spectrum_count(None, offs, lens, device_ptr=dev.data_ptr(), n=len(blob))
    same(*got, *want)
    identities(*got)
    # without rows: the same bins
    same(pol.spectrum_count(blob, offs, lens, rows=False)[0], None, want[0], None)


# ------------------------------------------------------------------------------- 4. one bin takes everything
def test_one_bin_takes_everything(pol, edges):
    """20,000 C: a single k-mer, every lane of every wavefront adds to the same LDS bin"""
    k, h, data = edges["k"], edges["h"], edges["data"]
    blob = b"C" * 20000
    m = int(SM.multiplicities(b"C" * k, data, k, h)[0])
    assert 37 <= m < 255
    pol.set_filter(data, h, k, counting=True)
    bins, rows = count_and_check(pol, blob, [0], [len(blob)], data, k, h)
    assert bins[m] == 20000 - k + 1 and int(bins.sum()) == 20000 - k + 1
    assert tuple(rows[0]) == (20000 - k + 1, m * (20000 - k + 1), 0)


# ------------------------------------------------------------------------------- 5. empty and degenerate input
def test_empty_and_degenerate(pol, edges):
    k, h = edges["k"], edges["h"]
    pol.set_filter(edges["data"], h, k, counting=True)
    zero = np.zeros(256, dtype=np.uint64)
    bins, rows = pol.spectrum_count(b"", [], [])
    assert (bins == zero).all() and rows.size == 0
    bins, rows = pol.spectrum_count(b"ACGT" * 100, [], [])
    assert (bins == zero).all() and rows.size == 0
    bins, rows = pol.spectrum_count(b"N" * 5000 + b"\n" + b"n" * 70, [0, 5001], [5000, 70])
    assert (bins == zero).all() and rows.size == 2 and not rows["kmers"].any()
    bins, rows = pol.spectrum_count(edges["entry"][:k - 1], [0], [k - 1])
    assert (bins == zero).all() and tuple(rows[0]) == (0, 0, 0)
    st = pol.spectrum_info()
    assert (st.kmers[0], st.kmers[1]) == (0, 0)


# ------------------------------------------------------------------------------- 6. through polish_batch
def _hip_params(**kw):
    import ntedit_amd
    return ntedit_amd.default_params(**kw)


def depth_of(before, after):
    from ntedit_amd import _lib
    rows = np.zeros(before.size, dtype=np.dtype(_lib.DEPTH_DTYPE))
    for f in ("kmers", "sum", "saturated"):
        rows[f + "_before"], rows[f + "_after"] = before[f], after[f]
    return rows


@pytest.fixture(scope="module")
def polish_case(tmp_path_factory, oracle_build):
    """spectrum_model.polish_case: the draft of H.make_case(.., 32001, "N lower") and a numpy counting filter over the truth"""
    return SM.polish_case(str(tmp_path_factory.mktemp("spectrum")))


def check_polish(tmp, recs, bf_path, tag, made_here=True, **par_kw):
    """the spectrum through polish_batch: before = the stand-alone call on the batch = the model, after = the model on
    the oracle's edited sequences, the rows' k-mers = the QV rows'; then with no apply flag at all"""
    import ntedit_amd
    hp = H.default_params(**par_kw)
    draft = os.path.join(tmp, tag + "_draft.fa")
    H.write_fasta(draft, recs)
    H.run_oracle(draft, bf_path, hp, os.path.join(tmp, tag + "_o"))
    bf = H.load_bf(bf_path)
    assert bf["counting"]
    k, h, data = bf["k"], bf["hash_num"], bf["data"]
    kept = [s for _, s in recs if len(s) >= hp.min_contig_len]
    edited = [s for _, s in H.read_fasta(os.path.join(tmp, tag + "_o_edited.fa"))]
    assert len(edited) == len(kept)
    want = SM.spectrum(kept, data, k, h), SM.spectrum(edited, data, k, h)
    if made_here:
        SM.check_not_degenerate(want[0][0])
    else:  # (a recorded filter holds what it holds: k-mers at 0 and at five or more other multiplicities)
        assert want[0][0][0] > 0 and int((want[0][0][1:] > 0).sum()) >= 5
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(bf_path, 0)
        pol.set_params(_hip_params(**par_kw))
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, hp.min_contig_len)
        alone = pol.spectrum_count(blob, offs, lens)
        same(*alone, *want[0])
        pol.set_spectrum(True)
        pol.set_apply(ntedit_amd.APPLY_QV)
        res = pol.polish_batch(blob, offs, lens)
        bins = res.spectrum(0), res.spectrum(1)
        depth, qv = res.depth(len(names)), res.qv(len(names))
        st = pol.spectrum_info()
        res.free()
        want_depth = depth_of(want[0][1], want[1][1])
        assert (bins[0] == alone[0]).all() and (bins[0] == want[0][0]).all() and (bins[1] == want[1][0]).all()
        assert (depth == want_depth).all()
        assert (depth["kmers_before"] == qv["kmers_before"]).all() and (depth["kmers_after"] == qv["kmers_after"]).all()
        assert (st.kmers[0], st.kmers[1]) == (int(bins[0].sum()), int(bins[1].sum())) and st.ms[0] > 0 and st.ms[1] > 0
        for which, stage in enumerate(("before", "after")):
            assert int(bins[which].sum()) == int(depth["kmers_" + stage].sum())
            assert int((np.arange(256, dtype=np.uint64) * bins[which]).sum()) == int(depth["sum_" + stage].sum())
            assert int(bins[which][255]) == int(depth["saturated_" + stage].sum())
            # a draft of A, C, G, T, N: the k-mers below max(1, -p) are the QV rows' absent ones (their -s 0 counts)
            assert int(bins[which][:max(1, hp.min_threshold)].sum()) == int(qv["absent_" + stage].sum())
        # no apply flag at all: the applier still runs, the edited bases go with the call
        pol.set_apply(0)
        res = pol.polish_batch(blob, offs, lens)
        assert (res.spectrum(0) == bins[0]).all() and (res.spectrum(1) == bins[1]).all() and (res.depth(len(names)) == want_depth).all()
        with pytest.raises(ntedit_amd.NtEditHipError):
            res.edited(len(names))
        with pytest.raises(ntedit_amd.NtEditHipError):
            res.qv(len(names))
        res.free()
    finally:
        pol.close()
    return bins, want_depth, names


def test_polish_make_case(polish_case):
    bins, depth, _ = check_polish(polish_case["tmp"], polish_case["recs"], polish_case["counts_bf"], "p2", min_threshold=2)
    # sanity on truth: the polish moves k-mers out of the bins below -p
    assert bins[1][:2].sum() < bins[0][:2].sum()


def test_polish_snv_mode(polish_case):
    """-s 1: step 1 marks every k-mer, no bitmap is read here -- the spectrum is the stand-alone one all the same"""
    check_polish(polish_case["tmp"], polish_case["recs"], polish_case["counts_bf"], "snv", min_threshold=2, snv=1)


def test_polish_golden_counting_p2(tmp_path, oracle_build):
    import test_golden as TG
    d = os.path.join(H.GOLDEN, "cases", "counting_p2")
    hp = TG.params_from_file(os.path.join(d, "params.txt"))
    kw = {f[0]: getattr(hp, f[0]) for f in hp._fields_}
    assert hp.min_threshold == 2
    check_polish(str(tmp_path), H.read_fasta(os.path.join(d, "draft.fa")), os.path.join(d, "filter.bf"), "gold", made_here=False, **kw)


def test_reserve_leaves_no_trace(pol, edges):
    k, h, e = edges["k"], edges["h"], edges["entry"]
    pol.set_filter(edges["data"], h, k, counting=True)
    got = pol.spectrum_count(e, [0], [len(e)])
    before = pol.spectrum_info()
    pol.set_spectrum(True)
    try:
        pol.reserve(1 << 20, 16)
    finally:
        pol.set_spectrum(False)
    after = pol.spectrum_info()
    assert (after.kmers[0], after.kmers[1], after.ms[0], after.ms[1]) == (before.kmers[0], before.kmers[1], before.ms[0], before.ms[1])
    assert after.kmers[0] == int(got[0].sum())


# ------------------------------------------------------------------------------- 7. the switch off; refusals
def test_switch_off_and_refusals(polish_case):
    import ntedit_amd
    recs = polish_case["recs"]
    blob, offs, lens, names = ntedit_amd.pack_batch(recs, 100)
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_params(_hip_params())
        # no PRIMARY filter
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\)" % E_ARG):
            pol.spectrum_count(blob, offs, lens)
        pol.set_spectrum(True)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\)" % E_ARG):
            pol.polish_batch(blob, offs, lens)
        # a plain PRIMARY filter: before anything is polished
        pol.load_filter_file(polish_case["bf"], 0)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\).*counting" % E_UNSUPPORTED):
            pol.spectrum_count(blob, offs, lens)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\).*counting" % E_UNSUPPORTED):
            pol.polish_batch(blob, offs, lens)
        msg = pol._lib.ntedit_hip_last_error(pol._h).decode()
        assert "\n" not in msg and msg.startswith("polish_batch:")
        # the switch off: the polish runs as ever, the result has no spectrum
        pol.set_spectrum(False)
        res = pol.polish_batch(blob, offs, lens)
        with pytest.raises(ntedit_amd.NtEditHipError, match="ntedit_hip_set_spectrum"):
            res.spectrum(0)
        with pytest.raises(ntedit_amd.NtEditHipError, match="ntedit_hip_set_spectrum"):
            res.depth(len(names))
        assert res.stats().events > 0
        res.free()
    finally:
        pol.close()


# ------------------------------------------------------------------------------- 8. CLI
def _run(cmd, cwd=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(path):
    with open(str(path), "rb") as f:
        return f.read()


def _model_tables(prefix, bf_path, draft_path, edited_path, min_len=100):
    """both tables under `prefix`, from the formatters applied to the model"""
    import ntedit_amd
    bf = H.load_bf(str(bf_path))
    recs = [(n, s) for n, s in H.read_fasta(str(draft_path)) if len(s) >= min_len]
    edited = [s for _, s in H.read_fasta(str(edited_path))]
    assert len(edited) == len(recs)
    before = SM.spectrum([s for _, s in recs], bf["data"], bf["k"], bf["hash_num"])
    after = SM.spectrum(edited, bf["data"], bf["k"], bf["hash_num"])
    pol = ntedit_amd.Polisher(0)
    try:
        pol.write_spectrum_tables(str(prefix), [n for n, _ in recs], before[0], after[0], depth_of(before[1], after[1]))
    finally:
        pol.close()
    return before, after


def test_cli_spectrum(polish_case, tmp_path):
    base = [NTEDIT, "-f", polish_case["draft"], "-r", polish_case["counts_bf"], "-p", 2]
    plain = _run(base + ["-b", tmp_path / "plain"])
    spec = _run(base + ["-b", tmp_path / "out", "--spectrum", "--report"])
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert _read(tmp_path / ("plain" + suffix)) == _read(tmp_path / ("out" + suffix)), suffix
    assert not list(tmp_path.glob("plain_spectrum*")) and not list(tmp_path.glob("plain_depth*"))
    assert "k-mer spectrum" not in plain.stdout
    before, after = _model_tables(tmp_path / "model", polish_case["counts_bf"], polish_case["draft"], tmp_path / "out_edited.fa")
    SM.check_not_degenerate(before[0])
    for suffix in ("_spectrum.tsv", "_depth.tsv"):
        assert _read(tmp_path / ("out" + suffix)) == _read(tmp_path / ("model" + suffix)), suffix
    assert len(_read(tmp_path / "out_spectrum.tsv").splitlines()) == 257
    assert _read(tmp_path / "out_depth.tsv").splitlines()[-1].startswith(b"#total\t")
    lines = [l for l in spec.stdout.splitlines() if l.startswith("k-mer spectrum (k=25): before ")]
    assert len(lines) == 1 and str(tmp_path / "out_spectrum.tsv") in lines[0] and str(tmp_path / "out_depth.tsv") in lines[0]
    assert "before %d k-mers" % int(before[0].sum()) in lines[0] and "after %d k-mers" % int(after[0].sum()) in lines[0]
    rep = [json.loads(l) for l in spec.stdout.splitlines() if l.startswith('{"spectrum": {')]
    assert len(rep) == 1
    rep = rep[0]["spectrum"]
    peak = lambda b: 1 + int(np.argmax(b[1:255]))  # noqa: E731  (the smallest multiplicity with the largest bin)
    assert (rep["kmers_before"], rep["zero_before"], rep["saturated_before"], rep["peak_before"]) == \
        (int(before[0].sum()), int(before[0][0]), int(before[0][255]), peak(before[0]))
    assert (rep["kmers_after"], rep["zero_after"], rep["saturated_after"], rep["peak_after"]) == \
        (int(after[0].sum()), int(after[0][0]), int(after[0][255]), peak(after[0]))
    assert rep["spectrum_before_ms"] > 0 and rep["spectrum_after_ms"] > 0
    # the same draft in one batch per contig: the bins are summed over the batches, the rows keep their order
    _run(base + ["-b", tmp_path / "small", "--spectrum", "--batch-bases", 1])
    for suffix in ("_spectrum.tsv", "_depth.tsv"):
        assert _read(tmp_path / ("small" + suffix)) == _read(tmp_path / ("out" + suffix)), suffix
    # a plain -r file is refused as soon as its header is read
    r = subprocess.run([NTEDIT, "-f", polish_case["draft"], "-r", polish_case["bf"], "-b", str(tmp_path / "no"), "--spectrum"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--spectrum" in r.stderr and "plain filter" in r.stderr and not list(tmp_path.glob("no_*"))


def test_cli_spectrum_cascade(tmp_path, cascade_case):
    """`--reads --counts -k 40,25 --spectrum`: a pair of tables per round under that round's prefix, each equal to the
    model against that round's saved filter"""
    prefix = tmp_path / "out"
    r = _run([NTEDIT, "-f", cascade_case["draft"], "--reads", *cascade_case["files"]["plain"], "--counts", "--cutoff", 2, "--bf", 1 << 20, "-k", "40,25", "-b", prefix,
              "--spectrum", "--save_bf", tmp_path / "f_{k}.bf"])
    assert r.stdout.count("k-mer spectrum (k=") == 2
    rounds = ((40, cascade_case["draft"], "out_k40"), (25, tmp_path / "out_k40_edited.fa", "out"))
    for k, draft, name in rounds:
        _model_tables(tmp_path / ("model_%d" % k), tmp_path / ("f_%d.bf" % k), draft, tmp_path / (name + "_edited.fa"))
        for suffix in ("_spectrum.tsv", "_depth.tsv"):
            assert _read(tmp_path / (name + suffix)) == _read(tmp_path / ("model_%d%s" % (k, suffix))), (k, suffix)
