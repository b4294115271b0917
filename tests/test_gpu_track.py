"""The unsupported regions as intervals (NTEDIT_HIP_APPLY_TRACK, ntedit_hip_track_extract, `ntedit --qv --bed`) against
tests/track_model.py, the numpy restatement of the definition.  Every comparison is exact equality of the record arrays."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import track_model as M
from test_gpu_reads_cascade import case as cascade_case  # noqa: F401  (the small read set of that file, built once here)

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
TILE = 16384
LONG = 3 * TILE + 37  # one entry of three tiles + 37 positions


@pytest.fixture(scope="module")
def pol():
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p.close()


def same(got, want):
    got = np.asarray(got).astype(M.DTYPE)
    assert got.shape == want.shape, "%d records, the model has %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "record %d: got %s, want %s (%d differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)


# ------------------------------------------------------------------------------------------- crafted bitmaps
@pytest.mark.parametrize("k", [12, 25, 64, 65, 200])
@pytest.mark.parametrize("extra", [0, 1])
def test_gap_boundary(pol, k, extra):
    """pairs of marks exactly k (one interval) and k + 1 (two) apart, across a word boundary, across a tile boundary from
    both sides, and with the second mark on the last valid start; at k = 200 the look-behind spans four words"""
    gap = k + extra
    last = LONG - k
    bits = np.zeros(LONG, dtype=np.uint8)
    pairs = [(63, 63 + gap), (TILE - 1, TILE - 1 + gap), (2 * TILE - gap, 2 * TILE), (last - gap, last)]
    for a, b in pairs:
        assert bits[max(a - 2 * k - 2, 0):b + 2 * k + 2].sum() == 0  # (the pairs stay apart)
        bits[a] = bits[b] = 1
    assert pairs[0][0] // 64 != pairs[0][1] // 64 and pairs[1][0] // TILE != pairs[1][1] // TILE
    assert pairs[2][0] // TILE != pairs[2][1] // TILE
    bits[last + 1:] = 1  # the last k - 1 positions start no k-mer
    want = M.intervals(bits, [0], [LONG], k)
    assert want.size == (8 if extra else 4) and set(want["absent"]) == ({1} if extra else {2})
    same(pol.track_extract(M.words_of(bits), [0], [LONG], k, n=LONG), want)


@pytest.mark.parametrize("k", [25, 200])
def test_long_interval(pol, k):
    """all ones: one record, whose begin and whose end are found by different workgroups"""
    words = np.full((LONG + 63) // 64, 2 ** 64 - 1, dtype=np.uint64)
    got = pol.track_extract(words, [0], [LONG], k, n=LONG)
    same(got, np.array([(0, 0, LONG, LONG - k + 1)], dtype=M.DTYPE))
    st = pol.track_info()
    assert (st.intervals[0], st.bases[0], st.intervals[1], st.bases[1]) == (1, LONG, 0, 0)


def test_entries_sharing_words(pol):
    """400 entries of 10 to 63 bases, abutting or a separator apart, every bit set: separators, the last k - 1 positions
    and the padding behind n are ignored, entries shorter than k give nothing, abutting entries give separate records"""
    k = 25
    rng = np.random.default_rng(7001)
    lens = rng.integers(10, 64, size=400).astype(np.uint32)
    lens[:6] = (k - 1, k, 63, 10, 2 * k - 1, k)
    seps = rng.integers(0, 2, size=400)
    seps[:6] = (0, 0, 1, 0, 0, 1)
    offs = np.concatenate(([0], np.cumsum(lens.astype(np.int64) + seps)[:-1])).astype(np.uint64)
    if int(offs[-1] + lens[-1]) % 64 == 0:
        lens[-1] -= 1  # (the last word has padding behind n)
    n = int(offs[-1] + lens[-1])
    assert n % 64 != 0 and (seps == 0).sum() > 100 and (seps == 1).sum() > 100 and (lens < k).sum() > 50
    words = np.full((n + 63) // 64, 2 ** 64 - 1, dtype=np.uint64)
    got = pol.track_extract(words, offs, lens, k, n=n)
    same(got, M.intervals(M.bits_of(words), offs, lens, k))
    per_entry = np.bincount(got["entry"], weights=got["absent"], minlength=400).astype(np.int64)
    assert (per_entry == np.maximum(lens.astype(np.int64) - k + 1, 0)).all()
    assert got.size == int((lens >= k).sum()) and (got["begin"] == 0).all() and (got["end"] == lens[got["entry"]]).all()


def test_empty_and_overflow(pol):
    k = 25
    zero = np.zeros(4, dtype=np.uint64)
    ones = np.full(4, 2 ** 64 - 1, dtype=np.uint64)
    assert pol.track_extract(zero, [0, 100], [100, 100], k).size == 0
    assert pol.track_extract(ones, [], [], k).size == 0
    assert pol.track_extract(ones, [3], [k - 1], k).size == 0
    # cap one too small: NTEDIT_E_OVERFLOW, *n correct
    offs, lens = np.array([0, 100], dtype=np.uint64), np.array([100, 100], dtype=np.uint32)
    bits = np.zeros(256, dtype=np.uint8)
    bits[[0, 40, 99, 100, 160]] = 1  # (99: no start of entry 0)
    words = M.words_of(bits)
    want = M.intervals(bits, offs, lens, k)
    assert want.size == 4
    vp = ctypes.c_void_p
    out = np.zeros(4, dtype=M.DTYPE)
    n = ctypes.c_uint64()
    args = (pol._h, words.ctypes.data_as(vp), 256, offs.ctypes.data_as(vp), lens.ctypes.data_as(vp), 2, k, out.ctypes.data_as(vp))
    assert pol._lib.ntedit_hip_track_extract(*args, 3, ctypes.byref(n)) == -4 and n.value == 4
    assert pol._lib.ntedit_hip_track_extract(*args, 4, ctypes.byref(n)) == 0 and n.value == 4
    same(out, want)


@pytest.mark.parametrize("k", [25, 65])
@pytest.mark.parametrize("density", ["1/4", "1/k", "1/(4k)"])
def test_random(pol, k, density):
    n = 100000
    rng = np.random.default_rng(9000 + k + len(density))
    cuts = np.sort(rng.choice(np.arange(1, n), size=299, replace=False))
    begins = np.concatenate(([0], cuts))
    ends = np.concatenate((cuts, [n]))
    seps = rng.integers(0, 2, size=300)  # (a separator is the entry's last position given up)
    lens = np.maximum(ends - begins - seps, 0).astype(np.uint32)
    offs = begins.astype(np.uint64)
    assert (lens < k).any() and (lens > 1000).any()
    p = {"1/4": 0.25, "1/k": 1.0 / k, "1/(4k)": 0.25 / k}[density]
    bits = (rng.random(n) < p).astype(np.uint8)
    want = M.intervals(bits, offs, lens, k)
    assert want.size > 50
    same(pol.track_extract(M.words_of(bits), offs, lens, k, n=n), want)


# ------------------------------------------------------------------------------------------------ the polish
def _hip_params(**kw):
    import ntedit_amd
    return ntedit_amd.default_params(**kw)


def model_tracks(seqs, bf, k, p=1):
    """the model on the oracle's screening of a batch of these sequences"""
    blob, offs, lens, _ = H.pack_batch([(b"s", s) for s in seqs])
    return M.intervals(M.bits_of(H.oracle_screen(blob, bf, min_threshold=p)), offs, lens, k)


def check_tracks(tmp, recs, bf_path, flags_too=False, **par_kw):
    """Result.track() of recs against the model on the draft and on the oracle's edited sequences, and against the result's
    own QV rows; returns (before, after)"""
    import ntedit_amd
    hp = H.default_params(**par_kw)
    draft = os.path.join(str(tmp), "tr_draft.fa")
    H.write_fasta(draft, recs)
    H.run_oracle(draft, bf_path, hp, os.path.join(str(tmp), "tr_o"))
    bf = H.load_bf(bf_path)
    k, p = bf["k"], (hp.min_threshold if bf["counting"] else 1)
    kept = [s for _, s in recs if len(s) >= hp.min_contig_len]
    edited = [s for _, s in H.read_fasta(os.path.join(str(tmp), "tr_o_edited.fa"))]
    assert len(edited) == len(kept)
    want = model_tracks(kept, bf, k, p), model_tracks(edited, bf, k, p)
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(bf_path, 0)
        pol.set_params(_hip_params(**par_kw))
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, hp.min_contig_len)
        pol.set_apply(ntedit_amd.APPLY_QV | ntedit_amd.APPLY_TRACK)
        res = pol.polish_batch(blob, offs, lens)
        got = res.track(0), res.track(1)
        rows = res.qv(len(names))
        st = pol.track_info()
        res.free()
        for which, field in ((0, "absent_before"), (1, "absent_after")):
            same(got[which], want[which])
            per_entry = np.bincount(got[which]["entry"], weights=got[which]["absent"], minlength=len(names)).astype(np.uint64)
            assert (per_entry == rows[field]).all(), field
            assert st.intervals[which] == got[which].size
            assert st.bases[which] == int((got[which]["end"].astype(np.int64) - got[which]["begin"]).sum())
        if flags_too:
            pol.set_apply(ntedit_amd.APPLY_TRACK)
            res = pol.polish_batch(blob, offs, lens)
            same(res.track(0), want[0])
            same(res.track(1), want[1])
            with pytest.raises(ntedit_amd.NtEditHipError):
                res.qv(len(names))
            res.free()
            pol.set_apply(ntedit_amd.APPLY_QV)
            res = pol.polish_batch(blob, offs, lens)
            with pytest.raises(ntedit_amd.NtEditHipError, match="APPLY_TRACK"):
                res.track(0)
            res.free()
    finally:
        pol.close()
    return got


def test_tracks_make_case(tmp_path, oracle_build):
    case = H.make_case(str(tmp_path), 32001, flavor="N lower")
    before, after = check_tracks(tmp_path, H.read_fasta(case["draft"]), case["bf"], flags_too=True)
    assert 0 < after.size < before.size


def test_tracks_many_contigs(tmp_path, oracle_build):
    case = H.make_many_case(str(tmp_path))
    before, _ = check_tracks(tmp_path, H.read_fasta(case["draft"]), case["bf"])
    assert np.unique(before["entry"]).size > 1000


@pytest.mark.parametrize("name", ["counting_p2", "snv_mode"])
def test_tracks_golden(tmp_path, oracle_build, name):
    import test_golden as TG
    d = os.path.join(H.GOLDEN, "cases", name)
    hp = TG.params_from_file(os.path.join(d, "params.txt"))
    kw = {f[0]: getattr(hp, f[0]) for f in hp._fields_}
    check_tracks(tmp_path, H.read_fasta(os.path.join(d, "draft.fa")), os.path.join(d, "filter.bf"), **kw)


def test_tracks_tiny_contigs_sharing_bitmap_words(tmp_path, oracle_build):
    """every contig shorter than 64 bases (-z k - 1): every contig shares its first bitmap word with its neighbour"""
    k = 25
    rng = np.random.default_rng(5150)
    truth = H.random_genome(rng, 50000)
    H.write_fasta(os.path.join(str(tmp_path), "truth.fa"), [(b"t", truth)])
    bf = os.path.join(str(tmp_path), "t.bf")
    H.mkbf([os.path.join(str(tmp_path), "truth.fa")], bf, k=k, hashes=3, nbytes=1 << 17)
    recs = []
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
        recs.append((b"tiny%d" % i, bytes(d)))
    assert all(len(s) < 64 for _, s in recs) and {k - 1, k, 2 * k - 1} <= {len(s) for _, s in recs}
    before, _ = check_tracks(tmp_path, recs, bf, min_contig_len=k - 1)
    assert before.size > 100


def test_truth_has_no_interval(tmp_path, oracle_build):
    case = H.make_case(str(tmp_path), 32002)
    before, after = check_tracks(tmp_path, H.read_fasta(case["truth"]), case["bf"])
    assert before.size == 0 and after.size == 0


# ---------------------------------------------------------------------------------------------------------- CLI
def _run(cmd, cwd=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _strip_times(text):
    """standard output without the wall-clock stamps behind the stage lines"""
    return [l.split(" : ")[0] if l.startswith("----------") else l for l in text.splitlines()]


def _read(path):
    with open(str(path), "rb") as f:
        return f.read()


def _bed(path):
    rows = [l.split(b"\t") for l in _read(path).splitlines()]
    assert all(len(r) == 4 for r in rows)
    return [(r[0], int(r[1]), int(r[2]), int(r[3])) for r in rows]


def test_cli_bed(tmp_path, oracle_build):
    import ntedit_amd
    case = H.make_case(str(tmp_path), 32003, flavor="N lower")
    recs = [(b"%s some words\tand a tab" % name, seq) for name, seq in H.read_fasta(case["draft"])]
    draft = str(tmp_path / "named.fa")
    H.write_fasta(draft, recs)
    base = [NTEDIT, "-f", draft, "-r", case["bf"]]
    qv = _run(base + ["-b", tmp_path / "qv", "--qv"])
    bed = _run(base + ["-b", tmp_path / "bed", "--qv", "--bed"])
    for suffix in ("_edited.fa", "_changes.tsv", "_qv.tsv"):
        assert _read(tmp_path / ("qv" + suffix)) == _read(tmp_path / ("bed" + suffix)), suffix
    assert not list(tmp_path.glob("qv_absent_*"))
    a = _strip_times(qv.stdout.replace(str(tmp_path / "qv"), "P"))
    b = _strip_times(bed.stdout.replace(str(tmp_path / "bed"), "P"))
    extra = [l for l in b if l not in a]
    assert len(b) == len(a) + 1 and len(extra) == 1, (a, b)
    assert extra[0].startswith("unsupported regions: before ") and "P_absent_before.bed" in extra[0] and "P_absent_after.bed" in extra[0]
    said = [int(x) for x in re.match(r"unsupported regions: before (\d+) intervals over (\d+) bases, after (\d+) over (\d+); ", extra[0]).groups()]
    # the rows equal the ABI's records under the names' first words
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(case["bf"], 0)
        pol.set_params(_hip_params())
        pol.polish_records(recs, str(tmp_path / "py"), qv=True, bed=True)
        pol.set_apply(ntedit_amd.APPLY_QV | ntedit_amd.APPLY_TRACK)
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, pol.params.min_contig_len)
        res = pol.polish_batch(blob, offs, lens)
        tracks = res.track(0), res.track(1)
        res.free()
    finally:
        pol.close()
    first_words = [n.split(b" ")[0].split(b"\t")[0] for n in names]
    assert all(b" " in n and w for n, w in zip(names, first_words))
    for which, stage in enumerate(("before", "after")):
        rows = _bed(tmp_path / ("bed_absent_%s.bed" % stage))
        want = [(first_words[r["entry"]], int(r["begin"]), int(r["end"]), int(r["absent"])) for r in tracks[which]]
        assert rows == want and len(rows) > 0
        assert _read(tmp_path / ("py_absent_%s.bed" % stage)) == _read(tmp_path / ("bed_absent_%s.bed" % stage))
        assert said[2 * which:2 * which + 2] == [len(rows), sum(r[2] - r[1] for r in rows)]
    # the same draft in one batch per contig (the smallest --batch-bases the option takes): the same two files
    assert len(names) >= 3
    _run(base + ["-b", tmp_path / "small", "--qv", "--bed", "--batch-bases", 1])
    for stage in ("before", "after"):
        assert _read(tmp_path / ("small_absent_%s.bed" % stage)) == _read(tmp_path / ("bed_absent_%s.bed" % stage)), stage
    # --report: one JSON line more
    rep = _run(base + ["-b", tmp_path / "rep", "--qv", "--bed", "--report"])
    assert sum(l.startswith('{"bed": {') for l in rep.stdout.splitlines()) == 1


def test_cli_bed_cascade(tmp_path, cascade_case):
    """`--reads -k 31,25 --qv --bed`: a pair of tracks per round, under that round's prefix"""
    prefix = tmp_path / "casc"
    r = _run([NTEDIT, "-f", cascade_case["draft"], "--reads", *cascade_case["files"]["plain"], "-k", "31,25", "--cutoff", 2,
              "--bf", 1 << 20, "-b", prefix, "--qv", "--bed"])
    assert r.stdout.count("unsupported regions: before ") == 2
    for mid in ("_k31", ""):
        total = open(str(prefix) + mid + "_qv.tsv").read().splitlines()[-1].split("\t")
        assert total[0] == "#total"
        for stage, col in (("before", 4), ("after", 7)):
            rows = _bed(str(prefix) + mid + "_absent_%s.bed" % stage)
            assert sum(row[3] for row in rows) == int(total[col]), (mid, stage)
            assert {row[0] for row in rows} <= {b"ctg1", b"ctg2"}
