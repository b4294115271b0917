"""The k-mer spectrum split by assembly copy number (ntedit_hip_set_cn, ntedit_hip_cn_append / _finish / _table / _rows,
`ntedit --spectrum --cn`) against tests/cn_model.py, the numpy restatement of the definition.  Every comparison is exact
equality of integers.

The fixture draft (cn_model.fixture_draft; k = 25) holds 49,184 k-mers whose exact classes -- from a dictionary of canonical
k-mers -- are 41,644 / 970 / 1,434 / 1,904 / 3,232.  With h = 3 and 2^22 counters the sketch's copy number equals the exact
count for every one of them (0 differ; 79 differ at 2^20, most at 2^16 and 2^6, always upwards), so the truth test runs at
2^22 and the collision tests at 2^16 and 2^6, where only GPU == model is asserted."""
import json
import os
import subprocess

import numpy as np
import pytest

import cn_model as CM
import helpers as H
import spectrum_model as SM
from test_gpu_reads_cascade import case as cascade_case  # noqa: F401  (the small read set of that file)
from test_gpu_spectrum import polish_case  # noqa: F401  (the small polish case of that file, with its counting filter)

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
TILE = 16384
E_ARG, E_OVERFLOW, E_UNSUPPORTED = -1, -4, -6
K, HASHES = CM.FIXTURE_K, 3
CLASSES = [41644, 970, 1434, 1904, 3232]


@pytest.fixture(scope="module")
def pol():
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    p.set_params(ntedit_amd.default_params())
    yield p
    p.close()


def spread(i):
    """counts for the k-mers of a test filter by index: a fifth not entered, the rest over 1..40"""
    return np.where(i % 5 == 0, 0, 1 + (i * 7) % 40)


@pytest.fixture(scope="module")
def draft():
    contigs, seg = CM.fixture_draft()
    data = SM.counting_filter(contigs, K, HASHES, 1 << 17, spread)
    return dict(contigs=contigs, seg=seg, data=data)


_models = {}


def model(batches, data, k, h, counters):
    """cn_model.side, computed once per (entries, filter, k, h, counters): the splits of one draft share it"""
    key = (tuple(CM.entries(batches)), data.tobytes(), k, h, counters)
    if key not in _models:
        _models[key] = CM.side(batches, data, k, h, counters)
    return _models[key]


def packed(entries):
    """one batch in the layout of include/ntedit_hip.h: the entries separated by a newline"""
    blob, offs, lens, _ = H.pack_batch([(b"e", e) for e in entries])
    return blob, np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint32)


def count(pol, sides, counters, cap=1 << 30):
    """both sides, each a list of batches of entries, through the stand-alone calls; returns per side (occ, w5, rows) and
    the info"""
    pol.set_cn(True, cap)
    for which, batches in enumerate(sides):
        for b in batches:
            pol.cn_append(which, *packed(b))
    pol.cn_finish(counters)
    got = []
    for which, batches in enumerate(sides):
        occ, w5 = pol.cn_table(which)
        got.append((occ, w5, pol.cn_rows(which, len(CM.entries(batches)))))
    return got, pol.cn_info()


def same(got, want, what=""):
    occ, w5, rows = got
    bad = np.argwhere(occ != want[0])
    assert bad.size == 0, "%s occ[%d][%d]: got %d, want %d (%d differ)" % (what, bad[0][0], bad[0][1], occ[tuple(bad[0])], want[0][tuple(bad[0])], len(bad))
    bad = np.flatnonzero(w5 != want[1])
    assert bad.size == 0, "%s w5[%d]: got %d, want %d (%d differ)" % (what, bad[0], w5[bad[0]], want[1][bad[0]], bad.size)
    rows = np.asarray(rows).astype(CM.ROW_DTYPE)
    assert rows.shape == want[2].shape, what
    bad = np.flatnonzero(rows != want[2])
    assert bad.size == 0, "%s entry %d: got %s, want %s (%d differ)" % (what, bad[0], rows[bad[0]], want[2][bad[0]], bad.size)


def identities(occ, rows):
    for c, f in enumerate(("cn1", "cn2", "cn3", "cn4", "cn5plus")):
        assert int(occ[c].sum()) == int(rows[f].sum()), f
    assert (rows["kmers"] == rows["cn1"] + rows["cn2"] + rows["cn3"] + rows["cn4"] + rows["cn5plus"]).all()


def check(pol, sides, data, k, h, counters):
    """GPU == model on both sides, the identities, the info; returns what count() returns"""
    got, info = count(pol, sides, counters)
    for which, batches in enumerate(sides):
        want = model(batches, data, k, h, counters)
        same(got[which], want, "side %d" % which)
        identities(got[which][0], got[which][2])
        assert info.nonzero[which] == want[3]
        assert info.batches[which] == sum(1 for b in batches if len(b)) and info.entries[which] == len(CM.entries(batches))
    assert (info.state, info.finished, info.counters) == (1, 1, counters)
    return got, info


# ------------------------------------------------------------------------------- 1. the truth: no collisions at 2^22
def test_truth_without_collisions(pol, draft):
    """model == the dictionary count with no exception, GPU == model, all five classes occupied, divisibility"""
    contigs, data = draft["contigs"], draft["data"]
    counters = 1 << 22
    want = model([contigs], data, K, HASHES, counters)
    occ_bf, w5_bf, rows_bf = CM.brute_force([contigs], data, K, HASHES)
    assert want[0].tolist() == occ_bf and want[1].tolist() == w5_bf and [tuple(int(x) for x in r) for r in want[2]] == rows_bf
    assert int(want[0].sum()) == 49184 and want[0].sum(axis=1).tolist() == CLASSES
    pol.set_filter(data, HASHES, K, counting=True)
    (before, after), info = check(pol, ([contigs], [contigs[::-1]]), data, K, HASHES, counters)
    occ, w5, rows = before
    assert occ.sum(axis=1).tolist() == CLASSES and all(n > 0 for n in CLASSES)
    for c in range(1, 5):
        assert not (occ[c - 1] % np.uint64(c)).any(), c  # (a k-mer of copy number c occurs c times, at one multiplicity)
    # the other side is the same draft in reverse order: the same table, the rows reversed
    assert (after[0] == occ).all() and (after[1] == w5).all() and (after[2] == rows[::-1]).all()
    # the reverse-complement copies land in the class of the forward ones: segment c is class min(c, 5) in every contig
    sketch = CM.side_sketch([contigs], K, HASHES, counters)
    for c, s in draft["seg"].items():
        for i in range(6):
            if i < c:
                at = contigs[i].find(CM.revcomp(s) if i % 2 else s)
                assert at > 0 and (CM.copy_numbers(contigs[i][at:at + 500], sketch, K, HASHES) == c).all(), (c, i)
    # the run of A: 376 occurrences of one k-mer sit at cn = 255 in 5plus, w5 takes RECIP[255] for each
    m_a = int(SM.multiplicities(b"A" * K, data, K, HASHES)[0])
    assert CM.copy_numbers(b"A" * K, sketch, K, HASHES)[0] == 255
    only_a = CM.side([[contigs[6]]], data, K, HASHES, counters)
    assert only_a[0][4][m_a] >= 376 and int(rows["cn5plus"][6]) == 376
    assert int(CM.RECIP[255]) == ((1 << 32) + 127) // 255
    six = occ[4].astype(object).sum() - 376  # (the occurrences of the segment held six times)
    assert int(w5.astype(object).sum()) == 376 * int(CM.RECIP[255]) + int(six) * int(CM.RECIP[6])
    # distinct k-mers: the library's rule == the model's; 376 occurrences at 255 count as one or two k-mers
    distinct = pol.cn_distinct(occ, w5)
    assert (distinct == CM.distinct(occ, w5)).all()
    assert distinct.sum(axis=1)[:4].tolist() == [41644, 485, 478, 476]
    assert abs(int(distinct[4].sum()) - (476 + 1)) <= 1
    assert info.ms[0] > 0 and info.ms[1] > 0 and info.ms[2] > 0 and info.ms[3] > 0


# ------------------------------------------------------------------------------- 2. batching
SPLITS = {1: [slice(0, 9)], 2: [slice(0, 1), slice(1, 9)], 5: [slice(0, 1), slice(1, 2), slice(2, 4), slice(4, 7), slice(7, 9)]}


@pytest.mark.parametrize("counters", [1 << 22, 1 << 16, 1 << 6])
def test_batch_splits_give_one_table(pol, draft, counters):
    """1, 2 and 5 batches, cut so that the copies of every segment fall into different batches: identical tables, the rows
    in entry order"""
    contigs, data = draft["contigs"], draft["data"]
    pol.set_filter(data, HASHES, K, counting=True)
    tables = []
    for n, cuts in sorted(SPLITS.items()):
        batches = [contigs[c] for c in cuts]
        assert len(batches) == n and CM.entries(batches) == contigs
        (before, after), _ = check(pol, (batches, [contigs]), data, K, HASHES, counters)
        tables.append(before)
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and (before[2] == after[2]).all()
    for t in tables[1:]:
        assert (t[0] == tables[0][0]).all() and (t[1] == tables[0][1]).all() and (t[2] == tables[0][2]).all()
    if counters < 1 << 22:  # (the collisions are there: the copy numbers differ from the truth, upwards)
        assert tables[0][0].sum(axis=1).tolist() != CLASSES and int(tables[0][0][0].sum()) < CLASSES[0]


# ------------------------------------------------------------------------------- 3. tile and stream edges
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_tile_and_stream_edges(pol, draft, shift):
    """the draft in one batch of more than three tiles of 16,384 starts; 1..3 bytes further on behind a short first entry
    the 64-start streams and the 16-byte staging chunks fall differently"""
    contigs, data = draft["contigs"], draft["data"]
    entries = list(contigs)
    if shift:
        entries = [contigs[0][100:100 + 30 + shift - 1]] + entries  # (with its separator: 30 + shift bytes in front)
    blob, offs, _ = packed(entries)
    assert len(blob) > 3 * TILE and (not shift or int(offs[1]) % 16 == (30 + shift) % 16)
    pol.set_filter(data, HASHES, K, counting=True)
    check(pol, ([entries], []), data, K, HASHES, 1 << 22)


# ------------------------------------------------------------------------------- 4. awkward layouts
def test_abutting_short_and_empty(pol, draft):
    """entries that abut without a separator (the window over the border is no k-mer of either), entries shorter than k,
    an empty batch, and a side with no batch at all"""
    contigs, data = draft["contigs"], draft["data"]
    a, b, c = contigs[0][5000:5300], contigs[0][5300:5700], contigs[1][5000:5500]  # (a + b: a piece of segment 2, cut in two)
    short = [contigs[2][:K - 1], contigs[2][:K], b""]
    blob = a + b + b"\n" + c + short[0] + short[1]
    offs = np.array([0, len(a), len(a) + len(b) + 1, len(a) + len(b) + 1 + len(c), len(a) + len(b) + 1 + len(c) + K - 1, len(blob)], dtype=np.uint64)
    lens = np.array([len(a), len(b), len(c), K - 1, K, 0], dtype=np.uint32)
    entries = [a, b, c] + short
    assert SM.entries_of(blob, offs, lens) == entries and len(blob) % 16 != 0
    pol.set_filter(data, HASHES, K, counting=True)
    for counters in (1 << 22, 1 << 6):
        want = model([entries], data, K, HASHES, counters)
        pol.set_cn(True)
        pol.cn_append(0, b"", [], [])  # (an empty batch: nothing is stored)
        pol.cn_append(0, blob, offs, lens)
        pol.cn_append(0, b"", [], [])
        pol.cn_finish(counters)
        occ, w5 = pol.cn_table(0)
        rows = pol.cn_rows(0, len(entries))
        same((occ, w5, rows), want)
        assert rows["kmers"].tolist() == [len(a) - K + 1, len(b) - K + 1, len(c) - K + 1, 0, 1, 0]
        info = pol.cn_info()
        assert (info.batches[0], info.batches[1], info.entries[1], info.bytes[1], info.nonzero[1]) == (1, 0, 0, 0, 0)
        # the side without a batch: zeros, and no row
        occ1, w51 = pol.cn_table(1)
        assert not occ1.any() and not w51.any() and pol.cn_rows(1, 0).size == 0
        with pytest.raises(Exception, match=r"\(%d\)" % E_ARG):
            pol.cn_rows(0, len(entries) + 1)
    assert int(want[0].sum()) == int(rows["kmers"].sum())
    # a sketch that is no power of two, or out of range
    for bad in (3 << 20, (1 << 22) + 1, 1 << 5, 1 << 37):
        with pytest.raises(Exception, match=r"\(%d\)" % E_ARG):
            pol.cn_finish(bad)
    # the default: the smallest power of two at or above 8 x the stored bytes, at least 2^20
    pol.cn_finish(0)
    assert pol.cn_info().counters == 1 << 20
    pol.set_cn(False)


# ------------------------------------------------------------------------------- 5. parameter matrix
@pytest.fixture(scope="module")
def matrix_entries():
    """20,000 bases in three entries: an N run, lower case, a run of 300 T, and a stretch of 400 bases held three times,
    once reverse-complemented; the length is no multiple of 16"""
    rng = np.random.default_rng(1401)
    g = bytearray(H.random_genome(rng, 20000))
    g[3000:3010] = b"N" * 10
    g[9000:9500] = bytes(g[9000:9500]).lower()
    g[15000:15300] = b"T" * 300
    g[12000:12400] = g[500:900]
    g[17000:17400] = CM.revcomp(bytes(g[500:900]))
    out = [bytes(g[:7003]), bytes(g[7003:13001]), bytes(g[13001:])]
    assert sum(map(len, out)) == 20000 and len(packed(out)[0]) % 16 != 0
    return out


@pytest.mark.parametrize("sketch", [1 << 6, 1 << 16, 1 << 22])
@pytest.mark.parametrize("counters", [1 << 17, 100003])
@pytest.mark.parametrize("k", [12, 25, 64, 200])
@pytest.mark.parametrize("h", [1, 3, 8])
def test_matrix(pol, matrix_entries, h, k, counters, sketch):
    data = SM.counting_filter(matrix_entries, k, h, counters, spread, pinned=[(b"T" * 300, 255)])
    pol.set_filter(data, h, k, counting=True)
    (before, after), _ = check(pol, ([matrix_entries], [matrix_entries[:1], matrix_entries[1:]]), data, k, h, sketch)
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert int((before[0].sum(axis=1) > 0).sum()) >= (3 if sketch == 1 << 22 else 1)


# ------------------------------------------------------------------------------- 6. against the plain spectrum
def test_identities_against_the_spectrum(pol, draft):
    """sum over the classes of occ[c][m] = k_spectrum's bins[m]; a row's kmers = the depth row's"""
    contigs, data = draft["contigs"], draft["data"]
    pol.set_filter(data, HASHES, K, counting=True)
    blob, offs, lens = packed(contigs)
    bins, depth = pol.spectrum_count(blob, offs, lens)
    for counters in (1 << 22, 1 << 16):
        (before, _), _ = count(pol, ([contigs], []), counters)
        assert (before[0].sum(axis=0) == bins).all()
        assert (before[2]["kmers"] == depth["kmers"]).all()
        identities(before[0], before[2])
    pol.set_cn(False)


# ------------------------------------------------------------------------------- 7. through polish_batch
def test_polish_batch_appends_both_sides(polish_case):
    import ntedit_amd
    recs, data, k, h = polish_case["recs"], polish_case["data"], polish_case["k"], polish_case["h"]
    blob, offs, lens, names = ntedit_amd.pack_batch(recs, 100)
    n = len(names)
    before_entries = SM.entries_of(blob, offs, lens)
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_params(ntedit_amd.default_params(min_threshold=2))
        pol.load_filter_file(polish_case["counts_bf"], 0)
        # the switch off: the reference results of this batch, and the getters answer NTEDIT_E_ARG
        pol.set_apply(ntedit_amd.APPLY_EDITED)
        res = pol.polish_batch(blob, offs, lens)
        ref_edited = [x.copy() for x in res.edited(n)]
        ref_stats = res.stats()
        ref_events = ref_stats.events
        res.free()
        for call in (lambda: pol.cn_table(0), lambda: pol.cn_rows(0, n), lambda: pol.cn_finish(0), lambda: pol.cn_append(0, blob, offs, lens)):
            with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\)" % E_ARG):
                call()
        info = pol.cn_info()
        assert (info.state, info.finished, info.batches[0], info.bytes[0]) == (0, 0, 0, 0)
        # reserve with the switch on leaves no trace
        pol.set_cn(True)
        pol.reserve(1 << 20, 16)
        info = pol.cn_info()
        assert (info.state, info.batches[0], info.batches[1], info.bytes[0], info.bytes[1]) == (1, 0, 0, 0, 0)
        # the switch on, no apply flag: the applier runs all the same, the polish results are what they were
        pol.set_apply(0)
        res = pol.polish_batch(blob, offs, lens)
        assert res.stats().events == ref_events
        with pytest.raises(ntedit_amd.NtEditHipError):
            res.edited(n)
        res.free()
        pol.set_apply(ntedit_amd.APPLY_EDITED)
        res = pol.polish_batch(blob, offs, lens)
        edited = res.edited(n)
        assert all((x == y).all() for x, y in zip(edited, ref_edited))
        res.free()
        ebytes, eoffs, elens = edited
        after_entries = SM.entries_of(ebytes.tobytes(), eoffs, elens)
        assert after_entries != before_entries  # (the polish edited something)
        info = pol.cn_info()
        assert (info.batches[0], info.batches[1], info.entries[0], info.entries[1]) == (2, 2, 2 * n, 2 * n)
        assert info.bytes[0] == 2 * len(blob) and info.bytes[1] == 2 * int(edited[0].size)
        counters = 1 << 22
        pol.cn_finish(counters)
        for which, entries in enumerate((before_entries, after_entries)):
            want = model([entries, entries], data, k, h, counters)
            occ, w5 = pol.cn_table(which)
            same((occ, w5, pol.cn_rows(which, 2 * n)), want, "side %d" % which)
            assert int(occ[0].sum()) < int(occ[1].sum())  # (the batch went in twice: copy number 2 at the least)
        # a new PRIMARY filter empties the store: the next round starts clean
        pol.load_filter_file(polish_case["counts_bf"], 0)
        info = pol.cn_info()
        assert (info.state, info.finished, info.batches[0], info.batches[1], info.bytes[0]) == (1, 0, 0, 0, 0)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\)" % E_ARG):
            pol.cn_table(0)
        # the cap: one byte too small for the second side's batch
        cap = len(blob) + int(edited[0].size)
        for this_cap, state in ((cap, 1), (cap - 1, 2)):
            pol.set_cn(True, this_cap)
            res = pol.polish_batch(blob, offs, lens)
            assert res.stats().events == ref_events and all((x == y).all() for x, y in zip(res.edited(n), ref_edited))
            res.free()
            info = pol.cn_info()
            assert info.state == state and info.cap == this_cap
            if state == 1:
                pol.cn_finish(counters)
                same(pol.cn_table(0) + (pol.cn_rows(0, n),), model([before_entries], data, k, h, counters))
            else:
                assert (info.batches[0], info.batches[1], info.bytes[0], info.bytes[1]) == (0, 0, 0, 0)
                with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\).*cap" % E_OVERFLOW):
                    pol.cn_finish(counters)
                assert "\n" not in pol._lib.ntedit_hip_last_error(pol._h).decode()
                # ... and the batches that follow are polished as ever
                res = pol.polish_batch(blob, offs, lens)
                assert res.stats().events == ref_events
                res.free()
                assert pol.cn_info().state == 2
        pol.set_cn(False)
        # a plain PRIMARY filter is refused before anything is polished; without a filter NTEDIT_E_ARG
        pol.set_apply(0)
        pol.set_cn(True)
        pol.load_filter_file(polish_case["bf"], 0)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\).*counting" % E_UNSUPPORTED):
            pol.polish_batch(blob, offs, lens)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\).*counting" % E_UNSUPPORTED):
            pol.cn_append(0, blob, offs, lens)
    finally:
        pol.close()
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_params(ntedit_amd.default_params())
        pol.set_cn(True)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(%d\)" % E_ARG):
            pol.polish_batch(blob, offs, lens)
    finally:
        pol.close()


# ------------------------------------------------------------------------------- 8. CLI
def _run(cmd):
    r = subprocess.run(["timeout", "-k", "10", "300"] + [str(c) for c in cmd], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(path):
    with open(str(path), "rb") as f:
        return f.read()


def _model_tables(prefix, bf_path, draft_path, edited_path, counters, min_len=100):
    """both tables under `prefix`, from the formatters applied to the model; returns the two sides"""
    import ntedit_amd
    bf = H.load_bf(str(bf_path))
    recs = [(n, s) for n, s in H.read_fasta(str(draft_path)) if len(s) >= min_len]
    edited = [s for _, s in H.read_fasta(str(edited_path))]
    assert len(edited) == len(recs)
    sides = [CM.side([x], bf["data"], bf["k"], bf["hash_num"], counters) for x in ([s for _, s in recs], edited)]
    pol = ntedit_amd.Polisher(0)
    try:
        pol.write_cn_tables(str(prefix), [n for n, _ in recs], CM.distinct(sides[0][0], sides[0][1]), CM.distinct(sides[1][0], sides[1][1]),
                            sides[0][2], sides[1][2])
    finally:
        pol.close()
    return sides


def _default_counters(*fasta_paths):
    """ntedit_hip_cn_finish(ctx, 0): the smallest power of two at or above 8 x the larger side's bytes, 2^20 at the least"""
    larger = max(sum(len(s) for _, s in H.read_fasta(str(p))) for p in fasta_paths)
    counters = 1 << 20
    while counters < 8 * larger:
        counters <<= 1
    return counters


def _summary(sides, counters, h):
    """the figures of the summary line and of the --report object, from the model"""
    out = {}
    for side, stage in zip(sides, ("before", "after")):
        d = CM.distinct(side[0], side[1])
        out["distinct_" + stage] = int(d.sum())
        out["single_copy_" + stage] = int(d[0].sum())
        out["occurrences_" + stage] = int(side[0].sum())
        out["multi_copy_occurrences_" + stage] = int(side[0][1:].sum())
        out["nonzero_" + stage] = side[3]
    out["sketch_counters"] = counters
    return out


def test_cli_cn(polish_case, tmp_path):
    base = [NTEDIT, "-f", polish_case["draft"], "-r", polish_case["counts_bf"], "-p", 2, "--spectrum"]
    plain = _run(base + ["-b", tmp_path / "plain"])
    cn = _run(base + ["-b", tmp_path / "out", "--cn", "--report"])
    counters = _default_counters(polish_case["draft"], tmp_path / "out_edited.fa")
    assert counters == 1 << 21  # (three contigs of 60 kbp)
    for suffix in ("_edited.fa", "_changes.tsv", "_spectrum.tsv", "_depth.tsv"):
        assert _read(tmp_path / ("plain" + suffix)) == _read(tmp_path / ("out" + suffix)), suffix
    assert not list(tmp_path.glob("plain*cn*")) and "k-mer copy numbers" not in plain.stdout
    sides = _model_tables(tmp_path / "model", polish_case["counts_bf"], polish_case["draft"], tmp_path / "out_edited.fa", counters)
    for suffix in ("_spectrum_cn.tsv", "_cn_contigs.tsv"):
        assert _read(tmp_path / ("out" + suffix)) == _read(tmp_path / ("model" + suffix)), suffix
    assert len(_read(tmp_path / "out_spectrum_cn.tsv").splitlines()) == 257
    assert _read(tmp_path / "out_cn_contigs.tsv").splitlines()[-1].startswith(b"#total\t")
    want = _summary(sides, counters, polish_case["h"])
    lines = [l for l in cn.stdout.splitlines() if l.startswith("k-mer copy numbers (k=25): before ")]
    assert len(lines) == 1 and str(tmp_path / "out_spectrum_cn.tsv") in lines[0] and str(tmp_path / "out_cn_contigs.tsv") in lines[0]
    assert "before %d distinct k-mers" % want["distinct_before"] in lines[0] and "after %d distinct k-mers" % want["distinct_after"] in lines[0]
    assert "sketch %d counters" % counters in lines[0]
    rep = [json.loads(l) for l in cn.stdout.splitlines() if l.startswith('{"cn": {')]
    assert len(rep) == 1
    rep = rep[0]["cn"]
    assert {f: rep[f] for f in want} == want and rep["state"] == "on"
    assert all(rep[f] > 0 for f in ("cn_count_before_ms", "spectrum_cn_before_ms", "cn_count_after_ms", "spectrum_cn_after_ms"))
    for stage, nz in (("before", want["nonzero_before"]), ("after", want["nonzero_after"])):
        assert abs(rep["inflated_" + stage] - (nz / counters) ** polish_case["h"]) <= 1e-5 * (nz / counters) ** polish_case["h"]
    # one batch per contig and a sketch of another size: the tables against the model at that size, the rows in order
    _run(base + ["-b", tmp_path / "small", "--cn", "--batch-bases", 1, "--cn_sketch", 1 << 22])
    _model_tables(tmp_path / "model22", polish_case["counts_bf"], polish_case["draft"], tmp_path / "small_edited.fa", 1 << 22)
    for suffix in ("_spectrum_cn.tsv", "_cn_contigs.tsv"):
        assert _read(tmp_path / ("small" + suffix)) == _read(tmp_path / ("model22" + suffix)), suffix
    # over the cap: the polish and every other output as usual, no cn file, one line on standard error, exit status 0
    over = _run(base + ["-b", tmp_path / "over", "--cn", "--cn_store", 1000, "--report"])
    for suffix in ("_edited.fa", "_changes.tsv", "_spectrum.tsv", "_depth.tsv"):
        assert _read(tmp_path / ("plain" + suffix)) == _read(tmp_path / ("over" + suffix)), suffix
    assert not list(tmp_path.glob("over*cn*")) and "k-mer copy numbers" not in over.stdout
    lines = [l for l in over.stderr.splitlines() if "--cn" in l]
    assert len(lines) == 1 and "--cn_store" in lines[0]
    rep = [json.loads(l) for l in over.stdout.splitlines() if l.startswith('{"cn": {')]
    assert len(rep) == 1 and rep[0]["cn"] == {"state": "over_cap", "store_cap": 1000}


def test_cli_cn_cascade(tmp_path, cascade_case):
    """`--reads --counts -k 40,25 --spectrum --cn`: a pair of tables per round under that round's prefix, each equal to
    the model against that round's saved filter -- the store starts clean in every round"""
    prefix = tmp_path / "out"
    r = _run([NTEDIT, "-f", cascade_case["draft"], "--reads", *cascade_case["files"]["plain"], "--counts", "--cutoff", 2, "--bf", 1 << 20, "-k", "40,25",
              "-b", prefix, "--spectrum", "--cn", "--save_bf", tmp_path / "f_{k}.bf"])
    assert r.stdout.count("k-mer copy numbers (k=") == 2
    rounds = ((40, cascade_case["draft"], "out_k40"), (25, tmp_path / "out_k40_edited.fa", "out"))
    for k, draft_path, name in rounds:
        # the default sketch: the smallest power of two at or above 8 x the larger side's bytes (2^21 for 200 kbp)
        counters = _default_counters(draft_path, tmp_path / (name + "_edited.fa"))
        line = [l for l in r.stdout.splitlines() if l.startswith("k-mer copy numbers (k=%d)" % k)]
        assert len(line) == 1 and "sketch %d counters" % counters in line[0] and counters == 1 << 21
        _model_tables(tmp_path / ("model_%d" % k), tmp_path / ("f_%d.bf" % k), draft_path, tmp_path / (name + "_edited.fa"), counters)
        for suffix in ("_spectrum_cn.tsv", "_cn_contigs.tsv"):
            assert _read(tmp_path / (name + suffix)) == _read(tmp_path / ("model_%d%s" % (k, suffix))), (k, suffix)
