"""The reports behind the device applier (QV rows, completeness marks, intervals, the k-mer spectrum, the spectrum by copy
number, the BGZF writer) as state of one context: every report together gives what each gives alone, nothing of one filter
survives the next, ntedit_hip_reserve changes no result, the stand-alone calls give the stage's before side, and every
refusal of the stand-alone calls and of the result accessors keeps its return code and its text
(tests/golden/report_refusals.json, recorded from the library before the reports' state was grouped: DESIGN.md 9.22).

The oracle of the first cases is the same library with fewer switches on; its answers against the models are what
test_gpu_apply, _qv, _shared, _track, _spectrum, _cn and _bgzf_deflate establish.  Every comparison is exact equality."""
import ctypes
import json
import os
import types
import zlib

import numpy as np
import pytest

import helpers as H
import spectrum_model as SM
from reads_model import kmer_hashes

pytestmark = pytest.mark.gpu

K, HASHES = 25, 3
FILTER_BYTES = 1 << 17
TILE = 16384
CN_COUNTERS = 1 << 20
GOLDEN = os.path.join(H.ROOT, "tests", "golden", "report_refusals.json")


def _amd():
    import ntedit_amd
    return ntedit_amd


def make_shapes():
    """k = 25, h = 3; a plain and a counting PRIMARY filter of 2^17 bytes over a truth sequence; one batch of five entries
    cut from a mutated copy of it: k - 1 bases (no k-mer), k bases, about 3,000 with five substitutions and an insertion,
    3,000 unchanged, and 20,000 with a deletion, which cross the 16,384-base tile"""
    rng = np.random.default_rng(2209)
    truth = H.random_genome(rng, 30000)
    sub = lambda b: b"ACGT"[(b"ACGT".index(b) + 1) % 4]  # noqa: E731
    e2 = bytearray(truth[1000:4000])
    for q in (300, 900, 1500, 2100, 2700):
        e2[q] = sub(e2[q])
    e2[1200:1200] = bytes([sub(e2[1200])])
    e4 = bytearray(truth[9000:29001])
    del e4[12000]
    entries = [truth[100:100 + K - 1], truth[200:200 + K], bytes(e2), truth[5000:8000], bytes(e4)]
    assert [len(e) for e in entries] == [K - 1, K, 3001, 3000, 20000]
    blob, offs, lens, names = H.pack_batch([(b"entry%d some text" % i, e) for i, e in enumerate(entries)])
    offs, lens = np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint32)
    assert int(offs[4]) < TILE < int(offs[4]) + int(lens[4])
    hv = kmer_hashes(truth, K, HASHES)
    bits = np.zeros(FILTER_BYTES * 8, dtype=bool)
    bits[(hv % np.uint64(FILTER_BYTES * 8)).ravel().astype(np.int64)] = True
    plain = np.packbits(bits, bitorder="little")
    counting = SM.counting_filter([truth], K, HASHES, FILTER_BYTES, lambda i: 1 + (i * 7) % 60, pinned=[(truth[6000:6400], 255)])
    assert plain.size == FILTER_BYTES and counting.size == FILTER_BYTES
    return types.SimpleNamespace(blob=blob, offs=offs, lens=lens, names=names, n=len(lens), plain=plain, counting=counting)


@pytest.fixture(scope="module")
def shapes():
    return make_shapes()


@pytest.fixture(scope="module")
def pol():
    p = _amd().Polisher(0)
    yield p
    p.close()


def inflate(members):
    out = []
    while members:
        d = zlib.decompressobj(31)
        out.append(d.decompress(members))
        assert d.eof
        members = d.unused_data
    return b"".join(out)


def polish(pol, s, flags, spectrum=False, cn=False, names=True):
    """one polish of the batch with these switches; everything the switches give, as a dict of field -> value"""
    A = _amd()
    pol.set_apply(flags)
    pol.set_spectrum(spectrum)
    pol.set_cn(cn)  # (a store that begins holds nothing)
    if flags & A.APPLY_SHARED:
        pol.shared_begin()
        pol.shared_reset()
    if (flags & A.APPLY_BGZF) and names:
        pol.set_fa_names(s.names)
    res = pol.polish_batch(s.blob, s.offs, s.lens)
    out = {}
    if flags & A.APPLY_EDITED:
        out["edited"], out["edited_offs"], out["edited_lens"] = res.edited(s.n)
    if flags & A.APPLY_QV:
        out["qv"] = res.qv(s.n)
    if flags & A.APPLY_SHARED:
        out["marks0"], out["marks1"] = pol.shared_download(0), pol.shared_download(1)
    if flags & A.APPLY_TRACK:
        out["track0"], out["track1"] = res.track(0), res.track(1)
    if flags & A.APPLY_BGZF:
        members, plain, count = res.fa_bgzf()
        out["fa"] = inflate(members)
        assert len(out["fa"]) == plain and count >= 1
    if spectrum:
        out["bins0"], out["bins1"], out["depth"] = res.spectrum(0), res.spectrum(1), res.depth(s.n)
    if cn:
        pol.cn_finish(CN_COUNTERS)
        for which in (0, 1):
            out["cn_occ%d" % which], out["cn_w5%d" % which] = pol.cn_table(which)
            out["cn_rows%d" % which] = pol.cn_rows(which, s.n)
    res.free()
    pol.set_apply(0)
    pol.set_spectrum(False)
    pol.set_cn(False)
    return out


def same(got, want, keys=None):
    for key in keys if keys is not None else want:
        a, b = got[key], want[key]
        if isinstance(b, bytes):
            assert a == b, key
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), key
    assert keys is not None or set(got) == set(want)


def plain_group(pol, s):
    """every flag together, then each alone; returns the results of the polish with all of them"""
    A = _amd()
    flags = (A.APPLY_EDITED, A.APPLY_QV, A.APPLY_SHARED, A.APPLY_TRACK, A.APPLY_BGZF)
    together = polish(pol, s, sum(flags))
    assert len(together) == 9
    assert together["edited"].size and together["track0"].size and together["marks0"].any()
    assert int(together["qv"]["absent_before"].sum()) > int(together["qv"]["absent_after"].sum())
    seen = set()
    for f in flags:
        alone = polish(pol, s, f)
        same(together, alone, list(alone))
        seen |= set(alone)
    assert seen == set(together)
    return together


def counting_group(pol, s):
    A = _amd()
    together = polish(pol, s, A.APPLY_QV | A.APPLY_TRACK, spectrum=True, cn=True)
    assert len(together) == 12 and together["bins0"].sum() and together["cn_occ0"].any() and together["cn_occ1"].any()
    seen = set()
    for flags, spectrum, cn in ((A.APPLY_QV, False, False), (A.APPLY_TRACK, False, False), (0, True, False), (0, False, True)):
        alone = polish(pol, s, flags, spectrum=spectrum, cn=cn)
        same(together, alone, list(alone))
        seen |= set(alone)
    assert seen == set(together)
    return together


@pytest.fixture(scope="module")
def first(pol, shapes):
    """the plain group, then the counting group on the module's context, each once: (plain, counting)"""
    A = _amd()
    pol.set_params(A.default_params())
    pol.set_filter(shapes.plain, HASHES, K)
    plain = plain_group(pol, shapes)
    pol.shared_reset()
    pol.shared_mark(shapes.blob, 0)
    assert pol.shared_counts().marked_calls == 1
    pol.set_filter(shapes.counting, HASHES, K, counting=True)
    with pytest.raises(A.NtEditHipError):
        pol.shared_counts()  # (the marks were the plain filter's)
    counting = counting_group(pol, shapes)
    return plain, counting


# ------------------------------------------------------------------------------- 1. together equals alone
def test_together_equals_alone(pol, shapes, first):
    """the groups of `first` assert it; with -s 1 the stage screens both sides itself into the one bitmap"""
    A = _amd()
    plain, _ = first
    pol.set_filter(shapes.plain, HASHES, K)
    pol.set_params(A.default_params(snv=1))
    try:
        snv = plain_group(pol, shapes)
    finally:
        pol.set_params(A.default_params())
    same(snv, plain, ["marks0", "track0"])  # (the before side does not depend on the mode)
    assert (snv["qv"]["absent_before"] == plain["qv"]["absent_before"]).all()


# ------------------------------------------------------------------------------- 2. state across filters
def test_state_across_filters(pol, shapes, first):
    """a new PRIMARY filter takes the marks with it (`first` asserts that) and empties the draft store, which stays on; the
    groups then give what they gave before the other filter was there"""
    plain, counting = first
    pol.set_filter(shapes.counting, HASHES, K, counting=True)
    pol.set_cn(True)
    pol.cn_append(0, shapes.blob, shapes.offs, shapes.lens)
    st = pol.cn_info()
    assert (st.batches[0], st.batches[1]) == (1, 0)
    pol.set_filter(shapes.plain, HASHES, K)
    st = pol.cn_info()
    assert (st.batches[0], st.batches[1], st.state) == (0, 0, 1)
    pol.set_cn(False)
    same(plain_group(pol, shapes), plain)
    pol.set_filter(shapes.counting, HASHES, K, counting=True)
    same(counting_group(pol, shapes), counting)


# ------------------------------------------------------------------------------- 3. reserve changes nothing
def test_reserve_changes_nothing(shapes, first):
    A = _amd()
    plain, counting = first
    every = A.APPLY_EDITED | A.APPLY_QV | A.APPLY_SHARED | A.APPLY_TRACK | A.APPLY_BGZF
    p = A.Polisher(0)
    try:
        p.set_params(A.default_params())
        p.set_filter(shapes.plain, HASHES, K)
        p.set_apply(every)
        p.shared_begin()
        p.reserve(len(shapes.blob) * 2, 8)  # (BGZF on, no names: the warm-up asks for none)
        assert p.shared_counts().marked_calls == 0 and not p.shared_download(0).any() and not p.shared_download(1).any()
        p.set_fa_names(shapes.names)
        p.reserve(len(shapes.blob) * 2, 8)  # (and it does not use up the names of the next call)
        assert p.shared_counts().marked_calls == 0
        same(polish(p, shapes, every, names=False), plain)
        p.set_filter(shapes.counting, HASHES, K, counting=True)
        p.set_apply(A.APPLY_QV | A.APPLY_TRACK)
        p.set_spectrum(True)
        p.set_cn(True)
        p.reserve(len(shapes.blob) * 2, 8)
        st, sp = p.cn_info(), p.spectrum_info()
        assert (st.batches[0], st.batches[1], st.bytes[0], st.bytes[1]) == (0, 0, 0, 0)
        assert (sp.kmers[0], sp.kmers[1]) == (0, 0)
        same(polish(p, shapes, A.APPLY_QV | A.APPLY_TRACK, spectrum=True, cn=True), counting)
    finally:
        p.close()


# ------------------------------------------------------------------------------- 4. the empty batch
@pytest.mark.parametrize("n_entries", [0, 1])
def test_empty_batch(pol, shapes, first, n_entries):
    pol.set_filter(shapes.counting, HASHES, K, counting=True)
    pol.spectrum_count(shapes.blob, shapes.offs, shapes.lens)
    assert pol.spectrum_info().kmers[0] > 0
    pol.set_spectrum(True)
    try:
        res = pol.polish_batch(b"", np.zeros(n_entries, dtype=np.uint64), np.zeros(n_entries, dtype=np.uint32))
    finally:
        pol.set_spectrum(False)
    assert not res.spectrum(0).any() and not res.spectrum(1).any()
    depth = res.depth(n_entries)
    assert depth.shape == (n_entries,) and all(not depth[f].any() for f in depth.dtype.names)
    st = pol.spectrum_info()
    assert (st.ms[0], st.ms[1], st.kmers[0], st.kmers[1]) == (0.0, 0.0, 0, 0)
    res.free()


# ------------------------------------------------------------------------------- 5. stand-alone calls after a stage
def test_standalone_calls_after_a_stage(pol, shapes, first):
    """each on the batch of the stage, on the context whose buffers the stage has just used: the stage's before side, and
    zero in the figures of the other side"""
    A = _amd()
    s = shapes
    plain, counting = first
    pol.set_filter(s.plain, HASHES, K)
    stage = polish(pol, s, A.APPLY_QV | A.APPLY_SHARED | A.APPLY_TRACK)
    same(stage, plain, list(stage))
    got = pol.track_extract(pol.screen(s.blob), s.offs, s.lens, K, n=len(s.blob))
    assert got.dtype == stage["track0"].dtype and (got == stage["track0"]).all()
    st = pol.track_info()
    assert (st.intervals[0], st.intervals[1], st.bases[1], st.ms[1]) == (len(got), 0, 0, 0.0)
    pol.shared_reset()
    pol.shared_mark(s.blob, 0)
    assert (pol.shared_download(0) == stage["marks0"]).all() and not pol.shared_download(1).any()
    sc = pol.shared_counts()
    assert (sc.marked_calls, sc.ms_mark[1]) == (1, 0.0)
    pol.set_filter(s.counting, HASHES, K, counting=True)
    stage = polish(pol, s, A.APPLY_QV, spectrum=True, cn=True)
    same(stage, counting, list(stage))
    bins, rows = pol.spectrum_count(s.blob, s.offs, s.lens)
    assert (bins == stage["bins0"]).all()
    for f in ("kmers", "sum", "saturated"):
        assert (rows[f] == stage["depth"][f + "_before"]).all()
    sp = pol.spectrum_info()
    assert (sp.kmers[0], sp.kmers[1], sp.ms[1]) == (int(bins.sum()), 0, 0.0)
    pol.set_cn(True)
    try:
        pol.cn_append(0, s.blob, s.offs, s.lens)
        pol.cn_finish(CN_COUNTERS)
        occ, w5 = pol.cn_table(0)
        assert (occ == stage["cn_occ0"]).all() and (w5 == stage["cn_w50"]).all()
        assert (pol.cn_rows(0, s.n) == stage["cn_rows0"]).all()
        occ, w5 = pol.cn_table(1)
        ci = pol.cn_info()
        assert not occ.any() and not w5.any() and (ci.batches[1], ci.entries[1]) == (0, 0)
    finally:
        pol.set_cn(False)


# ------------------------------------------------------------------------------- 6. the refusal table
def refusal_rows(pol, s):
    """[label, return code, text] of every refused case of ntedit_hip_track_extract, _spectrum_count, _cn_append and
    _shared_mark (the text of ntedit_hip_last_error) and of the result accessors (ntedit_hip_result_last_error)"""
    A = _amd()
    lib, h = pol._lib, pol._h
    rows = []
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bases = ctypes.cast(ctypes.c_char_p(s.blob), ctypes.c_void_p)
    n, ne = len(s.blob), s.n
    offs, lens = vp(s.offs), vp(s.lens)
    broken = s.lens.copy()
    broken[1] = n  # (entry 1 runs past the batch)
    bitmap = np.full((n + 63) // 64, 0x0F0F0F0F0F0F0F0F, dtype=np.uint64)  # (a pattern: many intervals)
    found = ctypes.c_uint64()
    bins = np.zeros(256, dtype=np.uint64)

    def ctx(label, rc):
        assert rc != 0, label
        rows.append([label, rc, lib.ntedit_hip_last_error(h).decode()])

    def res(label, rc):
        assert rc != 0, label
        rows.append([label, rc, lib.ntedit_hip_result_last_error().decode()])

    # ---- the stand-alone calls
    pol.set_filter(s.plain, HASHES, K)
    te = lib.ntedit_hip_track_extract
    ctx("track_extract: null n", te(h, vp(bitmap), n, offs, lens, ne, K, None, 0, None))
    ctx("track_extract: null bitmap", te(h, None, n, offs, lens, ne, K, None, 0, ctypes.byref(found)))
    ctx("track_extract: null offs", te(h, vp(bitmap), n, None, lens, ne, K, None, 0, ctypes.byref(found)))
    ctx("track_extract: null out", te(h, vp(bitmap), n, offs, lens, ne, K, None, 4, ctypes.byref(found)))
    ctx("track_extract: k = 0", te(h, vp(bitmap), n, offs, lens, ne, 0, None, 0, ctypes.byref(found)))
    ctx("track_extract: layout", te(h, vp(bitmap), n, offs, vp(broken), ne, K, None, 0, ctypes.byref(found)))
    ctx("track_extract: too small", te(h, vp(bitmap), n, offs, lens, ne, K, None, 0, ctypes.byref(found)))
    assert found.value > 0
    sm = lib.ntedit_hip_shared_mark
    ctx("shared_mark: which = 2", sm(h, 2, bases, n, 0))
    ctx("shared_mark: null bases", sm(h, 0, None, n, 0))
    ctx("shared_mark: on_device = 2", sm(h, 0, bases, n, 2))
    sc = lib.ntedit_hip_spectrum_count
    ctx("spectrum_count: plain filter", sc(h, bases, n, 0, offs, lens, ne, vp(bins), None))
    ca = lib.ntedit_hip_cn_append
    ctx("cn_append: switched off", ca(h, 0, bases, n, 0, offs, lens, ne))
    pol.set_cn(True)
    ctx("cn_append: plain filter", ca(h, 0, bases, n, 0, offs, lens, ne))
    pol.set_cn(False)
    pol.set_filter(s.counting, HASHES, K, counting=True)
    ctx("shared_mark: counting filter", sm(h, 0, bases, n, 0))
    ctx("spectrum_count: null bins", sc(h, bases, n, 0, offs, lens, ne, None, None))
    ctx("spectrum_count: null bases", sc(h, None, n, 0, offs, lens, ne, vp(bins), None))
    ctx("spectrum_count: null lens", sc(h, bases, n, 0, offs, None, ne, vp(bins), None))
    ctx("spectrum_count: on_device = 2", sc(h, bases, n, 2, offs, lens, ne, vp(bins), None))
    ctx("spectrum_count: layout", sc(h, bases, n, 0, offs, vp(broken), ne, vp(bins), None))
    pol.set_cn(True)
    ctx("cn_append: which = 2", ca(h, 2, bases, n, 0, offs, lens, ne))
    ctx("cn_append: null offs", ca(h, 0, bases, n, 0, None, lens, ne))
    ctx("cn_append: on_device = 2", ca(h, 0, bases, n, 2, offs, lens, ne))
    ctx("cn_append: layout", ca(h, 0, bases, n, 0, offs, vp(broken), ne))
    pol.set_cn(False)

    # ---- the accessors: a result with nothing on, a result with everything a plain filter gives
    pol.set_filter(s.plain, HASHES, K)
    pol.set_apply(0)
    r0 = pol.polish_batch(s.blob, s.offs, s.lens)
    pol.set_apply(A.APPLY_EDITED | A.APPLY_QV | A.APPLY_TRACK | A.APPLY_BGZF)
    pol.set_fa_names(s.names)
    r1 = pol.polish_batch(s.blob, s.offs, s.lens)
    pol.set_apply(0)
    pol.set_filter(s.counting, HASHES, K, counting=True)
    pol.set_spectrum(True)
    r2 = pol.polish_batch(s.blob, s.offs, s.lens)
    pol.set_spectrum(False)
    big = np.zeros(4 * ne + 64, dtype=np.uint64)
    ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
    qv = lib.ntedit_hip_result_qv
    res("result_qv: null result", qv(None, vp(big), ne))
    res("result_qv: null rows", qv(r1._h, None, ne))
    res("result_qv: flag off", qv(r0._h, vp(big), ne))
    res("result_qv: entries", qv(r1._h, vp(big), ne + 1))
    dp = lib.ntedit_hip_result_depth
    res("result_depth: null rows", dp(r2._h, None, ne))
    res("result_depth: switch off", dp(r1._h, vp(big), ne))
    res("result_depth: entries", dp(r2._h, vp(big), ne - 1))
    tr = lib.ntedit_hip_result_track
    res("result_track: null n", tr(r1._h, 0, None, 0, None))
    res("result_track: which = 2", tr(r1._h, 2, None, 0, ctypes.byref(found)))
    res("result_track: null out", tr(r1._h, 0, None, 4, ctypes.byref(found)))
    res("result_track: flag off", tr(r0._h, 0, None, 0, ctypes.byref(found)))
    found.value = 0
    res("result_track: too small", tr(r1._h, 0, None, 0, ctypes.byref(found)))
    rows[-1].append(found.value)  # (NTEDIT_E_OVERFLOW sets *n)
    sp = lib.ntedit_hip_result_spectrum
    res("result_spectrum: null bins", sp(r2._h, 0, None))
    res("result_spectrum: which = 2", sp(r2._h, 2, vp(bins)))
    res("result_spectrum: switch off", sp(r1._h, 0, vp(bins)))
    bz = lib.ntedit_hip_result_fa_bgzf
    res("result_fa_bgzf: null result", bz(None, ctypes.byref(ptr), ctypes.byref(nb), None, None))
    res("result_fa_bgzf: flag off", bz(r0._h, ctypes.byref(ptr), ctypes.byref(nb), None, None))
    ed = lib.ntedit_hip_result_edited_device
    res("result_edited_device: null dev_ptr", ed(r1._h, None, ctypes.byref(nb), None, None, ne))
    res("result_edited_device: flag off", ed(r0._h, ctypes.byref(ptr), ctypes.byref(nb), None, None, ne))
    res("result_edited_device: entries", ed(r1._h, ctypes.byref(ptr), ctypes.byref(nb), vp(big), vp(big), ne + 1))
    eh = lib.ntedit_hip_result_edited
    res("result_edited: flag off", eh(r0._h, vp(big), 8, ctypes.byref(nb), None, None, ne))
    nb.value = 0
    res("result_edited: too small", eh(r1._h, vp(big), 8, ctypes.byref(nb), None, None, ne))
    rows[-1].append(nb.value)
    for r in (r0, r1, r2):
        r.free()
    return rows


def test_refusal_table(pol, shapes, first):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = refusal_rows(pol, shapes)
    assert len(got) == len(want) and len(got) >= 40
    for g, w in zip(got, want):
        assert g == w
