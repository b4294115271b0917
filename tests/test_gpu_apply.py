"""The device applier (ntedit_hip_set_apply, NTEDIT_HIP_APPLY_EDITED): the edited contigs in HBM.

Result.edited() must hold, entry by entry, the sequence lines of the product's own _edited.fa (the host renderer is the
specification) and of the oracle's; the caller's batch stays untouched; without the flag nothing changes."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def _hip_params(**kw):
    import ntedit_amd
    return ntedit_amd.default_params(**kw)


def _par_kw(hp):
    return {f[0]: getattr(hp, f[0]) for f in hp._fields_}


def _polisher(bf, rep=None, **par_kw):
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    pol.load_filter_file(bf, 0)
    if rep:
        pol.load_filter_file(rep, 1)
    pol.set_params(_hip_params(**par_kw))
    return pol


def _entries(buf, offs, lens):
    raw = buf.tobytes()
    return [raw[int(o):int(o) + int(l)] for o, l in zip(offs, lens)]


def _check_layout(buf, offs, lens):
    """entry after entry, one separator byte behind each"""
    pos = 0
    for o, l in zip(offs, lens):
        assert int(o) == pos
        pos += int(l) + 1
        assert buf[pos - 1] == ord("\n")
    assert buf.size == pos


def _device_copy(blob):
    import torch
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def check_applier(tmp, recs, bf, rep=None, oracle=None, **par_kw):
    """recs polished with APPLY_EDITED from host memory and from the caller's device memory: edited() against the
    product's _edited.fa and, when given, the oracle's (a list of sequences)"""
    import ntedit_amd
    import torch
    pol = _polisher(bf, rep, **par_kw)
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, pol.params.min_contig_len)
        pol.set_apply(ntedit_amd.APPLY_EDITED)
        out = {}
        for how in ("host", "device"):
            if how == "host":
                res = pol.polish_batch(blob, offs, lens)
            else:
                dev = _device_copy(blob)
                res = pol.polish_batch(None, offs, lens, device_ptr=dev.data_ptr(), n=len(blob))
                torch.cuda.synchronize()
                assert dev.cpu().numpy().tobytes() == blob, "the caller's device batch was written to"
            fa = os.path.join(str(tmp), "apply_%s_edited.fa" % how)
            open(fa, "wb").close()
            res.write(blob, offs, lens, names, fa, None, append=True)
            want = [s for _, s in H.read_fasta(fa)]
            buf, e_offs, e_lens = res.edited(len(names))
            got = _entries(buf, e_offs, e_lens)
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, "%s input, entry %d (%s): %d bytes against %d, first difference at %s" % (
                    how, i, names[i], len(g), len(w), next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), None))
            _check_layout(buf, e_offs, e_lens)
            if oracle is not None:
                assert got == oracle, "%s input: edited() differs from the oracle's _edited.fa" % how
            info = pol.apply_info()
            assert info.bytes == buf.size and info.pieces >= 2 * len(names)
            assert info.events_applied == res.stats().events_applied
            out[how] = got
            res.free()
        assert out["host"] == out["device"]
        return out["host"]
    finally:
        pol.close()


def _oracle_sequences(tmp, case, hp):
    H.run_oracle(case["draft"], case["bf"], hp, os.path.join(str(tmp), "o"), case["rep"])
    return [s for _, s in H.read_fasta(os.path.join(str(tmp), "o_edited.fa"))]


MAKE_CASE_CONFIGS = [dict(), dict(mode=1), dict(mode=2), dict(mask=1), dict(snv=1), dict(max_insertions=0, max_deletions=0)]


@pytest.mark.parametrize("par_kw", MAKE_CASE_CONFIGS, ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()) or "defaults")
def test_applier_make_case(tmp_path, oracle_build, par_kw):
    case = H.make_case(str(tmp_path), 31001, flavor="N lower")
    hp = H.default_params(**par_kw)
    got = check_applier(tmp_path, H.read_fasta(case["draft"]), case["bf"], oracle=_oracle_sequences(tmp_path, case, hp), **par_kw)
    assert len(got) == 3  # (the 40-base record is shorter than -z)


@pytest.mark.parametrize("which", ["sweep_rich", "tail", "contig_end", "many"])
def test_applier_shapes(tmp_path, oracle_build, which):
    par_kw = {}
    if which == "sweep_rich":
        case, par_kw = H.make_sweep_rich_case(str(tmp_path)), dict(min_threshold=2)
    elif which == "tail":
        case, par_kw = H.make_tail_case(str(tmp_path)), dict(snv=1, mask=1, min_contig_len=0)
    elif which == "contig_end":
        case = H.make_contig_end_case(str(tmp_path))
    else:
        case = H.make_many_case(str(tmp_path))
    hp = H.default_params(**par_kw)
    check_applier(tmp_path, H.read_fasta(case["draft"]), case["bf"], oracle=_oracle_sequences(tmp_path, case, hp), **par_kw)


def test_applier_golden_cases(tmp_path):
    import test_golden as TG
    assert {"counting_p2", "secondary_ratio"} <= set(TG.CASES) and len(TG.CASES) == 5
    for name in TG.CASES:
        d = os.path.join(H.GOLDEN, "cases", name)
        hp = TG.params_from_file(os.path.join(d, "params.txt"))
        rep = os.path.join(d, "secondary.bf")
        want = [s for _, s in H.read_fasta(os.path.join(d, "expected_edited.fa"))]
        sub = tmp_path / name
        sub.mkdir()
        check_applier(sub, H.read_fasta(os.path.join(d, "draft.fa")), os.path.join(d, "filter.bf"),
                      rep if os.path.exists(rep) else None, oracle=want, **_par_kw(hp))


# ------------------------------------------------------------------------------------------------- copy edges
def _edge_truth(tmp, n, seed=77):
    rng = np.random.default_rng(seed)
    truth = H.random_genome(rng, n)
    H.write_fasta(os.path.join(str(tmp), "truth.fa"), [(b"t", truth)])
    H.mkbf([os.path.join(str(tmp), "truth.fa")], os.path.join(str(tmp), "t.bf"), k=25, hashes=3, nbytes=1 << 20)
    return rng, truth, os.path.join(str(tmp), "t.bf")


def _first_insertion(bf, recs):
    """draft position of the first inserted run: the position node in front of it ends one base earlier"""
    import ntedit_amd
    from ntedit_amd import _lib
    pol = _polisher(bf)
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, 0)
        res = pol.polish_batch(blob, offs, lens)
        ed, _ = res.edits(blob, offs, lens)
        ins = ed[(ed["kind"] == _lib.EDIT_INS) & (ed["contig"] == 0)]
        assert ins.size, "the planted deletion was not repaired"
        return int(ins["draft_pos"][0])
    finally:
        pol.close()


@pytest.mark.parametrize("edge", ["piece_ends_on_last_byte", "piece_starts_on_first_byte"])
def test_copy_tile_edges(tmp_path, oracle_build, edge):
    """A clean stretch of four copy tiles, then a base the draft lacks: the applier's first piece is the position node in
    front of the inserted base.  The error is moved until that piece ends on the last byte of the fourth tile, or until
    the inserted byte is that last byte and the piece behind it starts on the first byte of the fifth."""
    from ntedit_amd import _lib
    tile = int(_lib.load().ntedit_hip_apply_tile())
    rng, truth, bf = _edge_truth(tmp_path, 4 * tile + 6000)
    target = 4 * tile if edge == "piece_ends_on_last_byte" else 4 * tile - 1
    cut = target

    def draft(at):
        return [(b"edge", truth[:at] + truth[at + 1:]), (b"other", H.mutate(rng, truth[1000:9000], 2e-3))]
    where = _first_insertion(bf, draft(cut))
    cut += target - where
    recs = draft(cut)
    assert _first_insertion(bf, recs) == target
    got = check_applier(tmp_path, recs, bf, min_contig_len=0)
    assert got[0] == truth  # (the one error of the contig is repaired)
    assert got[0][target - 1:target + 2] == truth[target - 1:target + 2]


def test_overtaken_events_clean_contig_and_k_bases(tmp_path, oracle_build):
    """substitutions every 2k bases or closer (many events start inside an earlier event's run: start < cover), a contig
    without any event between two edited ones, and -- a batch of its own -- one contig of exactly k bases"""
    rng, truth, bf = _edge_truth(tmp_path, 120000, seed=78)
    recs = [(b"dense", H.mutate(rng, truth[:40000], p_sub=2e-2, p_ins=0, p_del=0)),
            (b"clean", truth[40000:80000]),
            (b"dense2 with comment", H.mutate(rng, truth[80000:], p_sub=2e-2, p_ins=1e-3, p_del=1e-3))]
    H.write_fasta(os.path.join(str(tmp_path), "d.fa"), recs)
    hp = H.default_params(min_contig_len=0)
    want = _oracle_sequences(tmp_path, dict(draft=os.path.join(str(tmp_path), "d.fa"), bf=bf, rep=None), hp)
    got = check_applier(tmp_path, recs, bf, oracle=want, min_contig_len=0)
    assert got[1] == truth[40000:80000]
    import ntedit_amd
    pol = _polisher(bf, min_contig_len=0)
    try:
        blob, offs, lens, _ = ntedit_amd.pack_batch(recs, 0)
        res = pol.polish_batch(blob, offs, lens)
        st = res.stats()
        res.write(blob, offs, lens, [r[0] for r in recs], None, None)
        assert res.stats().events_applied < st.events, "no event was overtaken: the case does not reach start < cover"
    finally:
        pol.close()
    one = [(b"k_bases", truth[5000:5025])]
    assert check_applier(tmp_path, one, bf, min_contig_len=0) == [truth[5000:5025]]


# ------------------------------------------------------------------------------------------------ the flag off
def test_flag_off_changes_nothing(tmp_path, oracle_build):
    import ntedit_amd
    case = H.make_case(str(tmp_path), 31002)
    recs = H.read_fasta(case["draft"])
    pol = _polisher(case["bf"])
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, pol.params.min_contig_len)

        def outputs(tag):
            res = pol.polish_batch(blob, offs, lens)
            fa, tsv = str(tmp_path / (tag + ".fa")), str(tmp_path / (tag + ".tsv"))
            res.write(blob, offs, lens, names, fa, tsv)
            st = res.stats()
            with pytest.raises(ntedit_amd.NtEditHipError, match="APPLY_EDITED"):
                res.edited(len(names))
            with pytest.raises(ntedit_amd.NtEditHipError, match="APPLY_QV"):
                res.qv(len(names))
            res.free()
            counts = (st.bases, st.absent_kmers, st.events, st.events_deferred, st.events_applied, st.substitutions,
                      st.insertions, st.deletions, st.events_skipped, st.screen_launches, st.screen_binned)
            return open(fa, "rb").read(), open(tsv, "rb").read(), counts
        before = outputs("a")
        pol.set_apply(ntedit_amd.APPLY_EDITED | ntedit_amd.APPLY_QV)
        res = pol.polish_batch(blob, offs, lens)
        assert res.edited(len(names))[0].size > 0
        res.free()
        pol.set_apply(0)
        assert outputs("b") == before
    finally:
        pol.close()


def test_second_batch_does_not_alias_the_first(tmp_path, oracle_build):
    """a smaller batch behind a larger one on one context: both results keep their own edited bases"""
    import ntedit_amd
    case = H.make_case(str(tmp_path), 31003)
    recs = H.read_fasta(case["draft"])
    pol = _polisher(case["bf"])
    try:
        pol.set_apply(ntedit_amd.APPLY_EDITED)
        results, wants = [], []
        for part in (recs, recs[1:2]):
            blob, offs, lens, names = ntedit_amd.pack_batch(part, pol.params.min_contig_len)
            res = pol.polish_batch(blob, offs, lens)
            fa = str(tmp_path / ("p%d.fa" % len(results)))
            res.write(blob, offs, lens, names, fa, None)
            results.append((res, len(names)))
            wants.append([s for _, s in H.read_fasta(fa)])
        ptrs = []
        for (res, n), want in zip(results, wants):
            buf, e_offs, e_lens = res.edited(n)
            assert _entries(buf, e_offs, e_lens) == want
            ptr, nb, _, _ = res.edited_device(n)
            ptrs.append((ptr, nb))
        (p0, n0), (p1, n1) = ptrs
        assert p0 + n0 <= p1 or p1 + n1 <= p0, "the two results share device memory"
        for res, _ in results:
            res.free()
    finally:
        pol.close()


# ------------------------------------------------------------------------------------- the reports together
CN_COUNTERS = 1 << 20
TOGETHER_CASES = {
    "plain": ("plain", [dict()]),
    "plain_snv": ("plain", [dict(snv=1)]),
    "counting_p2": ("counting", [dict(min_threshold=2), dict(min_threshold=2, snv=1)]),
}


@pytest.fixture(scope="module")
def together_cases(tmp_path_factory, oracle_build):
    """the drafts of H.make_case (60 kbp, three contigs): one with its plain filter, one with spectrum_model's counting filter"""
    import spectrum_model as SM
    plain = H.make_case(str(tmp_path_factory.mktemp("together_plain")), 31004, flavor="N lower")
    plain["recs"] = H.read_fasta(plain["draft"])
    counting = SM.polish_case(str(tmp_path_factory.mktemp("together_counting")))
    counting["bf"] = counting["counts_bf"]
    return dict(plain=plain, counting=counting)


def _reports_of(kind):
    """the reports a filter of that kind takes: name -> apply flag (None: a switch of its own)"""
    import ntedit_amd
    reports = dict(edited=ntedit_amd.APPLY_EDITED, qv=ntedit_amd.APPLY_QV, track=ntedit_amd.APPLY_TRACK, bgzf=ntedit_amd.APPLY_BGZF)
    if kind == "plain":
        reports["shared"] = ntedit_amd.APPLY_SHARED
    else:
        reports.update(spectrum=None, cn=None)
    return reports


def _polish_with(pol, batch, on):
    """one polish_batch with the reports `on` (a dict of _reports_of) and no other; returns what each of them gives, the
    events of the call and the applier's byte count"""
    blob, offs, lens, names = batch
    n = len(names)
    pol.set_apply(sum(f for f in on.values() if f))
    pol.set_spectrum("spectrum" in on)
    pol.set_cn("cn" in on)  # (switching it on or off empties the store)
    if "shared" in on:
        pol.shared_begin()
        pol.shared_reset()
    if "bgzf" in on:
        pol.set_fa_names(names)
    res = pol.polish_batch(blob, offs, lens)
    return _gather(pol, res, n, on)


def _gather(pol, res, n, on):
    got = dict(events=int(res.stats().events), bytes=int(pol.apply_info().bytes))
    if "edited" in on:
        got["edited"] = [x.tobytes() for x in res.edited(n)]
    if "qv" in on:
        got["qv"] = res.qv(n).tobytes()
    if "track" in on:
        got["track"] = [res.track(0).tobytes(), res.track(1).tobytes()]
    if "bgzf" in on:
        got["bgzf"] = res.fa_bgzf()
    if "shared" in on:
        got["shared"] = [pol.shared_download(0).tobytes(), pol.shared_download(1).tobytes()]
    if "spectrum" in on:
        got["spectrum"] = [res.spectrum(0).tobytes(), res.spectrum(1).tobytes(), res.depth(n).tobytes()]
    if "cn" in on:
        pol.cn_finish(CN_COUNTERS)
        got["cn"] = [x.tobytes() for which in (0, 1) for x in pol.cn_table(which) + (pol.cn_rows(which, n),)]
    res.free()
    return got


_together = {}


def _everything_on(case, kind, par_kw):
    """the results of one batch polished with every report of its filter's kind on; computed once per configuration"""
    import ntedit_amd
    key = (kind,) + tuple(sorted(par_kw.items()))
    if key not in _together:
        pol = _polisher(case["bf"], **par_kw)
        try:
            batch = ntedit_amd.pack_batch(case["recs"], pol.params.min_contig_len)
            _together[key] = _polish_with(pol, batch, _reports_of(kind))
        finally:
            pol.close()
    return _together[key]


@pytest.mark.parametrize("name", list(TOGETHER_CASES))
def test_reports_together_equal_each_alone(together_cases, name):
    """every report alone, then all of them in one call: each gives the same bytes either way, the polish finds the same
    events, and the applier writes as many bytes as edited() holds"""
    import ntedit_amd
    kind, configs = TOGETHER_CASES[name]
    case = together_cases[kind]
    for par_kw in configs:
        reports = _reports_of(kind)
        together = _everything_on(case, kind, par_kw)
        edited_size = len(together["edited"][0])
        assert edited_size > 0 and together["bytes"] == edited_size and together["events"] > 0
        assert sorted(together) == sorted(list(reports) + ["events", "bytes"])
        pol = _polisher(case["bf"], **par_kw)
        try:
            batch = ntedit_amd.pack_batch(case["recs"], pol.params.min_contig_len)
            for report, flag in reports.items():
                alone = _polish_with(pol, batch, {report: flag})
                assert sorted(alone) == sorted([report, "events", "bytes"])
                assert alone[report] == together[report], "%s %s: alone and together differ" % (par_kw, report)
                assert alone["events"] == together["events"], (par_kw, report)
                assert alone["bytes"] == edited_size, (par_kw, report)
        finally:
            pol.close()
        # the reports say something: intervals on both sides, marks, a non-empty BGZF text
        assert all(len(x) > 0 for x in together["track"]) and together["bgzf"][1] > edited_size
        if kind == "plain":
            assert all(any(x) for x in together["shared"])


@pytest.mark.parametrize("kind", ["plain", "counting"])
def test_reserve_with_everything_on_leaves_no_trace(together_cases, kind):
    """every switch on and the names set, then reserve(): its warm-up batch leaves no mark, nothing in the store and no
    spectrum, and the next polish_batch runs with the switches and the names as they were set"""
    import ntedit_amd
    case = together_cases[kind]
    par_kw = dict() if kind == "plain" else dict(min_threshold=2)
    reports = _reports_of(kind)
    want = _everything_on(case, kind, par_kw)
    pol = _polisher(case["bf"], **par_kw)
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(case["recs"], pol.params.min_contig_len)
        pol.set_apply(sum(f for f in reports.values() if f))
        pol.set_spectrum("spectrum" in reports)
        pol.set_cn("cn" in reports)
        if kind == "plain":
            pol.shared_begin()
        pol.set_fa_names(names)
        pol.reserve(1 << 20, 16)
        if kind == "plain":
            st = pol.shared_counts()
            assert (st.marked_calls, st.shared_set[0], st.shared_set[1]) == (0, 0, 0)
        else:
            info = pol.cn_info()
            assert (info.state, info.batches[0], info.batches[1], info.bytes[0], info.bytes[1]) == (1, 0, 0, 0, 0)
            sp = pol.spectrum_info()
            assert (sp.kmers[0], sp.kmers[1], sp.ms[0], sp.ms[1]) == (0, 0, 0.0, 0.0)
        # the flags are what they were, and so are the names: every report of the next call is there and equals the reference
        res = pol.polish_batch(blob, offs, lens)
        assert _gather(pol, res, len(names), reports) == want
    finally:
        pol.close()
