"""The BGZF writer on the GPU: k_bz_deflate (ntedit_hip_bgzf_deflate) against the serial host model byte for byte and
back through the inflate kernel; a polish with NTEDIT_HIP_APPLY_BGZF against the _edited.fa text the renderer writes for
the same result; errors and lifetime; and `ntedit --bgzip` against runs without the flag (tests/deflate_corpus.py holds
the corpus; the CPU tier is tests/test_bgzf_deflate_cpu.py)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import bgzf_corpus as BC
import deflate_corpus as DC
import helpers as H
from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
E_ARG, E_OVERFLOW = -1, -4


@pytest.fixture(scope="module")
def pol():
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_sketch_free(p._h)  # (the inflate scratch of the round trip)
    p.close()


def read(path):
    with open(str(path), "rb") as f:
        return f.read()


# ---------------------------------------------------------------------------------- 1. the kernels
def test_host_bytes_equal_the_model_on_the_corpus(pol):
    want = DC.model_of_corpus()
    for name, data in DC.corpus():
        got = pol.bgzf_deflate(data)
        assert got == want[name], name
        st = pol.bgzf_info()
        assert (st.plain_bytes, st.bgzf_bytes, st.members) == (len(data), len(got), len(DC.blocks(data))), name
        assert st.ms_image == 0 and st.ms_deflate > 0 and st.ms_copy > 0
        if name in DC.STORED:
            assert st.stored_members == 1 and len(got) <= 65536
        if name in ("one_value", "fibonacci_21", "demo_draft", "fasta_39_blocks"):
            assert st.stored_members == 0, name


def test_device_bytes_equal_the_model_on_the_corpus(pol):
    """the corpus as one device buffer: every entry starts where the one before ended, at any alignment"""
    import torch
    want = DC.model_of_corpus()
    joined = b"".join(d for _, d in DC.corpus())
    dev = torch.frombuffer(bytearray(joined) + bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    at = 0
    seen = set()
    for name, data in DC.corpus():
        assert pol.bgzf_deflate(device_ptr=dev.data_ptr() + at, n=len(data)) == want[name], name
        seen.add(at % 4)
        at += len(data)
    assert seen == {0, 1, 2, 3}
    torch.cuda.synchronize()
    assert bytes(dev.cpu().numpy()[:len(joined)]) == joined, "the caller's device bytes were written to"


def test_empty_input_and_a_buffer_too_small(pol):
    n = ctypes.c_uint64(77)
    assert pol._lib.ntedit_hip_bgzf_deflate(pol._h, None, 0, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert pol.bgzf_info().members == 0
    name = "acgt_%d" % (2 * DC.BLOCK + 1)
    data, whole = dict(DC.corpus())[name], DC.model_of_corpus()[name]
    for cap in (0, len(whole) - 1):
        out = ctypes.create_string_buffer(b"\xEE" * (cap + 64), cap + 64)
        assert pol._lib.ntedit_hip_bgzf_deflate(pol._h, data, len(data), 0, out, cap, ctypes.byref(n)) == E_OVERFLOW
        assert n.value == len(whole) and out.raw == b"\xEE" * (cap + 64)
    assert pol._lib.ntedit_hip_bgzf_deflate(pol._h, data, len(data), 7, None, 0, ctypes.byref(n)) == E_ARG


def test_the_members_come_back_through_the_inflate_kernel(pol):
    """device round trip on the whole corpus: k_bz_deflate's members through k_bz_inflate, status 0 and the plain bytes"""
    import torch
    for name, data in DC.corpus():
        bgzf = pol.bgzf_deflate(data)
        rc, members, used = BC.walk(pol._lib, bgzf)
        assert rc == _lib.BGZF_END and used == len(bgzf) and len(members) == len(DC.blocks(data))
        out = torch.full((len(data) + BC.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        status = (ctypes.c_uint32 * len(members))()
        torch.cuda.synchronize()
        rc = pol._lib.ntedit_hip_reads_inflate_device(pol._h, bgzf, len(bgzf), 0, BC.table(members), len(members), out.data_ptr(),
                                                      len(data), status)
        assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
        torch.cuda.synchronize()
        host = bytes(out.cpu().numpy())
        assert list(status) == [0] * len(members), name
        assert host[:len(data)] == data and host[len(data):] == b"\xEE" * BC.GUARD, name


# ---------------------------------------------------------------------------------- 2. a polish with APPLY_BGZF
@pytest.fixture(scope="module")
def truth_case(tmp_path_factory, oracle_build):
    """a 400 kbp truth and its filter"""
    d = tmp_path_factory.mktemp("bgzf_polish")
    rng = np.random.default_rng(20261019)
    truth = H.random_genome(rng, 400000)
    H.write_fasta(str(d / "truth.fa"), [(b"t", truth)])
    H.mkbf([str(d / "truth.fa")], str(d / "t.bf"), k=25, hashes=3, nbytes=1 << 21)
    return dict(dir=d, rng=rng, truth=truth, bf=str(d / "t.bf"))


def _recs(case, which):
    rng, truth = np.random.default_rng(7), case["truth"]
    if which == "block_edge":
        # the first header line is 9 bytes + '>' and '\n': image offset 65,280 is base 65,269 of the first contig;
        # indels are dense in the 3 kbp around it and absent elsewhere
        a = H.mutate(rng, truth[:64000], p_sub=1e-3, p_ins=0, p_del=0)
        assert len(a) == 64000
        mid = H.mutate(rng, truth[64000:67000], p_sub=2e-3, p_ins=4e-3, p_del=4e-3)
        b = H.mutate(rng, truth[67000:150000], p_sub=1e-3, p_ins=0, p_del=0)
        return [(b"edge_ctg1", a + mid + b), (b"second with a comment", H.mutate(rng, truth[150000:190000], 2e-3))]
    recs = [(b"c20k", H.mutate(rng, truth[:20000], 2e-3, 3e-4, 3e-4)),
            (b"c200k some comment", H.mutate(rng, truth[20000:220000], 2e-3, 3e-4, 3e-4)),
            (b"c", H.mutate(rng, truth[220000:280000], 2e-3, 3e-4, 3e-4)),
            (b"short_one", truth[300000:300150])]
    if which == "snv":
        recs = recs[:1] + recs[2:]
    return recs


def _polisher(case, **par_kw):
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    p.load_filter_file(case["bf"], 0)
    p.set_params(ntedit_amd.default_params(**par_kw))
    return p


@pytest.mark.parametrize("which", ["contigs", "block_edge", "snv"])
def test_polish_with_apply_bgzf(tmp_path, truth_case, which):
    """gunzip of result_fa_bgzf = the bytes write_outputs_ex appends to fa_path for the same result; the same with
    APPLY_QV | APPLY_BGZF, with result_qv unchanged"""
    import ntedit_amd
    par_kw = dict(snv=1) if which == "snv" else {}
    p = _polisher(truth_case, **par_kw)
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(_recs(truth_case, which), p.params.min_contig_len)
        p.set_apply(ntedit_amd.APPLY_QV)
        res = p.polish_batch(blob, offs, lens)
        qv_alone = res.qv(len(names)).copy()
        res.free()
        for tag, flags in (("bgzf", ntedit_amd.APPLY_BGZF), ("qv_bgzf", ntedit_amd.APPLY_QV | ntedit_amd.APPLY_BGZF)):
            p.set_apply(flags)
            p.set_fa_names(names)
            res = p.polish_batch(blob, offs, lens)
            fa, tsv = str(tmp_path / (tag + ".fa")), str(tmp_path / (tag + ".tsv"))
            res.write(blob, offs, lens, names, fa, tsv)
            want = read(fa)
            gz, plain, members = res.fa_bgzf()
            assert DC.gunzip(gz) == want, tag
            assert plain == len(want) and members == len(DC.blocks(want)) and members >= 2
            DC.check_members(gz, want)
            assert gz == DC.model(p._lib, want)  # (the image is the text: the members are the model's of it)
            st = p.bgzf_info()
            assert (st.plain_bytes, st.bgzf_bytes, st.members, st.stored_members) == (len(want), len(gz), members, 0)
            assert st.ms_image > 0 and st.ms_deflate > 0 and st.ms_copy > 0
            if which != "snv":
                assert res.stats().insertions + res.stats().deletions > 0
            if which == "block_edge":
                ed, _ = res.edits(blob, offs, lens)
                near = ed[(ed["contig"] == 0) & (ed["kind"] != _lib.EDIT_SUB) & (abs(ed["draft_pos"].astype(np.int64) - 65269) < 1500)]
                assert near.size >= 2, "no indel near image offset 65,280: the case does not reach the block edge"
            if flags & ntedit_amd.APPLY_QV:
                assert np.array_equal(res.qv(len(names)), qv_alone)
            else:
                with pytest.raises(ntedit_amd.NtEditHipError, match="APPLY_EDITED"):
                    res.edited(len(names))
            res.free()
    finally:
        p.close()


def test_errors_and_lifetime(tmp_path, truth_case):
    import ntedit_amd
    p = _polisher(truth_case)
    try:
        recs = _recs(truth_case, "contigs")
        blob, offs, lens, names = ntedit_amd.pack_batch(recs, p.params.min_contig_len)
        # without the flag: the result refuses
        res = p.polish_batch(blob, offs, lens)
        with pytest.raises(ntedit_amd.NtEditHipError, match="APPLY_BGZF"):
            res.fa_bgzf()
        res.free()
        p.set_apply(ntedit_amd.APPLY_BGZF)
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(-1\).*no names"):
            p.polish_batch(blob, offs, lens)
        p.set_fa_names(names[:-1])
        with pytest.raises(ntedit_amd.NtEditHipError, match=r"\(-1\).*another number of names"):
            p.polish_batch(blob, offs, lens)
        # the names serve one call
        p.set_fa_names(names)
        first = p.polish_batch(blob, offs, lens)
        with pytest.raises(ntedit_amd.NtEditHipError, match="no names"):
            p.polish_batch(blob, offs, lens)
        gz1 = first.fa_bgzf()[0]
        ptr1 = ctypes.c_void_p()
        assert p._lib.ntedit_hip_result_fa_bgzf(first._h, ctypes.byref(ptr1), None, None, None) == 0
        # a second, smaller batch on the context: the first result's bytes stay, at their own address
        blob2, offs2, lens2, names2 = ntedit_amd.pack_batch(recs[2:3], 0)
        p.set_fa_names(names2)
        second = p.polish_batch(blob2, offs2, lens2)
        ptr2 = ctypes.c_void_p()
        n2 = ctypes.c_uint64()
        assert p._lib.ntedit_hip_result_fa_bgzf(second._h, ctypes.byref(ptr2), ctypes.byref(n2), None, None) == 0
        assert ptr1.value + len(gz1) <= ptr2.value or ptr2.value + n2.value <= ptr1.value
        assert first.fa_bgzf()[0] == gz1
        fa = str(tmp_path / "first.fa")
        first.write(blob, offs, lens, names, fa, None)
        assert DC.gunzip(gz1) == read(fa)
        fa2 = str(tmp_path / "second.fa")
        second.write(blob2, offs2, lens2, names2, fa2, None)
        assert DC.gunzip(second.fa_bgzf()[0]) == read(fa2)
        # freed: the buffers go back to the context, and the next result is right all the same
        first.free()
        second.free()
        p.set_fa_names(names)
        third = p.polish_batch(blob, offs, lens)
        assert third.fa_bgzf()[0] == gz1
        third.free()
        # an empty batch: no members
        p.set_fa_names([])
        empty = p.polish_batch(b"", np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        assert empty.fa_bgzf() == (b"", 0, 0)
        empty.free()
    finally:
        p.close()


# ---------------------------------------------------------------------------------- 3. the ntedit binary
def run(cmd, cwd):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300, cwd=str(cwd))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def same_tables(a, b):
    assert read(a + "_changes.tsv") == read(b + "_changes.tsv")
    assert H.vcf_body(a + "_variants.vcf") == H.vcf_body(b + "_variants.vcf")


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory, truth_case):
    """one small draft (seven contigs, one under -z) polished by the binary without the flag and with it"""
    d = tmp_path_factory.mktemp("bgzip_cli")
    rng, truth = np.random.default_rng(11), truth_case["truth"]
    recs = [(b"ctg%d" % i if i % 2 else b"ctg%d with a comment" % i, H.mutate(rng, truth[i * 50000:i * 50000 + 30000 + 3000 * i], 2e-3, 3e-4, 3e-4))
            for i in range(6)] + [(b"tiny", b"ACGT" * 10)]
    H.write_fasta(str(d / "draft.fa"), recs, width=70)
    base = [NTEDIT, "-f", "draft.fa", "-r", truth_case["bf"], "--report"]
    plain = run(base + ["-b", "plain"], d)
    gz = run(base + ["-b", "gz", "--bgzip"], d)
    return dict(dir=d, base=base, plain=plain, gz=gz, bf=truth_case["bf"])


def test_bgzip_holds_the_edited_draft(cli_case):
    d = cli_case["dir"]
    want = read(d / "plain_edited.fa")
    got = read(d / "gz_edited.fa.gz")
    assert len(want) > 3 * DC.BLOCK and not (d / "gz_edited.fa").exists() and not (d / "plain_edited.fa.gz").exists()
    assert DC.gunzip(got) == want
    assert got.endswith(DC.EOF_MEMBER)
    assert DC.check_members(got[:-28], want) == 0
    same_tables(str(d / "plain"), str(d / "gz"))
    # the summary line and --report
    line, = [l for l in cli_case["gz"].stdout.splitlines() if l.startswith("BGZF: ")]
    assert line.startswith("BGZF: %d plain bytes in %d BGZF bytes" % (len(want), len(got) - 28)) and "0 of them stored" in line
    rep, = [json.loads(l)["bgzip"] for l in cli_case["gz"].stdout.splitlines() if l.startswith('{"bgzip"')]
    assert (rep["plain_bytes"], rep["bgzf_bytes"], rep["members"], rep["stored_members"]) == (len(want), len(got) - 28, len(DC.blocks(want)), 0)
    assert rep["deflate_ms"] > 0


def test_without_the_flag_nothing_of_it_shows(cli_case):
    out = cli_case["plain"].stdout
    assert "bgzip" not in out and "BGZF" not in out and "fa.gz" not in out
    assert not any(l.startswith('{"bgzip"') for l in out.splitlines())


def test_the_compressed_draft_polishes_like_the_plain_one(cli_case):
    d = cli_case["dir"]
    base = [NTEDIT, "-r", cli_case["bf"]]
    run(base + ["-f", "plain_edited.fa", "-b", "again_plain"], d)
    run(base + ["-f", "gz_edited.fa.gz", "-b", "again_gz"], d)
    assert read(d / "again_plain_edited.fa") == read(d / "again_gz_edited.fa")
    same_tables(str(d / "again_plain"), str(d / "again_gz"))


def test_small_batches_give_other_members_and_the_same_text(cli_case):
    d = cli_case["dir"]
    r = run(cli_case["base"] + ["-b", "small", "--bgzip", "--batch-bases", 70000], d)
    got = read(d / "small_edited.fa.gz")
    assert got != read(d / "gz_edited.fa.gz")  # (every batch ends in a short member)
    assert DC.gunzip(got) == read(d / "plain_edited.fa") and got.endswith(DC.EOF_MEMBER)
    same_tables(str(d / "plain"), str(d / "small"))
    rep, = [json.loads(l)["bgzip"] for l in r.stdout.splitlines() if l.startswith('{"bgzip"')]
    assert rep["members"] == len(DC.walk(got)) - 1 > len(DC.blocks(read(d / "plain_edited.fa")))


def test_with_qv_and_snv(cli_case):
    d = cli_case["dir"]
    for tag, extra in (("qv", ["--qv", "--completeness"]), ("snv", ["-s", "1"])):
        run(cli_case["base"] + ["-b", tag + "_plain"] + extra, d)
        run(cli_case["base"] + ["-b", tag + "_gz", "--bgzip"] + extra, d)
        assert DC.gunzip(read(d / (tag + "_gz_edited.fa.gz"))) == read(d / (tag + "_plain_edited.fa")), tag
        same_tables(str(d / (tag + "_plain")), str(d / (tag + "_gz")))
    assert read(d / "qv_gz_qv.tsv") == read(d / "qv_plain_qv.tsv")
    assert read(d / "qv_gz_completeness.tsv") == read(d / "qv_plain_completeness.tsv")


def test_no_contig_passes_z(cli_case):
    d = cli_case["dir"]
    run(cli_case["base"] + ["-b", "none", "--bgzip", "-z", 1000000], d)
    assert read(d / "none_edited.fa.gz") == DC.EOF_MEMBER


def test_a_cascade_with_bgzip(tmp_path, truth_case):
    """-k 40,30 --bgzip against the same cascade without it: every round's tables, every round's text"""
    from reads_model import simulate_reads
    rng, truth = np.random.default_rng(13), truth_case["truth"][:100000]
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft[:70000]), (b"ctg2 x", draft[70000:])], width=80)
    H.write_fasta(str(tmp_path / "reads.fa"), [(b"r%d" % i, bytes(r)) for i, r in enumerate(simulate_reads(rng, truth, 20))])
    base = [NTEDIT, "-f", "draft.fa", "--reads", "reads.fa", "-k", "40,30", "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", 1 << 24]
    run(base + ["-b", "p"], tmp_path)
    run(base + ["-b", "g", "--bgzip"], tmp_path)
    for stem in ("_k40", ""):
        assert DC.gunzip(read(tmp_path / ("g%s_edited.fa.gz" % stem))) == read(tmp_path / ("p%s_edited.fa" % stem)), stem
        same_tables(str(tmp_path / ("p" + stem)), str(tmp_path / ("g" + stem)))
    assert read(tmp_path / "p_edited.fa") != read(tmp_path / "p_k40_edited.fa")
    assert not (tmp_path / "g_k40_edited.fa").exists()
