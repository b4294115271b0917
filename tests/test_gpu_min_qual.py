"""--min_qual on the GPU: the masking copy of the text parser and the masking decode of the BAM unit against their serial
models and the twin's counts, at the shapes where a quality address can go wrong; the same through BGZF; an unclean chunk
handed back; and the four front ends by the twin -- the filter built with --min_qual Q from a file equals, byte for byte,
the filter built without it from that file with the low-quality bases rewritten to N (tests/min_qual_twin.py; the CPU tier
is tests/test_min_qual_cpu.py)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import bam_corpus as BAM
import helpers as H
import min_qual_twin as MQ
import parse_corpus as PC
from ntedit_amd import _lib
from reads_model import simulate_reads

pytestmark = pytest.mark.gpu

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
K = MQ.K
Q = 20
T = _lib.PARSE_TILE
GUARD = 256
MASK_LINE = re.compile(r"--min_qual (\d+): (\d+) of (\d+) bases with a quality masked")


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_reads_set_min_qual(p._h, 0)
    p._lib.ntedit_hip_reads_bam_set_segment(p._h, 0)
    p._lib.ntedit_hip_sketch_free(p._h)  # (the parser's scratch)
    p.close()


def counts(pol):
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert pol._lib.ntedit_hip_reads_min_qual_info(pol._h, a, b) == 0
    return a.value, b.value


def device_parse(pol, raw, k, q):
    """ntedit_hip_reads_parse_device under set_min_qual(q) -> (the result, the text when clean, what the counts grew by)"""
    import torch
    lib = pol._lib
    assert lib.ntedit_hip_reads_set_min_qual(pol._h, q) == 0
    cap = (len(raw) + 15) // 16 * 16
    text = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsParseResult()
    before = counts(pol)
    torch.cuda.synchronize()
    rc = lib.ntedit_hip_reads_parse_device(pol._h, raw, len(raw), 0, k, text.data_ptr(), cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    after = counts(pol)
    host = bytes(text.cpu().numpy())
    assert host[cap:] == b"\xEE" * GUARD
    return res, host[:res.text_len] if res.clean else None, (after[0] - before[0], after[1] - before[1])


def check_parse(pol, recs, raw, k=K, qs=(Q,)):
    """the device under q against the model under q -- text, reads, bases -- and against the twin's counts"""
    lib = pol._lib
    for q in qs:
        mres, mtext = MQ.parse_model_q(lib, raw, k, q)
        res, text, grew = device_parse(pol, raw, k, q)
        assert mres.clean == 1 and res.clean == 1, (res.broken, mres.broken)
        assert text == mtext and (res.reads, res.bases, res.text_len) == (mres.reads, mres.bases, mres.text_len)
        assert mtext == MQ.text_of(MQ.mask_records(recs, q), k)
        assert grew == MQ.count_masked(recs, q, k), q
    # ... and off is the text without the flag, with nothing counted
    res, text, grew = device_parse(pol, raw, k, 0)
    assert text == PC.model(lib, raw, k)[1] and grew == (0, 0)


def records_of_size(rng, size):
    """FASTQ records of 100 bases whose 4-line layout is exactly `size` bytes"""
    recs, used = [], 0
    while size - used > 500:
        recs += MQ.draw_records(rng, 1, lengths=(100, 100), tag=b"s%d_" % len(recs))
        used = len(MQ.fastq(recs))
    left = size - used  # one more record "@t..\nS\n+\nQ\n": name + 2 n + 6 bytes
    name = b"t" if left % 2 == 1 else b"tt"
    n = (left - 6 - len(name)) // 2
    recs.append((name, bytes(rng.choice(b"ACGT") for _ in range(n)), MQ.draw_qual(rng, n)))
    assert len(MQ.fastq(recs)) == size
    return recs


# ---------------------------------------------------------------------------------- 1. the masking copy
@pytest.mark.parametrize("size", [T - 1, T, T + 1])
def test_chunks_of_one_tile_and_its_neighbours(pol, size):
    recs = records_of_size(random.Random(size), size)
    check_parse(pol, recs, MQ.fastq(recs), qs=MQ.QS)


@pytest.mark.parametrize("newline_at", [T - 1, T - 3, 2 * T - 1])
def test_a_sequence_line_ends_a_tile_and_its_qualities_start_the_next(pol, newline_at):
    """the sequence line's '\\n' on a tile's last byte ('+' opens the next tile), and two bytes earlier (the quality line
    opens it)"""
    rng = random.Random(newline_at)
    first = MQ.draw_records(rng, 1, lengths=(300, 300), tag=b"first")
    name = b"edge" + b"x" * (newline_at - len(MQ.fastq(first)) - 1 - 4 - 1 - 200)  # "@" name "\n" 200 bases "\n"
    recs = first + [(name, bytes(rng.choice(b"ACGT") for _ in range(200)), MQ.draw_qual(rng, 200, 0.3))]
    recs += MQ.draw_records(rng, 40, lengths=(1, 400), tag=b"after")
    raw = MQ.fastq(recs)
    assert raw[newline_at] == 10 and raw[newline_at + 1:newline_at + 3] == b"+\n"
    check_parse(pol, recs, raw)


def test_one_record_of_300_kb(pol):
    """the quality line lies many tiles behind the bases a lane holds"""
    rng = np.random.default_rng(4)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 300_000))
    qual = bytes(np.where(rng.random(300_000) < 0.1, rng.integers(33, 33 + Q, 300_000), rng.integers(33 + Q, 127, 300_000)).astype(np.uint8))
    recs = [(b"short", seq[:200], qual[:200]), (b"long", seq, qual), (b"after", seq[:77], qual[5:82])]
    check_parse(pol, recs, MQ.fastq(recs))


@pytest.fixture(scope="module")
def ten_thousand():
    """10^4 reads of 1..400 bases: lanes cross several line ends within their 16 bytes"""
    rng = np.random.default_rng(5)
    genome = H.random_genome(rng, 50000)
    lengths = rng.integers(1, 401, 10_000)
    starts = rng.integers(0, 50000 - 400, 10_000)
    recs = []
    for i, (s, n) in enumerate(zip(starts, lengths)):
        low = rng.random(n) < 0.1
        qual = np.where(low, rng.integers(33, 33 + Q, n), rng.integers(33 + Q, 127, n)).astype(np.uint8)
        recs.append((b"read%d" % i, genome[s:s + n], bytes(qual)))
    return recs


def test_ten_thousand_reads_of_every_length(pol, ten_thousand):
    check_parse(pol, ten_thousand, MQ.fastq(ten_thousand))


def test_the_same_through_bgzf(pol, ten_thousand, tmp_path):
    """the 10^4-read set as BGZF (tests/bgzf_corpus.py): its members inflated in HBM in groups, each chunk cut at its last
    record start on the device and parsed where it lies, the rest carried in front of the next group, as the pass does it
    -- the texts' concatenation, reads, bases and counts against the model and the twin; then the pass itself over the
    file, with no chunk handed back to the host parser"""
    import torch
    import bgzf_corpus as BZ
    lib, h = pol._lib, pol._h
    recs = ten_thousand
    raw = MQ.fastq(recs)
    blob = BZ.bgzf(raw, block=20000)
    why, members, used = BZ.walk(lib, blob)
    assert why == _lib.BGZF_END and used == len(blob) and sum(m.n_out for m in members) == len(raw) and len(members) > 100
    want_text = MQ.text_of(MQ.mask_records(recs, Q), K)
    mres, mtext = MQ.parse_model_q(lib, raw, K, Q)
    assert mres.clean == 1 and mtext == want_text
    assert lib.ntedit_hip_reads_set_min_qual(h, Q) == 0
    before = counts(pol)
    group, tail, text, reads, bases, chunks = 37, b"", b"", 0, 0, 0  # (37 members of 20,000 bytes: chunks of about 45 tiles)
    members = [m for m in members if m.n_out]  # (the end-of-file member)
    for g in range(0, len(members), group):
        ms = members[g:g + group]
        first, n_out = ms[0], sum(m.n_out for m in ms)
        part = [_lib.BgzfMember(in_off=m.in_off, out_off=len(tail) + m.out_off - first.out_off, n_in=m.n_in, n_out=m.n_out, crc=m.crc)
                for m in ms]
        total = len(tail) + n_out
        buf = torch.zeros((total + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
        if tail:
            buf[:len(tail)] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).cuda()
        status = (ctypes.c_uint32 * len(part))()
        torch.cuda.synchronize()
        assert lib.ntedit_hip_reads_inflate_device(h, blob, len(blob), 0, BZ.table(part), len(part), buf.data_ptr(), total, status) == 0
        assert not any(status)
        cut = ctypes.c_uint64(total)
        if g + group < len(members):
            assert lib.ntedit_hip_reads_last_start_device(h, buf.data_ptr(), total, 1, cut) == 0
            assert 0 < cut.value < total
        out = torch.full(((cut.value + 15) // 16 * 16 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        res = _lib.ReadsParseResult()
        rc = lib.ntedit_hip_reads_parse_device(h, buf.data_ptr(), cut.value, 1, K, out.data_ptr(), (cut.value + 15) // 16 * 16, res)
        assert rc == 0 and res.clean == 1, (res.broken, lib.ntedit_hip_reads_last_error(h))
        torch.cuda.synchronize()
        text += bytes(out[:res.text_len].cpu().numpy())
        reads, bases, chunks = reads + res.reads, bases + res.bases, chunks + 1
        tail = bytes(buf[cut.value:total].cpu().numpy())
    after = counts(pol)
    assert chunks > 5 and text == want_text and (reads, bases) == (mres.reads, mres.bases)
    assert (after[0] - before[0], after[1] - before[1]) == MQ.count_masked(recs, Q, K)
    # the pass over the file: the sketch of the BGZF file under the flag is the sketch of the twin, plain and without it
    (tmp_path / "r.fq.gz").write_bytes(blob)
    (tmp_path / "twin.fq").write_bytes(MQ.mask(raw, Q))
    sketches = {}
    for name, path, parse, q in (("bgzf", "r.fq.gz", 1, Q), ("twin", "twin.fq", 0, 0)):
        assert lib.ntedit_hip_sketch_alloc(h, 1 << 22, 3, K) == 0
        assert lib.ntedit_hip_reads_set_device_parse(h, parse) == 0 and lib.ntedit_hip_reads_set_min_qual(h, q) == 0
        files = (ctypes.c_char_p * 1)(str(tmp_path / path).encode())
        st = _lib.ReadsPassStats()
        rc = lib.ntedit_hip_reads_pass(h, _lib.READS_PASS_COUNT, files, (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)((1 << 64) - 1), 1,
                                       1 << 18, 0, st, None, None)
        assert rc == 0, lib.ntedit_hip_reads_last_error(h)
        sk = np.zeros(1 << 22, dtype=np.uint8)
        assert lib.ntedit_hip_sketch_download(h, sk.ctypes.data) == 0
        sketches[name] = (sk, st.bases, counts(pol))
        if parse:
            ps, zs = _lib.ReadsParseStats(), _lib.ReadsInflateStats()
            assert lib.ntedit_hip_reads_parse_info(h, ps) == 0 and lib.ntedit_hip_reads_inflate_info(h, zs) == 0
            assert ps.fallback_chunks == 0 and ps.broken == 0 and ps.host_files == 0 and ps.device_chunks > 5
            assert zs.files == 1 and zs.handed_back == 0 and zs.raw_bytes == len(raw)
        lib.ntedit_hip_sketch_free(h)
    lib.ntedit_hip_reads_set_device_parse(h, 0)
    assert (sketches["bgzf"][0] == sketches["twin"][0]).all() and sketches["bgzf"][0].any()
    assert sketches["bgzf"][1] == sketches["twin"][1] == mres.bases
    assert sketches["bgzf"][2] == MQ.count_masked(recs, Q, K) and sketches["twin"][2] == (0, 0)


def test_a_chunk_whose_last_line_has_no_newline(pol):
    recs = MQ.draw_records(random.Random(8), 30, lengths=(1, 200), low=0.3)
    raw = MQ.fastq(recs, last_eol=False)
    assert raw[-1:] != b"\n"
    check_parse(pol, recs, raw, qs=MQ.QS)


def test_a_fasta_chunk_is_never_masked(pol):
    raw = PC.well_formed()["fasta_wrapped_60"]
    res, text, grew = device_parse(pol, raw, 12, 93)
    assert res.clean == 1 and text == PC.model(pol._lib, raw, 12)[1] and grew == (0, 0)


def test_the_setting_is_checked_and_outlives_the_sketch(pol):
    lib, h = pol._lib, pol._h
    assert lib.ntedit_hip_reads_set_min_qual(h, 94) == _lib.E_ARG
    assert lib.ntedit_hip_reads_set_min_qual(h, 93) == 0
    assert lib.ntedit_hip_sketch_alloc(h, 1 << 20, 3, K) == 0
    assert lib.ntedit_hip_sketch_reset(h, 1 << 20, 3, 40) == 0
    lib.ntedit_hip_sketch_free(h)
    recs = MQ.draw_records(random.Random(2), 5, lengths=(30, 60))
    raw = MQ.fastq(recs)
    import torch
    text = torch.zeros(len(raw) + 16, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsParseResult()
    assert lib.ntedit_hip_reads_parse_device(h, raw, len(raw), 0, K, text.data_ptr(), (len(raw) + 15) // 16 * 16, res) == 0
    torch.cuda.synchronize()
    assert bytes(text.cpu().numpy())[:res.text_len] == MQ.text_of(MQ.mask_records(recs, 93), K)  # (still 93)


# ---------------------------------------------------------------------------------- 2. an unclean chunk
def test_an_unclean_chunk_is_reported_as_without_the_flag(pol):
    """a quality line one byte short: the same verdict with the setting on (the copy has run by then, bounded)"""
    raw = PC.odd()["fastq_quality_one_short"] + MQ.fastq(MQ.draw_records(random.Random(1), 50, lengths=(1, 300)))
    off, _, _ = device_parse(pol, raw, 12, 0)
    on, text, grew = device_parse(pol, raw, 12, Q)
    assert off.clean == on.clean == 0 and off.broken == on.broken == _lib.PARSE_BAD["fq_qual"] and text is None
    assert grew == (0, 0)
    # and the next chunk on the same context parses as if nothing had happened
    recs = MQ.draw_records(random.Random(9), 20, lengths=(1, 200))
    check_parse(pol, recs, MQ.fastq(recs))


# ---------------------------------------------------------------------------------- 3. the masking decode
def device_bam(pol, raw, q, segment, min_len=K):
    import torch
    lib = pol._lib
    assert lib.ntedit_hip_reads_bam_set_segment(pol._h, segment) == 0 and lib.ntedit_hip_reads_set_min_qual(pol._h, q) == 0
    cap = len(raw)
    out = torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsBamResult()
    before = counts(pol)
    torch.cuda.synchronize()
    rc = lib.ntedit_hip_reads_bam_device(pol._h, raw, len(raw), 0, 1, min_len, out.data_ptr() + GUARD, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    after = counts(pol)
    host = bytes(out.cpu().numpy())
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + cap:] == b"\xEE" * GUARD
    return BAM.result_dict(res), host[GUARD:GUARD + res.text_len], (after[0] - before[0], after[1] - before[1])


def bam_sets():
    """150-base reads; 15-20 kb reads; short reads of odd and even lengths (a record boundary inside a lane's 16 text
    bytes); in each a record with 0xFF qualities between two ordinary ones"""
    rng = random.Random(21)
    sets = {}
    for name, lengths, n in (("reads_150", (150, 150), 120), ("reads_15_to_20_kb", (15000, 20000), 4), ("short_odd_and_even", (1, 31), 200)):
        recs = MQ.draw_records(rng, n, lengths=lengths, low=0.15)
        recs.insert(1, (b"absent", bytes(rng.choice(b"ACGT") for _ in range(lengths[0] | 1)), MQ.NO_QUAL))
        sets[name] = recs
    return sets


@pytest.mark.parametrize("segment", [64, 256, 4096])
@pytest.mark.parametrize("name", list(bam_sets()))
def test_the_bam_decode_equals_the_model(pol, name, segment):
    lib = pol._lib
    recs = bam_sets()[name]
    _, raw = MQ.bam_of(recs)
    min_len = 1 if name == "short_odd_and_even" else K
    assert any(len(s) % 2 for _, s, _ in recs)
    for q in MQ.QS:
        want, want_text = MQ.bam_model_q(lib, raw, min_len, q)
        got, text, grew = device_bam(pol, raw, q, segment, min_len)
        assert got == BAM.result_dict(want) and text == want_text, (name, q)
        assert text == MQ.text_of(MQ.mask_records(recs, q), min_len)
        assert grew == MQ.count_masked(recs, q, min_len)
    got, text, grew = device_bam(pol, raw, 0, segment, min_len)
    assert text == BAM.model(lib, raw, 1, min_len)[2] and grew == (0, 0)


# ---------------------------------------------------------------------------------- 4. the tool, by the twin
def run(args, timeout=900):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def masked_of(r):
    return [(int(q), int(m), int(b)) for q, m, b in MASK_LINE.findall(r.stderr)]


@pytest.fixture(scope="module")
def read_set(tmp_path_factory):
    """2 Mbases of 150-base reads at 30x, qualities drawn so that about a tenth of the bases fall below Q = 20; the file,
    its twin (those bases rewritten to N), the same set as BAM, and what the pass has to report"""
    d = tmp_path_factory.mktemp("min_qual")
    rng = np.random.default_rng(77)
    truth = H.random_genome(rng, 66_000)
    reads = simulate_reads(rng, truth, 30)
    # as sequencers err: a 3' tail of 0..28 low-quality bases per read, and one base in a hundred anywhere (scattered
    # evenly, a tenth of the bases would leave 0.9^25 of the 25-mers whole, and --solid no valley to find)
    tail = rng.integers(0, 29, reads.shape[0])
    low = (np.arange(reads.shape[1])[None, :] >= reads.shape[1] - tail[:, None]) | (rng.random(reads.shape) < 0.01)
    qual = np.where(low, rng.integers(33, 33 + Q, reads.shape), rng.integers(33 + Q, 127, reads.shape)).astype(np.uint8)
    recs = [(b"r%d" % i, bytes(s), bytes(c)) for i, (s, c) in enumerate(zip(reads, qual))]
    assert 0.05 < low.mean() < 0.15 and 1_900_000 < reads.size < 2_100_000
    (d / "r.fq").write_bytes(MQ.fastq(recs))
    (d / "twin.fq").write_bytes(MQ.fastq(MQ.mask_records(recs, Q)))
    assert (d / "twin.fq").read_bytes() == MQ.mask((d / "r.fq").read_bytes(), Q)
    (d / "r.bam").write_bytes(MQ.bam_of(recs)[0])
    (d / "r.fq.gz").write_bytes(BAM.bgzf((d / "r.fq").read_bytes()))
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:40000]), (b"ctg2", draft[40000:])], width=80)
    return dict(dir=d, fq=d / "r.fq", twin=d / "twin.fq", bam=d / "r.bam", bgzf=d / "r.fq.gz", draft=d / "draft.fa",
                counts=MQ.count_masked(recs, Q, K))


BUILD = ["-k", K, "-c", 2, "--bf", 2_000_000]


def three_ways(read_set, tag, args, outputs=("",), k_args=BUILD):
    """the tool with --min_qual on the file, host parser and --gpu_parse, and without it on the twin: every output equal"""
    d = read_set["dir"]
    runs = {}
    for name, src, flags in (("host", read_set["fq"], ["--min_qual", Q]), ("gpu", read_set["fq"], ["--min_qual", Q, "--gpu_parse"]),
                             ("twin", read_set["twin"], [])):
        out = d / ("%s_%s.bf" % (tag, name))
        a = [str(x).replace("{out}", str(out)) for x in args]
        runs[name] = (run([TOOL, "--reads", src, "-o", out] + k_args + a + flags), out)
    for suffix in outputs:
        twin = open(str(runs["twin"][1]) + suffix, "rb").read()
        assert open(str(runs["host"][1]) + suffix, "rb").read() == twin, (tag, suffix, "host parser")
        assert open(str(runs["gpu"][1]) + suffix, "rb").read() == twin, (tag, suffix, "--gpu_parse")
    assert not masked_of(runs["twin"][0]) and "--min_qual" not in runs["twin"][0].stdout
    for name in ("host", "gpu"):
        lines = masked_of(runs[name][0])
        assert lines and all(l == (Q, read_set["counts"][1], read_set["counts"][0]) for l in lines), (name, lines)
    assert "unclean" not in runs["gpu"][0].stderr
    return runs


def test_the_filter_equals_the_twins(read_set):
    runs = three_ways(read_set, "cut", [])
    assert len(masked_of(runs["gpu"][0])) == 2  # (pass 1 and pass 2 both read the file)
    # the flag matters: a k-mer of the unmasked set's filter is absent from the masked one
    plain = read_set["dir"] / "plain.bf"
    run([TOOL, "--reads", read_set["fq"], "-o", plain] + BUILD)
    a = np.frombuffer(plain.read_bytes(), dtype=np.uint8)
    b = np.frombuffer(runs["twin"][1].read_bytes(), dtype=np.uint8)
    assert a.size == b.size and int(np.bitwise_and(a, np.bitwise_not(b)).any())


def test_solid_and_hist_equal_the_twins(read_set):
    runs = three_ways(read_set, "solid", ["--solid", "--hist", "{out}.hist"], outputs=("", ".hist"), k_args=["-k", K, "--bf", 2_000_000])
    cut = {name: re.search(r"--solid: minimum k-mer count (\d+)", r.stderr).group(1) for name, (r, _) in runs.items()}
    assert len(set(cut.values())) == 1, cut


def test_the_reject_filter_equals_the_twins(read_set):
    three_ways(read_set, "reject", ["--reject_cutoff", 30, "--reject_bf", 500_000, "--reject_out", "{out}.reject"],
               outputs=("", ".reject"))


def test_the_bam_and_the_bgzf_fastq_equal_the_twin(read_set):
    d = read_set["dir"]
    twin = d / "bam_twin.bf"
    run([TOOL, "--reads", read_set["twin"], "-o", twin] + BUILD)
    for name, src in (("bam", read_set["bam"]), ("bgzf", read_set["bgzf"])):
        out = d / ("%s.bf" % name)
        r = run([TOOL, "--reads", src, "-o", out, "--gpu_parse", "--min_qual", Q] + BUILD)
        assert out.read_bytes() == twin.read_bytes(), name
        assert masked_of(r) == [(Q, read_set["counts"][1], read_set["counts"][0])] * 2, name
        # well-formed input: nothing goes back to the host parser
        assert "unclean" not in r.stderr and ("0 files handed back" in r.stderr or name == "bam"), r.stderr[-3000:]


def test_an_unclean_chunk_is_handed_back_and_still_masked(read_set, tmp_path):
    """CR LF line ends, which the device refuses: the host parser finishes the range, masked by the same rule"""
    recs = MQ.draw_records(random.Random(31), 3000, lengths=(20, 151), low=0.2)
    (tmp_path / "crlf.fq").write_bytes(MQ.fastq(recs, eol=b"\r\n"))
    (tmp_path / "twin.fq").write_bytes(MQ.fastq(MQ.mask_records(recs, Q)))
    small = ["-k", K, "-c", 1, "--bf", 300_000, "--batch_bytes", 65536]
    r = run([TOOL, "--reads", tmp_path / "crlf.fq", "-o", tmp_path / "a.bf", "--gpu_parse", "--min_qual", Q] + small)
    run([TOOL, "--reads", tmp_path / "twin.fq", "-o", tmp_path / "b.bf"] + small)
    assert (tmp_path / "a.bf").read_bytes() == (tmp_path / "b.bf").read_bytes()
    assert "1 unclean chunks sent the rest of their ranges to the host parser (a carriage return)" in r.stderr
    want = MQ.count_masked(recs, Q, K)
    assert masked_of(r) == [(Q, want[1], want[0])] * 2
    # a quality line one byte short in mid-file: unclean as without the flag, and the host parser's reads, masked, up to it
    cut = MQ.fastq(recs[:2000]) + PC.odd()["fastq_quality_one_short"] + MQ.fastq(recs[2000:])
    (tmp_path / "short.fq").write_bytes(cut)
    (tmp_path / "short_twin.fq").write_bytes(MQ.mask(cut, Q))
    r = run([TOOL, "--reads", tmp_path / "short.fq", "-o", tmp_path / "c.bf", "--gpu_parse", "--min_qual", Q] + small)
    run([TOOL, "--reads", tmp_path / "short_twin.fq", "-o", tmp_path / "d.bf"] + small)
    assert (tmp_path / "c.bf").read_bytes() == (tmp_path / "d.bf").read_bytes()
    assert "a quality line not as long as its sequence" in r.stderr


# ---------------------------------------------------------------------------------- 5. the polisher front ends
def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_ntedit_reads_equals_ntedit_with_the_twins_filter(read_set):
    d = read_set["dir"]
    twin_bf = d / "polish_twin.bf"
    run([TOOL, "--reads", read_set["twin"], "-o", twin_bf] + BUILD)
    run([NTEDIT, "-f", read_set["draft"], "-r", twin_bf, "-b", d / "by_filter"])
    for tag, flags in (("host", []), ("gpu", ["--gpu_parse"])):
        r = run([NTEDIT, "-f", read_set["draft"], "--reads", read_set["fq"], "-k", K, "--cutoff", 2, "--bf", 2_000_000, "--min_qual", Q,
                 "--save_bf", d / ("n_%s.bf" % tag), "-b", d / ("n_" + tag)] + flags)
        assert read(d / ("n_%s.bf" % tag)) == read(twin_bf)
        for suffix in ("_edited.fa", "_changes.tsv"):
            assert read(str(d / ("n_" + tag)) + suffix) == read(str(d / "by_filter") + suffix), (tag, suffix)
        assert masked_of(r) == [(Q, read_set["counts"][1], read_set["counts"][0])]  # (pass 2 reads the store)


def test_the_cascade_masks_alike_in_every_round(read_set):
    """-k 40,25: both rounds equal the rounds run from the masked file; the store is resident, the inputs parsed once"""
    d = read_set["dir"]
    common = ["-f", read_set["draft"], "-k", "40,25", "--cutoff", 2, "--bf", 2_000_000]
    run([NTEDIT] + common + ["--reads", read_set["twin"], "-b", d / "casc_twin"])
    r = run([NTEDIT] + common + ["--reads", read_set["fq"], "--min_qual", Q, "--gpu_parse", "-b", d / "casc"])
    for suffix in ("_k40_edited.fa", "_k40_changes.tsv", "_edited.fa", "_changes.tsv"):
        assert read(str(d / "casc") + suffix) == read(str(d / "casc_twin") + suffix), suffix
    assert len(masked_of(r)) == 1 and "no read file was opened" in r.stdout


@pytest.fixture(scope="module")
def twin_filter(read_set):
    """the single-process tool on the twin, without the flag"""
    out = read_set["dir"] / "ranks_twin.bf"
    run([TOOL, "--reads", read_set["twin"], "-o", out] + BUILD)
    return out


@pytest.mark.parametrize("flags", [[], ["--gpu_parse"]], ids=["host_parser", "gpu_parse"])
def test_make_reads_at_world_2_masks_alike_on_every_rank(read_set, twin_filter, flags):
    """over gloo, the plain FASTQ cut into ranges: the bytes of the single-process tool on the twin"""
    from test_gpu_reads_multi import _driver
    out = read_set["dir"] / ("w2_%d.bf" % len(flags))
    r = _driver(2, ["--reads", str(read_set["fq"]), "-o", str(out), "--min_qual", str(Q)] + [str(x) for x in BUILD] + flags, "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert out.read_bytes() == twin_filter.read_bytes()
    assert int(re.search(r"(\d+) units", r.stderr).group(1)) > 2
    by_rank = [(int(m), int(b)) for _, m, b in MASK_LINE.findall(r.stderr)]
    assert len(by_rank) == 4 and "rank 1/2: --min_qual" in r.stderr  # (two passes on each of two ranks)
    assert sum(m for m, _ in by_rank) == 2 * read_set["counts"][1] and sum(b for _, b in by_rank) == 2 * read_set["counts"][0]


def test_run_reads_at_world_1_equals_ntedit_with_the_twins_filter(read_set, twin_filter):
    from test_gpu_reads_run import driver, reports
    d = read_set["dir"]
    run([NTEDIT, "-f", read_set["draft"], "-r", twin_filter, "-b", d / "ranks_by_filter"])
    r = driver(1, ["-f", read_set["draft"], "--reads", read_set["fq"], "-k", K, "--cutoff", 2, "--bf", 2_000_000, "--min_qual", Q,
                   "--save_bf", d / "run.bf", "-b", d / "run", "--report"], "nccl")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert read(d / "run.bf") == read(twin_filter)
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(d / "run") + suffix) == read(str(d / "ranks_by_filter") + suffix), suffix
    assert reports(r)[0]["reads"]["parse"]["1"]["min_qual"] == dict(q=Q, qual_bases=read_set["counts"][0],
                                                                    masked_bases=read_set["counts"][1])
