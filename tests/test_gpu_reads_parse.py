"""--gpu_parse on the GPU: the device parser (ntedit_hip_reads_parse_device) against the host parser and against the
serial model of the clean grammar, on the CPU tier's corpus and on sizes around the tile geometry; the four front ends
with and without the flag, byte for byte; and one full-size run per format that prints what each pass cost in both modes.

The yardstick everywhere is the same build without the flag: that code path is the host parser's, unchanged."""
import ctypes
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import parse_corpus as PC
from ntedit_amd import _lib
from reads_model import awkward_reads, simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq, write_large_reads

pytestmark = pytest.mark.gpu

K = 25
T = _lib.PARSE_TILE
PASS_LINE = re.compile(r"Pass (\S+) \([^)]*\): (\d+) bases, ([\d.]+) ms, [\d.]+ Gbases/s \(GPU calls ([\d.]+) ms")
PARSE_LINE = re.compile(r"--gpu_parse: (\d+) chunks parsed on the device \((\d+) raw bytes, (\d+) text bytes, ([\d.]+) ms")


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_sketch_free(p._h)  # (the parser's scratch)
    p.close()


def device_parse(pol, raw, k, on_device=False, guard=0):
    """-> (ReadsParseResult, the text when clean, the bytes behind the text buffer's cap)"""
    import torch
    n = len(raw)
    cap = (n + 15) // 16 * 16
    text = torch.full((cap + guard + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsParseResult()
    src = raw
    if on_device:
        dev = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
        src = dev.data_ptr()
    torch.cuda.synchronize()
    rc = pol._lib.ntedit_hip_reads_parse_device(pol._h, src, n, int(on_device), k, text.data_ptr(), cap, res)
    assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    host = bytes(text.cpu().numpy())
    return res, host[:res.text_len] if res.clean else None, host[cap:]


def check(pol, tmp_path, raw, k, on_device=False, expect_clean=None):
    """the device against the model (clean exactly where the model says so) and, wherever clean, the host parser"""
    lib = pol._lib
    mres, mtext = PC.model(lib, raw, k)
    res, text, behind = device_parse(pol, raw, k, on_device, guard=64)
    assert behind == b"\xEE" * len(behind)
    assert res.clean == mres.clean, (res.clean, res.broken, mres.broken)
    if expect_clean is not None:
        assert bool(res.clean) == expect_clean, res.broken
    if res.clean:
        path = tmp_path / "chunk.txt"
        path.write_bytes(raw)
        htext, reads, bases = PC.host_text(lib, str(path), k)
        assert text == htext and text == mtext
        assert (res.reads, res.bases, res.text_len, res.lines) == (reads, bases, len(htext), mres.lines)
    else:
        assert res.broken != 0
    return res


# ---------------------------------------------------------------------------------- 1. the device parser
@pytest.mark.parametrize("k", PC.KS)
def test_fixed_corpus(pol, tmp_path, k):
    for name, raw in sorted(PC.well_formed().items()):
        check(pol, tmp_path, raw, k, expect_clean=True)
    for name, raw in sorted(PC.odd().items()):
        check(pol, tmp_path, raw, k, expect_clean=False)
    # device-resident raw bytes take the same way
    for name in ("fasta_wrapped_60", "fastq_4_line"):
        check(pol, tmp_path, PC.well_formed()[name], k, on_device=True, expect_clean=True)


def test_generated_corpus(pol, tmp_path):
    clean = 0
    for i, (raw, k, mutated) in enumerate(PC.generated(3000)):
        res = check(pol, tmp_path, raw, k, expect_clean=None if mutated else True)
        clean += res.clean
    assert clean >= 1500


def fasta_of_size(size, line=100, seed=0):
    """a FASTA chunk of exactly `size` bytes: records of three lines of `line` bases, the last line cut to fit"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    i = 0
    while len(out) < size:
        out += b">rec%d\n" % i
        for _ in range(3):
            out += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), line)) + b"\n"
        i += 1
    out = out[:size]
    # the cut may leave a header or an empty line at the end: end on a sequence byte and a newline instead
    out[-40:] = b"\n>tail\n" + b"ACGT" * 8 + b"\n"
    assert len(out) == size
    return bytes(out)


def fasta_with_newline_at(pos, total):
    """a FASTA chunk of `total` bytes whose first line break after the header's falls exactly on byte `pos`"""
    head = b">edge\n"
    seq1 = b"A" * (pos - len(head))
    rest = total - (len(head) + len(seq1) + 1)
    return head + seq1 + b"\n" + b"C" * (rest - 1) + b"\n"


@pytest.mark.parametrize("size", [T - 1, T, T + 1, 3 * T + 5])
def test_chunk_sizes_around_the_tile(pol, tmp_path, size):
    check(pol, tmp_path, fasta_of_size(size), K, expect_clean=True)
    check(pol, tmp_path, fasta_of_size(size, seed=1), K, on_device=True, expect_clean=True)


@pytest.mark.parametrize("pos", [T - 1, T, 2 * T - 1, 2 * T])
def test_newline_as_the_first_and_the_last_byte_of_a_tile(pol, tmp_path, pos):
    check(pol, tmp_path, fasta_with_newline_at(pos, 3 * T), 12, expect_clean=True)


def test_a_line_of_exactly_one_tile(pol, tmp_path):
    rng = np.random.default_rng(3)
    line = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), T))
    check(pol, tmp_path, b">a\n" + line + b"\n>b\n" + line[:77] + b"\n", K, expect_clean=True)
    # a line whose bytes are the tile's: T - 1 bases and the newline
    check(pol, tmp_path, b">a" + b"x" * (T - 3) + b"\n" + line[:T - 1] + b"\n" + line[:99] + b"\n", K, expect_clean=True)


def test_long_reads(pol, tmp_path):
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    mbp = bytes(rng.choice(acgt, 1_000_000))
    res = check(pol, tmp_path, b">short\nACGTACGTACGTAC\n>long one\n" + mbp + b"\n>after\n" + mbp[:5000] + b"\n", K,
                expect_clean=True)
    assert res.reads == 2
    kbp = bytes(rng.choice(acgt, 300_000))
    q = bytes(rng.integers(33, 127, 300_000).astype(np.uint8))
    res = check(pol, tmp_path, b"@a\n" + kbp[:200] + b"\n+\n" + q[:200] + b"\n@long\n" + kbp + b"\n+\n" + q + b"\n", K,
                expect_clean=True)
    assert res.reads == 2 and res.bases == 300_200


@pytest.mark.parametrize("fastq", [False, True])
def test_many_reads_of_every_length(pol, tmp_path, fastq):
    rng = np.random.default_rng(5)
    genome = H.random_genome(rng, 50000)
    lengths = rng.integers(1, 401, 100_000)
    starts = rng.integers(0, 50000 - 400, 100_000)
    parts = []
    for i, (s, n) in enumerate(zip(starts, lengths)):
        r = genome[s:s + n]
        parts.append(b"@read%d\n%s\n+\n%s\n" % (i, r, b"I" * n) if fastq else b">read%d\n%s\n" % (i, r))
    raw = b"".join(parts)
    res = check(pol, tmp_path, raw, K, expect_clean=True)
    assert res.reads == int((lengths >= K).sum())


def test_more_lines_than_the_table_holds_is_unclean_and_writes_nothing(pol, tmp_path):
    raw = b">a\n" + b"A\n" * 200_000
    res, _, behind = device_parse(pol, raw, 12, guard=4096)
    assert res.clean == 0 and res.broken & _lib.PARSE_BAD["table"]
    assert behind == b"\xEE" * len(behind)
    check(pol, tmp_path, raw, 12, expect_clean=False)
    # and the next chunk on the same context parses as if nothing had happened
    check(pol, tmp_path, PC.well_formed()["fastq_4_line"], 12, expect_clean=True)


# ---------------------------------------------------------------------------------- 2. the tool with and without the flag
def tool(args, timeout=900):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def passes_of(r):
    return [(name, int(bases)) for name, bases, _, _ in PASS_LINE.findall(r.stderr)]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_parse")
    rng = np.random.default_rng(61)
    genome = H.random_genome(rng, 60000)
    sim = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    awk = [r[:30].lower() + r[30:] if i % 4 == 0 else r for i, r in enumerate(awkward_reads(K, seed=9, genome_len=20000))]
    assert any(len(r) < K for r in awk) and any(b"N" in r for r in awk)
    half = len(sim) // 2
    write_fasta(d / "a.fa", sim[:half] + awk)
    write_fastq(d / "b.fq", sim[half:] + awk)
    write_fastq(d / "c.fq.gz", sim[:half], opener=gzip.open)
    with open(d / "crlf.fq", "wb") as f:
        for i, r in enumerate(sim[:2000]):
            f.write(b"@r%d\r\n%s\r\n+\r\n%s\r\n" % (i, r, b"I" * len(r)))
    return d


def both_ways(reads, tag, files, args):
    """the tool without and with --gpu_parse -> (the two runs); filters, --hist files and bases per pass must be equal"""
    d = reads
    runs = []
    for flag in ((), ("--gpu_parse",)):
        out = d / ("%s%d.bf" % (tag, len(flag)))
        a = [x.replace("{hist}", str(out) + ".hist") if isinstance(x, str) else x for x in args]
        runs.append((tool(["--reads"] + [d / f for f in files] + ["-k", K, "-o", out] + a + list(flag)), out))
    (r0, o0), (r1, o1) = runs
    assert o0.read_bytes() == o1.read_bytes(), tag
    if any("{hist}" in str(x) for x in args):
        assert open(str(o0) + ".hist", "rb").read() == open(str(o1) + ".hist", "rb").read(), tag
    assert passes_of(r0) == passes_of(r1) and passes_of(r0), (r0.stderr, r1.stderr)
    assert "--gpu_parse" not in r0.stderr
    return r0, r1


CUT = ["-c", 2, "--bf", 1 << 16, "--sketch_bytes", 1000003]


@pytest.mark.parametrize("tag,files,args", [
    ("fa", ["a.fa"], CUT),
    ("fq", ["b.fq"], CUT),
    ("two", ["a.fa", "b.fq"], CUT),
    ("small_batches", ["a.fa", "b.fq"], CUT + ["--batch_bytes", 4096]),
    ("solid_hist", ["a.fa", "b.fq"], ["--solid", "--hist", "{hist}"]),
    ("counts", ["b.fq"], CUT + ["--counts"]),
])
def test_the_tool_is_identical_with_the_flag(reads, tag, files, args):
    _, r1 = both_ways(reads, tag, files, args)
    lines = PARSE_LINE.findall(r1.stderr)
    assert len(lines) == len(passes_of(r1)), r1.stderr
    raw = sum(os.path.getsize(reads / f) for f in files)
    for chunks, raw_bytes, text_bytes, _ in lines:
        assert int(chunks) >= len(files) and int(raw_bytes) == raw and 0 < int(text_bytes) < raw
    if tag == "small_batches":
        assert all(int(chunks) > raw // 8192 for chunks, _, _, _ in lines)
    # well-formed plain inputs: nothing goes back to the host parser
    assert "unclean" not in r1.stderr and "gzip" not in r1.stderr


def test_a_gzip_file_beside_a_plain_one_stays_on_the_host(reads):
    _, r1 = both_ways(reads, "gz", ["c.fq.gz", "b.fq"], CUT)
    assert r1.stderr.count("1 gzip inputs stay with the host parser") == 2, r1.stderr
    for chunks, raw_bytes, _, _ in PARSE_LINE.findall(r1.stderr):
        assert int(raw_bytes) == os.path.getsize(reads / "b.fq")
    assert "unclean" not in r1.stderr


def test_a_crlf_fastq_falls_back_with_its_line(reads):
    _, r1 = both_ways(reads, "crlf", ["crlf.fq", "a.fa"], CUT)
    assert r1.stderr.count("1 unclean chunks sent the rest of their ranges to the host parser (a carriage return)") == 2, r1.stderr


def test_parse_info_reports_no_fallback_on_well_formed_input(reads, pol):
    lib, h = pol._lib, pol._h
    files = [str(reads / "a.fa").encode(), str(reads / "b.fq").encode()]
    lines = []
    log = _lib.READS_LOG_FN(lambda user, to_stdout, line: lines.append(line.decode()))
    results = {}
    for flag in (0, 1):
        args = _lib.ReadsBuildArgs(files=(ctypes.c_char_p * 2)(*files), n_files=2, k=K, hash_num=3, cmin=2, bf_bytes=1 << 16,
                                   fpr=0.01, sketch_counters=1000003, batch_bytes=1 << 20, log=log, device_parse=flag)
        res = _lib.ReadsBuildResult()
        assert lib.ntedit_hip_reads_build(h, args, res) == 0, lib.ntedit_hip_reads_last_error(h)
        st = _lib.ReadsParseStats()
        assert lib.ntedit_hip_reads_parse_info(h, st) == 0
        results[flag] = (pol.filter_download(0).tobytes(), [p.bases for p in res.passes], st)
    assert results[0][:2] == results[1][:2]
    st = results[1][2]
    assert st.fallback_chunks == 0 and st.host_files == 0 and st.broken == 0
    assert st.device_chunks >= 2 and st.raw_bytes == sum(os.path.getsize(f) for f in files) and st.text_bytes > 0


# ---------------------------------------------------------------------------------- 3. the polisher front ends
def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def polish_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_parse_polish")
    rng = np.random.default_rng(43)
    truth = H.random_genome(rng, 120000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:70000]), (b"ctg2", draft[70000:])], width=80)
    sim = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    half = len(sim) // 2
    write_fastq(d / "r1.fq", sim[:half] + list(awkward_reads(K, seed=5, genome_len=10000)))
    write_fasta(d / "r2.fa", sim[half:])
    return dict(dir=d, draft=d / "draft.fa", reads=[str(d / "r1.fq"), str(d / "r2.fa")])


def same_outputs(a, b):
    for suffix in ("_edited.fa", "_changes.tsv", ".bf"):
        assert read(str(a) + suffix) == read(str(b) + suffix), suffix
    assert H.vcf_body(str(a) + "_variants.vcf") == H.vcf_body(str(b) + "_variants.vcf")


@pytest.mark.parametrize("store", ["store", "no_store"])
def test_ntedit_reads_is_identical_with_the_flag(polish_case, store):
    c = polish_case
    extra = [] if store == "store" else ["--resident_cap", 0]
    outs = []
    for flag in ((), ("--gpu_parse",)):
        p = c["dir"] / ("n_%s_%d" % (store, len(flag)))
        r = subprocess.run([str(x) for x in [NTEDIT, "-f", c["draft"], "--reads"] + c["reads"] +
                            ["-k", K, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", 1 << 22, "--save_bf", str(p) + ".bf",
                             "-b", p] + extra + list(flag)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append((p, r))
    same_outputs(outs[0][0], outs[1][0])
    assert passes_of(outs[0][1]) == passes_of(outs[1][1])
    r1 = outs[1][1]
    # pass 1 always reads the files; the later passes read the store unless it is off
    assert len(PARSE_LINE.findall(r1.stderr)) == (1 if store == "store" else 2), r1.stderr
    assert "unclean" not in r1.stderr and "--gpu_parse" not in outs[0][1].stderr


def test_run_reads_world_1_rccl_is_identical_with_the_flag(polish_case):
    from test_gpu_reads_run import driver, reports
    c = polish_case
    outs = []
    for flag in ((), ("--gpu_parse",)):
        p = c["dir"] / ("run_%d" % len(flag))
        r = driver(1, ["-f", c["draft"], "--reads"] + c["reads"] + ["-k", K, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes",
                                                                     1 << 22, "--save_bf", str(p) + ".bf", "-b", p,
                                                                     "--report"] + list(flag), "nccl")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
        outs.append((p, reports(r)[0]))
    same_outputs(outs[0][0], outs[1][0])
    assert "parse" not in outs[0][1]["reads"]
    parse = outs[1][1]["reads"]["parse"]
    assert parse["1"]["fallback_chunks"] == 0 and parse["1"]["device_chunks"] >= 2
    assert parse["1"]["raw_bytes"] == sum(os.path.getsize(f) for f in c["reads"])
    assert outs[0][1]["reads"]["passes"]["1"]["bases"] == outs[1][1]["reads"]["passes"]["1"]["bases"]


def test_make_reads_world_2_gloo_cuts_a_plain_file_and_equals_the_tool(reads):
    from test_gpu_reads_multi import _driver
    ref = reads / "mr_ref.bf"
    tool(["--reads", reads / "b.fq", "-k", K, "-o", ref] + CUT)
    out = reads / "mr_w2.bf"
    r = _driver(2, ["--reads", str(reads / "b.fq"), "-k", str(K), "-o", str(out), "--gpu_parse"] + [str(x) for x in CUT], "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]  # (a failed cut-point check refuses the run)
    assert out.read_bytes() == ref.read_bytes()
    assert re.search(r"rank 1/2: --gpu_parse: \d+ chunks", r.stderr) and "unclean" not in r.stderr, r.stderr[-3000:]
    assert "units" in r.stderr and int(re.search(r"(\d+) units", r.stderr).group(1)) > 2


# ---------------------------------------------------------------------------------- 4. full size, one run
def fastq_of_fasta(fa, fq, chunk_rows=1_000_000, length=150):
    """the read set of write_large_reads (rows of '>r\\n' + 150 bases + '\\n') as 4-line FASTQ"""
    row = length + 4
    with open(fa, "rb") as f, open(fq, "wb") as g:
        while True:
            buf = f.read(row * chunk_rows)
            if not buf:
                break
            rows = np.frombuffer(buf, dtype=np.uint8).reshape(-1, row)
            out = np.empty((rows.shape[0], 3 + length + 1 + 2 + length + 1), dtype=np.uint8)
            out[:, 0], out[:, 1], out[:, 2] = ord("@"), ord("r"), ord("\n")
            out[:, 3:3 + length + 1] = rows[:, 3:]
            out[:, 4 + length], out[:, 5 + length] = ord("+"), ord("\n")
            out[:, 6 + length:6 + 2 * length] = ord("I")
            out[:, -1] = ord("\n")
            g.write(out.tobytes())


def test_full_size_fasta_and_fastq_with_and_without_the_flag(tmp_path):
    fa, fq = tmp_path / "large.fa", tmp_path / "large.fq"
    _, n_reads = write_large_reads(fa)
    table = []
    for form, path in (("fasta", fa), ("fastq", fq)):
        if form == "fastq":
            fastq_of_fasta(fa, fq)
            os.remove(fa)
        outs = []
        for i, flag in enumerate(((), ("--gpu_parse",), (), ("--gpu_parse",))):
            out = tmp_path / ("%s_%d.bf" % (form, i))
            r = tool(["--reads", path, "-k", K, "-c", 3, "--bf", 200_000_000, "--sketch_bytes", 1 << 32, "-o", out] +
                     list(flag), timeout=1800)
            found = PASS_LINE.findall(r.stderr)
            assert [int(b) for _, b, _, _ in found] == [n_reads * 150] * 2, r.stderr
            parse = PARSE_LINE.findall(r.stderr)
            if flag:
                assert len(parse) == 2 and "unclean" not in r.stderr, r.stderr
                assert all(int(raw) == os.path.getsize(path) for _, raw, _, _ in parse)
            table.append(dict(format=form, gpu_parse=bool(flag), run=i // 2,
                              passes=[dict(pass_=p, wall_ms=float(w), gpu_ms=float(g)) for p, _, w, g in found],
                              parse=[dict(chunks=int(c), raw_bytes=int(rb), text_bytes=int(tb), kernel_ms=float(ms))
                                     for c, rb, tb, ms in parse]))
            print(json.dumps(table[-1]))
            outs.append(out.read_bytes())
            os.remove(out)
        assert outs[0] == outs[1] == outs[2] == outs[3], form
