"""--gpu_parse on BGZF reads, on the GPU: the inflate kernel (ntedit_hip_reads_inflate_device) against the serial host
model and Python's zlib, the device's chunk cut against the exported host rule, and the four --reads front ends on BGZF
files with and without the flag (tests/bgzf_corpus.py builds the BGZF; the CPU tier is tests/test_reads_inflate_cpu.py)."""
import ctypes
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bgzf_corpus as BC
import helpers as H
from ntedit_amd import _lib
from reads_model import simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq

pytestmark = pytest.mark.gpu

K = 25
PASS_LINE = re.compile(r"Pass (\S+) \([^)]*\): (\d+) bases")
BGZF_LINE = re.compile(r"--gpu_parse: BGZF: (\d+) members of (\d+) files? inflated on the device \((\d+) compressed bytes, "
                       r"(\d+) inflated bytes, ([\d.]+) ms in the inflate kernels\), (\d+) files? handed back([^;]*); "
                       r"(\d+) gzip inputs stay with the host parser")


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_sketch_free(p._h)  # (the inflate and parse scratch)
    p.close()


@pytest.fixture(scope="module")
def corpus():
    return BC.corpus()


def device_inflate(pol, blob, members, n_out, on_device=False):
    """-> (statuses, the output bytes); the 0xEE guard behind out_cap is checked"""
    import torch
    out = torch.full((n_out + BC.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    status = (ctypes.c_uint32 * max(len(members), 1))()
    src = blob
    if on_device:
        dev = torch.frombuffer(bytearray(blob) + bytearray(16), dtype=torch.uint8).cuda()
        src = dev.data_ptr()
    torch.cuda.synchronize()
    rc = pol._lib.ntedit_hip_reads_inflate_device(pol._h, src, len(blob), int(on_device), BC.table(members), len(members),
                                                  out.data_ptr(), n_out, status)
    assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    host = bytes(out.cpu().numpy())
    assert host[n_out:] == b"\xEE" * BC.GUARD
    return list(status)[:len(members)], host[:n_out]


# ---------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("on_device", [False, True], ids=["host_input", "device_input"])
def test_the_device_equals_the_model_and_zlib_on_the_corpus(pol, corpus, on_device):
    blob, members, n_out = BC.table_of([m for _, m, _ in corpus])
    status, out = device_inflate(pol, blob, members, n_out, on_device)
    assert status == [0] * len(corpus), [(corpus[i][0], s) for i, s in enumerate(status) if s]
    assert out == b"".join(d for _, _, d in corpus)
    assert (status, out) == BC.model(pol._lib, blob, members, n_out)


@pytest.mark.parametrize("count", BC.COUNTS)
def test_member_counts_around_the_workgroup(pol, corpus, count):
    """1, 2, 4, 5, 65, 257 members a call: partial workgroups of four waves, and more members than one workgroup's"""
    small = [c for c in corpus if len(c[2]) <= 9001]
    picked = [small[(7 * i) % len(small)] for i in range(count)]
    blob, members, n_out = BC.table_of([m for _, m, _ in picked])
    status, out = device_inflate(pol, blob, members, n_out, on_device=count % 2 == 0)
    assert status == [0] * count and out == b"".join(d for _, _, d in picked)


def test_damaged_members_get_the_models_verdict_on_the_device(pol):
    """the first 200 flips and 50 truncations of the CPU tier's list, which the host build has shown to stay in bounds;
    one call, every member with its own output bytes"""
    flips, cuts = BC.damaged()
    cases = [m for _, m in flips[:200] + cuts[:50] if struct.unpack("<I", m[-4:])[0] <= 65536]
    assert len(cases) > 240
    blob, members, n_out = BC.table_of(cases)
    mstatus, mout = BC.model(pol._lib, blob, members, n_out)
    status, out = device_inflate(pol, blob, members, n_out)
    assert status == mstatus
    for m, st, mb in zip(cases, status, members):
        want = BC.verdict(m)
        assert (st == 0) == (want is not None)
        if want is not None:
            assert out[mb.out_off:mb.out_off + mb.n_out] == want == mout[mb.out_off:mb.out_off + mb.n_out]


def cut_buffers():
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40 + i)) for i in range(40)]
    fa = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    fa_wrapped = b"".join(b">w%d\n%s\n%s\n" % (i, s[:20], s[20:]) for i, s in enumerate(seqs))
    last_fa, last_fq = fa.rfind(b">"), fq.rfind(b"@r")
    return {
        # the candidate in the last line, in the third-last line, and nowhere past the first byte
        "fasta_header_is_the_last_line": (fa + b">last", ord(">")),
        "fasta_header_is_the_third_last_line": (fa_wrapped, ord(">")),
        "fasta_one_record": (fa[:fa.find(b">", 1)], ord(">")),
        "fasta_whole": (fa, ord(">")),
        "fastq_cut_behind_the_plus": (fq[:fq.find(b"+", last_fq) + 1], ord("@")),  # '@' third-last, '+' last line
        "fastq_cut_before_the_plus": (fq[:fq.find(b"+", last_fq)], ord("@")),       # that '@' line is no start yet
        "fastq_whole": (fq, ord("@")),
        "fastq_one_record": (fq[:fq.find(b"@r1\n")], ord("@")),
        # (the line table holds one line per 8 bytes: the names keep these within it)
        "fastq_quality_starts_with_at": (b"@name_a_long\nACGTACGT\n+\n@IIIIIII\n@name_b_long\nACGTACGT\n+\n@IIIIIII", ord("@")),
        "fastq_header_line_only": (b"@name_a_long\n", ord("@")),
    }, last_fa


@pytest.mark.parametrize("on_device", [False, True], ids=["host_input", "device_input"])
def test_the_device_cut_equals_the_host_rule(pol, on_device):
    import torch
    bufs, _ = cut_buffers()
    seen = set()
    for name, (raw, kind) in bufs.items():
        want = pol._lib.ntedit_hip_reads_last_record_start(raw, len(raw), kind)
        py = BC.python_last_record_start(raw, kind)
        assert want == (_lib.READS_NO_START if py is None else py), name
        src = raw
        if on_device:
            dev = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            src = dev.data_ptr()
        got = ctypes.c_uint64()
        rc = pol._lib.ntedit_hip_reads_last_start_device(pol._h, src, len(raw), int(on_device), got)
        assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
        assert got.value == want, (name, got.value, want)
        seen.add(want == _lib.READS_NO_START)
    assert seen == {True, False}


# ---------------------------------------------------------------------------------- 2. the tool
def run(args, timeout=600):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def tool(args):
    r = run([TOOL] + list(args))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def passes_of(r):
    return [(name, int(bases)) for name, bases in PASS_LINE.findall(r.stderr)]


SMALL = ["-k", K, "-c", 2, "--bf", 2000000, "--batch_bytes", 4096]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """2,000 simulated reads as plain FASTQ / FASTA and as BGZF at block sizes 300 and 65280"""
    d = tmp_path_factory.mktemp("gpu_inflate")
    rng = np.random.default_rng(1951)
    genome = H.random_genome(rng, 10000)
    sim = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    assert len(sim) == 2000
    write_fastq(d / "r.fq", sim)
    fq = (d / "r.fq").read_bytes()
    fa = b"".join(b">r%d\n%s" % (i, b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60))) for i, r in enumerate(sim))
    (d / "r.fa").write_bytes(fa)
    (d / "r300.fq.gz").write_bytes(BC.bgzf(fq, block=300))
    (d / "r65280.fq.gz").write_bytes(BC.bgzf(fq, block=65280))
    (d / "r300.fa.gz").write_bytes(BC.bgzf(fa, block=300, eof=False))
    (d / "single.fq.gz").write_bytes(gzip.compress(fq))
    half = fq.find(b"@r1500\n")
    (d / "crlf_later.fq.gz").write_bytes(BC.bgzf(fq[:half] + fq[half:].replace(b"\n", b"\r\n"), block=300))
    (d / "gzip_later.fq.gz").write_bytes(BC.bgzf(fq[:half], block=300, eof=False) + gzip.compress(fq[half:]))
    return dict(dir=d, fq=fq, fa=fa, sim=sim, half=half)


def both_ways(reads, tag, files, args):
    """the tool without and with --gpu_parse -> the two runs; every output and the bases per pass must be equal"""
    d = reads["dir"]
    runs = []
    for flag in ((), ("--gpu_parse",)):
        out = d / ("%s%d.bf" % (tag, len(flag)))
        a = [x.replace("{out}", str(out)) if isinstance(x, str) else x for x in args]
        runs.append((tool(["--reads"] + [d / f for f in files] + ["-o", out] + a + list(flag)), out))
    (r0, o0), (r1, o1) = runs
    assert o0.read_bytes() == o1.read_bytes(), tag
    for suffix in (".hist", ".reject"):
        if any(("{out}" + suffix) in str(x) for x in args):
            assert open(str(o0) + suffix, "rb").read() == open(str(o1) + suffix, "rb").read(), (tag, suffix)
    assert passes_of(r0) == passes_of(r1) and passes_of(r0), (r0.stderr, r1.stderr)
    assert "--gpu_parse" not in r0.stderr
    return r0, r1, o1.read_bytes()


def plain_filter(reads, plain):
    """the filter of the plain file, without the flag (made once)"""
    ref = reads["dir"] / (plain + ".ref.bf")
    if not ref.exists():
        tool(["--reads", reads["dir"] / plain, "-o", ref] + SMALL)
    return ref.read_bytes()


@pytest.mark.parametrize("name,plain", [("r300.fq.gz", "r.fq"), ("r65280.fq.gz", "r.fq"), ("r300.fa.gz", "r.fa")])
def test_bgzf_reads_are_inflated_on_the_device_with_the_same_filter(reads, name, plain):
    d = reads["dir"]
    _, r1, bf = both_ways(reads, name.replace(".", "_"), [name], SMALL)
    assert bf == plain_filter(reads, plain)
    lines = BGZF_LINE.findall(r1.stderr)
    assert len(lines) == len(passes_of(r1)) == 2, r1.stderr
    data = reads["fa"] if plain.endswith(".fa") else reads["fq"]
    block = 65280 if "65280" in name else 300
    for members, files, comp, raw, _, handed_back, _, gzip_inputs in lines:
        assert int(members) == (len(data) + block - 1) // block + (0 if name.endswith(".fa.gz") else 1) and int(files) == 1
        assert int(raw) == len(data) and int(comp) == os.path.getsize(d / name)
        assert int(handed_back) == 0 and int(gzip_inputs) == 0
    assert "0 files handed back; 0 gzip inputs stay with the host parser" in r1.stderr and "unclean" not in r1.stderr


def test_solid_hist_and_reject_outputs_are_identical(reads):
    _, r1, _ = both_ways(reads, "solid", ["r300.fq.gz", "r65280.fq.gz"],
                         ["-k", K, "--solid", "--hist", "{out}.hist", "--reject_cutoff", 30, "--reject_out", "{out}.reject",
                          "--batch_bytes", 4096])
    lines = BGZF_LINE.findall(r1.stderr)
    assert len(lines) == 3 and all(int(l[1]) == 2 and int(l[5]) == 0 for l in lines), r1.stderr


def test_single_stream_gzip_stays_with_the_host_parser(reads):
    _, r1, bf = both_ways(reads, "single", ["single.fq.gz"], SMALL)
    assert bf == plain_filter(reads, "r.fq")
    assert r1.stderr.count("1 gzip inputs stay with the host parser") == 2 and "BGZF" not in r1.stderr, r1.stderr
    assert r1.stderr.count("--gpu_parse: 0 chunks parsed on the device") == 2


@pytest.mark.parametrize("name", ["crlf_later.fq.gz", "gzip_later.fq.gz"])
def test_the_rest_of_a_file_is_handed_back_at_a_record_start(reads, name):
    _, r1, bf = both_ways(reads, name.split(".")[0], [name], SMALL)
    lines = BGZF_LINE.findall(r1.stderr)
    assert len(lines) == 2, r1.stderr
    for members, _, _, raw, _, handed_back, where, _ in lines:
        assert int(handed_back) == 1 and "1 file handed back" in r1.stderr
        at = int(re.search(r"inflated offset (\d+)", where).group(1))
        # an exact record start, behind clean chunks and not past the first byte the device could not take
        assert 0 < at <= reads["half"] and reads["fq"][at:at + 2] == b"@r" and reads["fq"][at - 1:at] == b"\n"
        assert int(members) > 0 and int(raw) >= at
    if name.startswith("gzip"):
        assert bf == plain_filter(reads, "r.fq")


def test_a_damaged_member_fails_the_pass_with_and_without_the_flag(reads):
    d = reads["dir"]
    good = (d / "r65280.fq.gz").read_bytes()
    rc, members, _ = BC.walk(_lib.load(), good)
    assert len(members) >= 4
    target = 2
    blob = bytearray(good)
    start = members[target].in_off - BC.HEADER
    size = BC.HEADER + members[target].n_in + 8
    bit = (members[target].in_off + members[target].n_in // 2) * 8
    while True:  # one flipped data bit that zlib refuses
        blob[bit >> 3] ^= 1 << (bit & 7)
        if BC.verdict(bytes(blob[start:start + size])) is None:
            break
        blob[bit >> 3] ^= 1 << (bit & 7)
        bit += 1
    (d / "damaged.fq.gz").write_bytes(bytes(blob))
    for flag in ((), ("--gpu_parse",)):
        out = d / ("damaged%d.bf" % len(flag))
        r = run([TOOL, "--reads", d / "damaged.fq.gz", "-o", out] + SMALL + list(flag))
        assert r.returncode != 0 and not out.exists(), r.stderr[-2000:]
        if flag:
            assert "BGZF member %d is damaged" % target in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------- 3. the other front ends
def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def polish_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_inflate_polish")
    rng = np.random.default_rng(44)
    truth = H.random_genome(rng, 40000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:25000]), (b"ctg2", draft[25000:])], width=80)
    sim = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    half = len(sim) // 2
    write_fastq(d / "r1.fq", sim[:half])
    write_fasta(d / "r2.fa", sim[half:])
    (d / "r1.fq.gz").write_bytes(BC.bgzf(read(d / "r1.fq"), block=65280))
    (d / "r2.fa.gz").write_bytes(BC.bgzf(read(d / "r2.fa"), block=5000))
    return dict(dir=d, draft=d / "draft.fa", reads=[str(d / "r1.fq.gz"), str(d / "r2.fa.gz")])


def same_outputs(a, b):
    for suffix in ("_edited.fa", "_changes.tsv", ".bf"):
        assert read(str(a) + suffix) == read(str(b) + suffix), suffix
    assert H.vcf_body(str(a) + "_variants.vcf") == H.vcf_body(str(b) + "_variants.vcf")


POLISH = ["-k", K, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", 1 << 22]


def test_ntedit_reads_on_bgzf_is_identical_with_the_flag(polish_case):
    c = polish_case
    outs = []
    for flag in ((), ("--gpu_parse",)):
        p = c["dir"] / ("n_%d" % len(flag))
        r = run([NTEDIT, "-f", c["draft"], "--reads"] + c["reads"] + POLISH + ["--save_bf", str(p) + ".bf", "-b", p] + list(flag))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append((p, r))
    same_outputs(outs[0][0], outs[1][0])
    assert passes_of(outs[0][1]) == passes_of(outs[1][1])
    lines = BGZF_LINE.findall(outs[1][1].stderr)
    assert lines and all(int(l[1]) == 2 and int(l[5]) == 0 and int(l[7]) == 0 for l in lines), outs[1][1].stderr
    assert "BGZF" not in outs[0][1].stderr


def test_run_reads_world_1_on_bgzf_is_identical_with_the_flag(polish_case):
    from test_gpu_reads_run import driver, reports
    c = polish_case
    outs = []
    for flag in ((), ("--gpu_parse",)):
        p = c["dir"] / ("run_%d" % len(flag))
        r = driver(1, ["-f", c["draft"], "--reads"] + c["reads"] + POLISH + ["--save_bf", str(p) + ".bf", "-b", p, "--report"] +
                   list(flag), "nccl")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
        outs.append((p, reports(r)[0]))
    same_outputs(outs[0][0], outs[1][0])
    parse = outs[1][1]["reads"]["parse"]
    assert parse["1"]["fallback_chunks"] == 0 and parse["1"]["host_files"] == 0 and parse["1"]["device_chunks"] >= 2
    assert parse["1"]["raw_bytes"] == sum(os.path.getsize(f[:-3]) for f in c["reads"])  # (the inflated bytes)
    bgzf = parse["1"]["bgzf"]
    assert bgzf["files"] == 2 and bgzf["handed_back"] == 0 and bgzf["inflated_bytes"] == parse["1"]["raw_bytes"]
    assert bgzf["compressed_bytes"] == sum(os.path.getsize(f) for f in c["reads"]) and bgzf["members"] > 2
    assert outs[0][1]["reads"]["passes"]["1"]["bases"] == outs[1][1]["reads"]["passes"]["1"]["bases"]


def test_make_reads_world_2_gloo_on_two_bgzf_files_equals_the_tool(polish_case):
    from test_gpu_reads_multi import _driver
    c = polish_case
    cut = ["-k", str(K), "-c", "2", "--bf", str(1 << 16), "--sketch_bytes", "1000003"]
    ref = c["dir"] / "mr_ref.bf"
    tool(["--reads"] + c["reads"] + ["-o", ref] + cut)
    out = c["dir"] / "mr_w2.bf"
    r = _driver(2, ["--reads"] + c["reads"] + ["-o", str(out), "--gpu_parse"] + cut, "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert out.read_bytes() == ref.read_bytes()
    # a BGZF file is one unit: each rank inflates one of the two on its device, none goes back
    for rank in (0, 1):
        assert re.search(r"rank %d/2: --gpu_parse: BGZF: \d+ members of 1 file inflated on the device" % rank, r.stderr), r.stderr[-3000:]
    assert "1 file handed back" not in r.stderr and "gzip inputs stay with the host parser" in r.stderr


# ---------------------------------------------------------------------------------- 4. full size, one run
def _members_of_group(args):
    data, block, level = args
    return b"".join(BC.member(data[i:i + block], level=level) for i in range(0, len(data), block))


def bgzf_file(src, dst, block=65280, level=6, group=128, procs=16):
    """src as a BGZF file, as `bgzip -@ 16` writes it (zlib's default level, 65280-byte blocks, the EOF member)"""
    import multiprocessing

    def groups():
        with open(src, "rb") as f:
            while True:
                data = f.read(block * group)
                if not data:
                    return
                yield data, block, level
    with multiprocessing.Pool(procs) as pool, open(dst, "wb") as g:
        for part in pool.imap(_members_of_group, groups()):
            g.write(part)
        g.write(BC.EOF_MEMBER)


def test_full_size_bgzf_fastq_with_and_without_the_flag(tmp_path):
    """3 Gbases as BGZF FASTQ, the flag off and on, alternated twice: identical filters; every pass's wall and GPU time
    is printed (DESIGN.md 9.6 holds a run's figures), and nothing about time is asserted"""
    import json
    from test_gpu_reads_bf import write_large_reads
    from test_gpu_reads_parse import PASS_LINE as TIMED_PASS_LINE, fastq_of_fasta
    fa, fq, gz = tmp_path / "large.fa", tmp_path / "large.fq", tmp_path / "large.fq.gz"
    _, n_reads = write_large_reads(fa)
    fastq_of_fasta(fa, fq)
    os.remove(fa)
    bgzf_file(fq, gz)
    inflated = os.path.getsize(fq)
    os.remove(fq)
    print(json.dumps(dict(reads=n_reads, inflated_bytes=inflated, bgzf_bytes=os.path.getsize(gz))), flush=True)
    outs = []
    for i, flag in enumerate(((), ("--gpu_parse",), (), ("--gpu_parse",))):
        out = tmp_path / ("bgzf_%d.bf" % i)
        r = run([TOOL, "--reads", gz, "-k", K, "-c", 3, "--bf", 200_000_000, "--sketch_bytes", 1 << 32, "-o", out] + list(flag),
                timeout=1800)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        found = TIMED_PASS_LINE.findall(r.stderr)
        assert [int(b) for _, b, _, _ in found] == [n_reads * 150] * 2, r.stderr
        lines = BGZF_LINE.findall(r.stderr)
        if flag:
            assert len(lines) == 2 and "unclean" not in r.stderr, r.stderr
            for _, files, comp, raw, _, handed_back, _, gzip_inputs in lines:
                assert (int(files), int(comp), int(raw), int(handed_back), int(gzip_inputs)) == (1, os.path.getsize(gz), inflated, 0, 0)
        else:
            assert not lines
        print(json.dumps(dict(gpu_parse=bool(flag), run=i // 2,
                              passes=[dict(pass_=p, wall_ms=float(w), gpu_ms=float(g)) for p, _, w, g in found],
                              bgzf=[dict(members=int(l[0]), compressed_bytes=int(l[2]), inflated_bytes=int(l[3]),
                                         inflate_kernel_ms=float(l[4]), handed_back=int(l[5])) for l in lines])), flush=True)
        outs.append(out.read_bytes())
        os.remove(out)
    assert outs[0] == outs[1] == outs[2] == outs[3]
