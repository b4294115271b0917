"""--gpu_parse on BAM reads, on the GPU: the walk and decode kernels (ntedit_hip_reads_bam_device) against the serial host
model in every result field and every text byte, at forced segment sizes, with the stitch's repairs counted; carried
chunks; and the front ends on a BAM against its twin FASTQ with the host parser (tests/bam_corpus.py builds the inputs;
the CPU tier is tests/test_reads_bam_cpu.py)."""
import ctypes
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_corpus as BAM
import helpers as H
from ntedit_amd import _lib
from reads_model import simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL
from test_reads_bam_cpu import damaged_inputs, small_case

pytestmark = pytest.mark.gpu

K = BAM.K
GUARD = 256
PASS_LINE = re.compile(r"Pass (\S+) \([^)]*\): (\d+) bases")
BAM_LINE = re.compile(r"--gpu_parse: BAM: (\d+) records of (\d+) files? walked on the device \((\d+) kept, (\d+) secondary or "
                      r"supplementary, (\d+) too short; (\d+) chunks, (\d+) segments, (\d+) walked again by the stitch, ")


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_reads_bam_set_segment(p._h, 0)
    p._lib.ntedit_hip_sketch_free(p._h)  # (the walk, inflate and parse scratch)
    p.close()


@pytest.fixture(scope="module")
def corpus():
    return BAM.corpus()


@pytest.fixture(scope="module")
def models(corpus):
    """the model's result and text of every case, computed once"""
    lib = _lib.load()
    return {c.name: BAM.model(lib, c.raw, 1, K)[1:] for c in corpus}


def stats(pol):
    st = _lib.ReadsBamStats()
    assert pol._lib.ntedit_hip_reads_bam_info(pol._h, st) == 0
    return st


def device_bam(pol, raw, at_header=1, min_len=K, on_device=False, segment=0):
    """-> (the result fields, the text); the 0xEE guards in front of and behind text_cap bytes are checked"""
    import torch
    assert pol._lib.ntedit_hip_reads_bam_set_segment(pol._h, segment) == 0
    cap = len(raw)
    out = torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    src = raw
    if on_device:
        dev = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
        src = dev.data_ptr()
    torch.cuda.synchronize()
    res = _lib.ReadsBamResult()
    rc = pol._lib.ntedit_hip_reads_bam_device(pol._h, src, len(raw), int(on_device), at_header, min_len, out.data_ptr() + GUARD, cap, res)
    assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    host = bytes(out.cpu().numpy())
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + cap:] == b"\xEE" * GUARD
    r = BAM.result_dict(res)
    if r["clean"]:
        assert host[GUARD + r["text_len"]:GUARD + cap] == b"\xEE" * (cap - r["text_len"])  # nothing behind the text
    return r, host[GUARD:GUARD + r["text_len"]] if r["clean"] else b""


# ---------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("on_device", [False, True], ids=["host_input", "device_input"])
@pytest.mark.parametrize("segment", [256, 4096, 0], ids=["segment_256", "segment_4096", "segment_default"])
def test_the_device_equals_the_model_on_the_corpus(pol, corpus, models, segment, on_device):
    """256-byte segments: the 70,000-base record and the 150 KB header span hundreds of segments, most segments of the
    long reads hold no record start; the decoys sit at multiples of 8192, a segment start at every size"""
    for c in corpus:
        before = stats(pol)
        got, text = device_bam(pol, c.raw, 1, K, on_device, segment)
        want, want_text = models[c.name]
        assert got == want, (c.name, got, want)
        assert text == want_text, c.name
        after = stats(pol)
        assert after.chunks == before.chunks + 1 and after.records == before.records + want["records"]
        assert after.segments - before.segments == (len(c.raw) + (segment or _lib.BAM_SEGMENT) - 1) // (segment or _lib.BAM_SEGMENT)
        if c.decoy:
            # the guesses landed on the images in the quality strings and the B array: without a repair this shows nothing
            assert after.rewalked - before.rewalked >= 1, (c.name, segment)


def test_min_len_and_one_chain(pol, corpus, models):
    """min_len 0 and 1 (the reads of no and one base are kept), and a segment of the chunk's size: one chain, no guess"""
    lib = _lib.load()
    for c in corpus:
        if c.name in ("lengths_and_codes", "names_cigars_aux"):
            for min_len in (0, 1):
                assert device_bam(pol, c.raw, 1, min_len, False, 256) == BAM.model(lib, c.raw, 1, min_len)[1:], (c.name, min_len)
        before = stats(pol)
        assert device_bam(pol, c.raw, 1, K, False, 1 << 30) == models[c.name], c.name
        after = stats(pol)
        assert after.segments - before.segments == 1 and after.rewalked == before.rewalked


def test_the_cut_at_every_offset_on_the_device(pol):
    """the small case ended at every offset, with the header and as a carried chunk (at_header = 0), 64-byte segments"""
    lib = _lib.load()
    head, recs = small_case()
    raw = head + b"".join(recs)
    for at_header, buf in ((1, raw), (0, raw[len(head):])):
        for n in range(len(buf) + 1):
            assert device_bam(pol, buf[:n], at_header, K, n % 2 == 1, 64) == BAM.model(lib, buf[:n], at_header, K)[1:], (at_header, n)


@pytest.mark.parametrize("segment", [256, 0])
def test_carried_chunks_concatenate_to_the_files_text(pol, corpus, models, segment):
    """chunks as the pass makes them: each ends anywhere, its bytes from the cut on go in front of the next one"""
    rng = np.random.default_rng(5)
    for c in corpus:
        if c.name not in ("one_reference", "lengths_and_codes", "header_longer_than_a_member", "decoys"):
            continue
        raw, at, text, fields = c.raw, 0, b"", dict.fromkeys(("records", "kept", "skipped_flag", "skipped_short", "bases"), 0)
        ends = sorted(int(x) for x in rng.integers(1, len(raw), size=6)) + [len(raw)]
        for end in ends:
            got, t = device_bam(pol, raw[at:end], 1 if at == 0 else 0, K, True, segment)
            assert got["clean"] == 1, (c.name, at, end, got)
            if at == 0:
                assert (got["cut"] == 0) == (end < c.header_len), (c.name, end)  # a header that does not fit: the chunk grows
            text += t
            for f in fields:
                fields[f] += got[f]
            at += got["cut"]
        want, want_text = models[c.name]
        assert at == len(raw) and text == want_text and all(fields[f] == want[f] for f in fields), c.name


def test_damaged_inputs_get_the_models_verdict_on_the_device(pol):
    """the bounds checks of the walk: every length that lies is met by a hop that checked it first"""
    lib = _lib.load()
    for name, (raw, bit, at) in damaged_inputs().items():
        for segment in (64, 0):
            got, _ = device_bam(pol, raw, 1, K, False, segment)
            assert got == BAM.model(lib, raw, 1, K)[1] and got["broken"] == bit and got["cut"] == at, (name, segment, got)


# ---------------------------------------------------------------------------------- 2. the front ends
def run(args, timeout=600):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def passes_of(r):
    return [(name, int(bases)) for name, bases in PASS_LINE.findall(r.stderr)]


def bam_of(reads, rng):
    """reads as BAM records with mixed flags, a secondary or supplementary copy of some in between -> (raw, the twin)"""
    recs = []
    for i, s in enumerate(reads):
        flag = (0, 0x10, 0x4, 0x1 | 0x40, 0x1 | 0x80 | 0x10)[i % 5]
        recs.append((b"r%d" % i, flag, s))
        if i % 7 == 0:
            recs.append((b"r%d" % i, (0x100, 0x800, 0x900 | 0x10)[i % 3], s[:len(s) // 2] if i % 2 else s))
    aux = BAM.all_aux()
    raw = BAM.header(b"@HD\tVN:1.6\n", [(b"chr1", 100000)]) + b"".join(
        BAM.record(n, f, s, cigar=((len(s) << 4,) if i % 2 else ()), aux=aux if i % 3 == 0 else b"", ref=0, pos=i)
        for i, (n, f, s) in enumerate(recs))
    return raw, BAM.twin(recs), recs


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_bam")
    rng = np.random.default_rng(1951)
    genome = H.random_genome(rng, 10000)
    sim = [bytes(r) for r in simulate_reads(rng, genome, 30)]
    raw, twin, recs = bam_of(sim, rng)
    (d / "x.bam").write_bytes(BAM.bgzf(raw, sizes=(300,)))
    (d / "x65280.bam").write_bytes(BAM.bgzf(raw, sizes=(65280,), eof=False))
    (d / "twin.fq").write_bytes(twin)
    return dict(dir=d, raw=raw, recs=recs)


SMALL = ["-k", K, "-c", 2, "--bf", 2000000, "--batch_bytes", 4096]


def tool(args):
    r = run([TOOL] + list(args))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


CASES = ("unaligned_header", "one_reference", "300_references", "header_longer_than_a_member", "lengths_and_codes",
         "names_cigars_aux", "random_members", "members_cut_records", "no_eof_member", "long_reads", "header_only", "decoys")


def test_the_case_list_is_the_corpus(corpus):
    assert tuple(c.name for c in corpus) == CASES


@pytest.mark.parametrize("name", CASES)
def test_the_pass_on_every_case_file_equals_the_twin(corpus, tmp_path, name):
    """every case as a file, with its own member layout, through the pass in chunks of 4 KiB: members of 1 to 65,280 bytes,
    a member boundary at each of the first 40 bytes of a record, a header of 150 KB that takes many chunks to fit (cut 0,
    the chunk grows), a record of 70,000 bases, far longer than a chunk, no EOF member; the filter is the twin's through
    the host parser, and the BAM line has the case's counts"""
    c = [c for c in corpus if c.name == name][0]
    (tmp_path / "x.bam").write_bytes(c.bam)
    r1 = tool(["--reads", tmp_path / "x.bam", "-o", tmp_path / "bam.bf", "--gpu_parse"] + SMALL)
    lines = BAM_LINE.findall(r1.stderr)
    assert len(lines) == 2, r1.stderr
    by_flag = sum(1 for _, f, _ in c.reads if f & 0x900)
    short = sum(1 for _, f, s in c.reads if not f & 0x900 and len(s) < K)
    for records, files, kept, got_flag, got_short, chunks, _, _ in lines:
        assert (int(records), int(files), int(got_flag), int(got_short)) == (len(c.reads), 1, by_flag, short), r1.stderr
        assert int(kept) == len(c.reads) - by_flag - short
        assert int(chunks) >= 1  # (a chunk is whole members: a case in one 65,280-byte member is one chunk)
    bases = sum(len(s) for _, f, s in c.reads if not f & 0x900 and len(s) >= K)
    assert passes_of(r1) == [("1", bases), ("2", bases)], r1.stderr
    assert "handed back to the host parser" not in r1.stderr and "0 chunks parsed on the device" in r1.stderr
    if c.twin:
        (tmp_path / "twin.fq").write_bytes(c.twin)
        r0 = tool(["--reads", tmp_path / "twin.fq", "-o", tmp_path / "twin.bf"] + SMALL)
        assert (tmp_path / "twin.bf").read_bytes() == (tmp_path / "bam.bf").read_bytes()
        assert passes_of(r0) == passes_of(r1)
    else:
        assert name == "header_only" and bases == 0


@pytest.mark.parametrize("name", ["x.bam", "x65280.bam"])
def test_the_tool_writes_the_twins_filter(reads, name):
    d = reads["dir"]
    r0 = tool(["--reads", d / "twin.fq", "-o", d / "twin.bf"] + SMALL)
    r1 = tool(["--reads", d / name, "-o", d / (name + ".bf"), "--gpu_parse"] + SMALL)
    assert (d / "twin.bf").read_bytes() == (d / (name + ".bf")).read_bytes()
    assert passes_of(r0) == passes_of(r1) and len(passes_of(r0)) == 2
    lines = BAM_LINE.findall(r1.stderr)
    assert len(lines) == 2, r1.stderr
    recs = reads["recs"]
    skipped = sum(1 for _, f, _ in recs if f & 0x900)
    short = sum(1 for _, f, s in recs if not f & 0x900 and len(s) < K)
    for records, files, kept, by_flag, by_len, chunks, _, _ in lines:
        assert (int(records), int(files), int(by_flag), int(by_len)) == (len(recs), 1, skipped, short)
        assert int(kept) == len(recs) - skipped - short
        assert int(chunks) > (20 if name == "x.bam" else 2)  # several chunks, and so several carries
    assert "handed back to the host parser" not in r1.stderr


def test_solid_and_hist_are_the_twins(reads):
    d = reads["dir"]
    args = ["-k", K, "--solid", "--batch_bytes", 4096]
    tool(["--reads", d / "twin.fq", "-o", d / "s_twin.bf", "--hist", d / "s_twin.hist"] + args)
    r1 = tool(["--reads", d / "x.bam", "-o", d / "s_bam.bf", "--hist", d / "s_bam.hist", "--gpu_parse"] + args)
    assert (d / "s_twin.bf").read_bytes() == (d / "s_bam.bf").read_bytes()
    assert (d / "s_twin.hist").read_bytes() == (d / "s_bam.hist").read_bytes()
    assert len(BAM_LINE.findall(r1.stderr)) == 3, r1.stderr


def test_make_reads_world_2_gloo_on_two_bams_equals_the_tool_on_the_twins(reads):
    """the sharded driver: a BAM is one unit, as a gzip file is; each rank walks one of the two on its device"""
    from test_gpu_reads_multi import _driver
    d = reads["dir"]
    cut = ["-k", str(K), "-c", "2", "--bf", str(1 << 16), "--sketch_bytes", "1000003"]
    tool(["--reads", d / "twin.fq", d / "twin.fq", "-o", d / "mr_ref.bf"] + cut)
    r = _driver(2, ["--reads", str(d / "x.bam"), str(d / "x65280.bam"), "-o", str(d / "mr_w2.bf"), "--gpu_parse"] + cut, "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert (d / "mr_w2.bf").read_bytes() == (d / "mr_ref.bf").read_bytes()
    assert "handed back to the host parser" not in r.stderr
    # ... and without the flag it refuses, as the tool does, before any rank opens a device
    r = _driver(2, ["--reads", str(d / "x.bam"), "-o", str(d / "mr_no.bf")] + cut, "gloo")
    assert r.returncode != 0 and "--reads %s: BAM needs --gpu_parse" % (d / "x.bam") in r.stderr + r.stdout
    assert not (d / "mr_no.bf").exists()


POLISH = ["-k", K, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", 1 << 22, "--batch_bytes", 1 << 16]


@pytest.fixture(scope="module")
def polished(tmp_path_factory):
    """a draft, its reads as BAM and as the twin, and `ntedit --reads` on both: the twin with the host parser"""
    tmp_path = tmp_path_factory.mktemp("gpu_bam_polish")
    rng = np.random.default_rng(44)
    truth = H.random_genome(rng, 40000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft[:25000]), (b"ctg2", draft[25000:])], width=80)
    raw, twin, _ = bam_of([bytes(r) for r in simulate_reads(rng, truth, 30)], rng)
    (tmp_path / "x.bam").write_bytes(BAM.bgzf(raw, sizes=(5000,)))
    (tmp_path / "twin.fq").write_bytes(twin)
    outs = {}
    for tag, extra in (("twin", ["--reads", tmp_path / "twin.fq"]), ("bam", ["--reads", tmp_path / "x.bam", "--gpu_parse"])):
        p = tmp_path / tag
        r = run([NTEDIT, "-f", tmp_path / "draft.fa", "-b", p] + extra + POLISH)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[tag] = (p, r)
    return dict(dir=tmp_path, outs=outs)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_ntedit_reads_on_a_bam_writes_the_twins_outputs(polished):
    (twin, _), (bam, r) = polished["outs"]["twin"], polished["outs"]["bam"]
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(twin) + suffix) == read(str(bam) + suffix), suffix
    assert len(read(str(bam) + "_changes.tsv").splitlines()) > 10
    assert BAM_LINE.search(r.stderr + r.stdout), r.stderr[-3000:]


def test_run_reads_on_a_bam_writes_the_twins_outputs(polished):
    """python -m ntedit_amd.run --reads x.bam --gpu_parse, one process: the files of `ntedit --reads` on the twin, and the
    BAM counts in --report"""
    from test_gpu_reads_run import driver, reports
    d = polished["dir"]
    p = d / "run_bam"
    r = driver(0, ["-f", d / "draft.fa", "--reads", d / "x.bam", "--gpu_parse", "-b", p, "--report"] + POLISH)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    twin = polished["outs"]["twin"][0]
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(twin) + suffix) == read(str(p) + suffix), suffix
    parse = reports(r)[0]["reads"]["parse"]["1"]
    m = BAM_LINE.search(polished["outs"]["bam"][1].stderr + polished["outs"]["bam"][1].stdout)
    assert parse["bam"]["files"] == 1 and parse["bam"]["records"] == int(m.group(1)) and parse["bam"]["kept"] == int(m.group(3))
    assert parse["device_chunks"] == 0 and parse["fallback_chunks"] == 0 and parse["host_files"] == 0
    # ... and without the flag it is refused before anything is written
    r = driver(0, ["-f", d / "draft.fa", "--reads", d / "x.bam", "-b", d / "run_no"] + POLISH)
    assert r.returncode != 0 and "--reads %s: BAM needs --gpu_parse" % (d / "x.bam") in r.stderr + r.stdout
    assert not [f for f in d.iterdir() if f.name.startswith("run_no")]


def test_truncated_and_damaged_bams_fail_the_pass_in_one_line(reads):
    """the bounds checks end to end: each run ends cleanly, with a non-zero status and one line that names the file and the
    inflated offset"""
    d, raw = reads["dir"], reads["raw"]
    whole = (d / "x.bam").read_bytes()
    third = len(raw) // 3
    at = raw.find(b"r700\0") - 36  # the record named r700: its read name's length to 0
    assert at > third
    cases = {
        "cut_in_a_member.bam": whole[:len(whole) // 2],                      # the file ends inside a BGZF member
        "cut_in_a_record.bam": BAM.bgzf(raw[:third], sizes=(300,)),          # whole members, the last record is not
        "cut_in_block_size.bam": BAM.bgzf(raw[:at + 2], sizes=(300,), eof=False),
        "damaged_record.bam": BAM.bgzf(raw[:at + 12] + b"\0" + raw[at + 13:], sizes=(300,)),
        "garbage_behind.bam": BAM.bgzf(raw[:at], sizes=(300,), eof=False) + b"not a BGZF member at all" * 4,
    }
    for name, data in cases.items():
        (d / name).write_bytes(data)
        out = d / (name + ".bf")
        r = run([TOOL, "--reads", d / name, "-o", out, "--gpu_parse"] + SMALL)
        assert r.returncode not in (0, -6, -11, 134, 139) and not out.exists(), (name, r.returncode, r.stderr[-2000:])
        lines = [l for l in r.stderr.splitlines() if "%s: BAM: " % (d / name) in l]
        assert len(lines) == 1 and re.search(r"at inflated offset \d+$", lines[0]), (name, r.stderr[-2000:])
        if name == "damaged_record.bam":
            assert lines[0].endswith("at inflated offset %d" % at), lines[0]
