"""--gpu_parse for genome FASTA on the GPU: the device parser (ntedit_hip_genome_parse_device) against the serial model
of the stateful grammar, field by field, on the CPU tier's corpus at chunk sizes around the tile geometry and in every
entry state; files parsed chunk after chunk on the device against the model's whole-file text; ntedit-make-genome-bf
with and without the flag, byte for byte; and ntedit --genome against the tool followed by ntedit -r.

The yardstick for the front ends is the same build without the flag: that code path is the host parser's, unchanged."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bgzf_corpus as BC
import genome_corpus as GC
import helpers as H
from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
MKBF = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-genome-bf")
K = 25
T = _lib.PARSE_TILE
GENOME_LINE = re.compile(r"--gpu_parse: genome: (\d+) chunks parsed on the device \((\d+) raw bytes, (\d+) text bytes, ([\d.]+) ms in "
                         r"the parse kernels\), (\d+) files? handed back.*?; (\d+) files? left to the host parser")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_sketch_free(p._h)  # (the parser's scratch)
    p.close()


def device_parse(pol, raw, state=GC.LINE_START, first_chunk=True, on_device=False, guard=64):
    """-> (GenomeParseResult, text, the bytes behind the text buffer's cap)"""
    import torch
    n = len(raw)
    cap = (n + 15) // 16 * 16
    text = torch.full((cap + guard + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.GenomeParseResult()
    src = raw
    if on_device:
        dev = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
        src = dev.data_ptr()
    torch.cuda.synchronize()
    rc = pol._lib.ntedit_hip_genome_parse_device(pol._h, src, n, int(on_device), state, int(first_chunk), text.data_ptr(), cap, res)
    assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    host = bytes(text.cpu().numpy())
    return res, host[:res.text_len], host[cap:]


def check(pol, raw, state=GC.LINE_START, first_chunk=True, on_device=False):
    """the device against the model: the text, every field of the result, and nothing written behind text_cap"""
    mres, mtext = GC.model(pol._lib, raw, state, first_chunk)
    res, text, behind = device_parse(pol, raw, state, first_chunk, on_device)
    assert behind == b"\xEE" * len(behind)
    assert GC.fields(res) == GC.fields(mres), (len(raw), state, first_chunk, on_device)
    assert text == mtext, (len(raw), state, first_chunk, on_device)
    return res


# ---------------------------------------------------------------------------------- 1. the device parser
SIZES = [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5, 16 * T + 3]


@pytest.fixture(scope="module")
def files():
    """the corpus, and one file long enough for the largest chunk size"""
    rng = np.random.default_rng(11)
    c = dict(GC.well_formed())
    c.update(GC.odd())
    big = bytearray()
    i = 0
    while len(big) < 16 * T + 100:
        big += b">contig%d of the long file\n" % i
        seq = bytes(rng.choice(ACGT, 3000 + 977 * i))
        big += b"".join(seq[j:j + 60] + b"\n" for j in range(0, len(seq), 60)) if i % 2 == 0 else seq + b"\n"
        i += 1
    c["long_mixed"] = bytes(big)
    return c


@pytest.mark.parametrize("size", SIZES)
def test_corpus_chunks_in_every_entry_state(pol, files, size):
    done = 0
    for name, raw in sorted(files.items()):
        # the chunk of `size` bytes at the file's start, one from its middle and the one at its end
        starts = {0, max(0, len(raw) // 2 - size // 2), max(0, len(raw) - size)} if len(raw) > size else {0}
        for at in sorted(starts):
            chunk = raw[at:at + size]
            for state in GC.STATES:
                for on_device in (False, True):
                    check(pol, chunk, state, first_chunk=(at == 0 and state == GC.LINE_START), on_device=on_device)
                    done += 1
    assert done >= 6 * len(files)


def test_whole_corpus_files_host_and_device_input(pol, files):
    for name, raw in sorted(files.items()):
        for on_device in (False, True):
            res = check(pol, raw, on_device=on_device)
            assert bool(res.clean) == (name in GC.well_formed() or name == "long_mixed"), name


def lines_file(n_lines, width=19):
    """a FASTA file of exactly n_lines lines: a header and sequence lines of `width` bases, a new record every 7 lines"""
    out = []
    for i in range(n_lines):
        out.append(b">r%d\n" % i if i % 7 == 0 else bytes(ACGT[(np.arange(width) + i) % 4]) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("n_lines", [63, 64, 65, 2047, 2048, 2049])
def test_line_counts_around_the_wave_and_the_scan_block(pol, n_lines):
    raw = lines_file(n_lines)
    res = check(pol, raw)
    assert res.clean == 1 and res.lines == n_lines
    res = check(pol, raw[:-1], on_device=True)  # the last line without its '\n'
    assert res.lines == n_lines and res.state_out == (GC.IN_HEADER if (n_lines - 1) % 7 == 0 else GC.IN_SEQ)
    check(pol, raw[5:], GC.IN_HEADER, False)


def test_a_line_of_40000_bytes(pol):
    rng = np.random.default_rng(12)
    line = bytes(rng.choice(ACGT, 40000))
    res = check(pol, b">a\n" + line + b"\n>b\n" + line[:77] + b"\n")
    assert res.clean == 1 and res.bases == 40077
    check(pol, line, GC.IN_SEQ, False)                       # only the middle of that line
    check(pol, line[:30000] + b"\n" + line[30000:], GC.IN_SEQ, False, on_device=True)
    res = check(pol, b">" + b"h" * 39998 + b"\n" + line[:500] + b"\n")  # a header of 40,000 bytes
    assert res.text_len == 501


def test_chunks_that_are_only_a_piece_of_a_line(pol):
    res = check(pol, b"chr7 unlocalized scaffold 12, whole genome shotgun", GC.IN_HEADER, False)
    assert (res.clean, res.text_len, res.state_out, res.last_header) == (1, 0, GC.IN_HEADER, GC.NO_START)
    res = check(pol, b"\n", GC.IN_SEQ, False)
    assert (res.clean, res.text_len, res.state_out, res.lines) == (1, 0, GC.LINE_START, 1)
    res = check(pol, b"\n", GC.LINE_START, False)
    assert res.clean == 0 and res.broken == _lib.PARSE_BAD["empty"]
    res = check(pol, b"", GC.IN_SEQ, False)
    assert (res.clean, res.state_out) == (1, GC.IN_SEQ)


def test_over_the_table_nothing_is_written(pol):
    raw = b">a\n" + b"A\n" * 200_000
    res, text, behind = device_parse(pol, raw, guard=4096)
    assert (res.clean, res.broken, res.text_len) == (0, GC.TABLE, 0) and behind == b"\xEE" * len(behind)
    check(pol, raw)
    # ... within the table's slack the chunk is unclean and still parsed, and the next chunk is not disturbed
    res = check(pol, b">a\n" + b"A\n" * 100_000)
    assert res.broken == GC.TABLE and res.bases == 100_000
    check(pol, GC.well_formed()["wrapped_60"])


# ---------------------------------------------------------------------------------- 2. files, chunk after chunk
def device_chunks(pol, raw, size):
    parse = lambda chunk, state, first: device_parse(pol, chunk, state, first)[:2]
    return GC.run_chunks(parse, raw, list(range(size, len(raw), size)))


@pytest.fixture(scope="module")
def file_100k():
    rng = np.random.default_rng(13)
    out = bytearray()
    i = 0
    while len(out) < 100_000:
        seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), 7000 + 3301 * i))
        out += b">scaffold_%d len=%d\n" % (i, len(seq))
        out += b"".join(seq[j:j + 60] + b"\n" for j in range(0, len(seq), 60)) if i % 3 else seq + b"\n"
        i += 1
    return bytes(out)


@pytest.mark.parametrize("size", [4096, T, T + 1, None])
def test_a_100_kb_file_in_chunks_equals_the_models_whole_file_text(pol, file_100k, size):
    raw = file_100k
    whole, wtext = GC.model(pol._lib, raw)
    assert whole.clean == 1
    got = device_chunks(pol, raw, size or len(raw))
    assert got["text"] == wtext
    assert (got["bases"], got["last_header"], got["state"], got["broken"]) == (whole.bases, whole.last_header, whole.state_out, 0)


def test_a_2_kb_file_in_chunks_of_7_bytes(pol):
    # (a chunk of 7 bytes with a '\n' before its last byte is over its own line bound, 7 / 8 + 1: reported, and parsed
    # all the same, so the text is the whole file's whatever the chunks report)
    rng = np.random.default_rng(14)
    seqs = [bytes(rng.choice(ACGT, 150 + 31 * i)) for i in range(8)]
    raw = b"".join(b">c%d\n%s\n" % (i, s) if i < 4 else b">c%d\n%s" % (i, b"".join(s[j:j + 50] + b"\n" for j in range(0, len(s), 50)))
                   for i, s in enumerate(seqs))
    assert 1900 < len(raw) < 2300
    whole, wtext = GC.model(pol._lib, raw)
    got = device_chunks(pol, raw, 7)
    assert got["text"] == wtext
    assert (got["bases"], got["last_header"], got["state"]) == (whole.bases, whole.last_header, whole.state_out)
    assert got["broken"] & ~GC.TABLE == whole.broken == 0


# ---------------------------------------------------------------------------------- 3. the tool with and without the flag
def tool(args, ok=True):
    r = subprocess.run([MKBF] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def info_lines(r):
    """the --gpu_parse lines of a run -> [(chunks, raw bytes, text bytes, handed back, left to the host)]"""
    return [(int(c), int(rb), int(tb), int(hb), int(hf)) for c, rb, tb, _, hb, hf in GENOME_LINE.findall(r.stderr + r.stdout)]


def existing_lines(r):
    """the console lines the tool always had: stdout whole, and stderr without the flag's additions and the time stamps"""
    err = [re.sub(r"^\[[^\]]*\] \[INFO\] ", "", l) for l in r.stderr.splitlines()]
    return r.stdout, [l for l in err if "--gpu_parse" not in l and not re.match(r"(Sizing|Insert) pass: ", l)]


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_genome")
    rng = np.random.default_rng(21)
    g1 = [(b"chr1 x", H.random_genome(rng, 120000)), (b"tiny", b"ACGTACGT"), (b"low", H.random_genome(rng, 3000).lower()),
          (b"gap", H.random_genome(rng, 20000) + b"N" * 500 + H.random_genome(rng, 20000))]
    g2 = [(b"other", H.random_genome(rng, 50000)), (b"last", H.random_genome(rng, 777))]
    long_rec = [(b"unwrapped", H.random_genome(rng, 300_000)), (b"after", H.random_genome(rng, 5000))]
    H.write_fasta(str(d / "g1.fa"), g1, width=60)
    H.write_fasta(str(d / "g2.fa"), g2, width=80)
    H.write_fasta(str(d / "long.fa"), long_rec)
    raw = (d / "g1.fa").read_bytes()
    (d / "g1_300.fa.gz").write_bytes(BC.bgzf(raw, block=300))
    (d / "g1_65280.fa.gz").write_bytes(BC.bgzf(raw, block=65280))
    with gzip.open(d / "g1_stream.fa.gz", "wb") as f:
        f.write(raw)
    half = raw.index(b">gap")
    (d / "g1_crlf.fa").write_bytes(raw[:half] + raw[half:].replace(b"\n", b"\r\n"))
    return dict(dir=d, bases=dict(g1=sum(len(s) for _, s in g1), g2=sum(len(s) for _, s in g2), long=305_000))


def both_ways(genome, tag, files, args, batch=None):
    """the tool without and with --gpu_parse: the same filter file and the same existing lines -> (flagless, flagged, out)"""
    d = genome["dir"]
    runs = []
    for flag in ((), ("--gpu_parse",) + (("--batch_bytes", batch) if batch else ())):
        out = d / ("%s_%d.bf" % (tag, len(flag)))
        runs.append((tool(["--genome"] + [d / f for f in files] + ["-k", K, "-o", out] + list(args) + list(flag)), out))
    (r0, o0), (r1, o1) = runs
    assert o0.read_bytes() == o1.read_bytes(), tag
    fix = lambda lines, o: (lines[0].replace(str(o), "OUT"), [l.replace(str(o), "OUT") for l in lines[1]])
    assert fix(existing_lines(r0), o0) == fix(existing_lines(r1), o1)
    assert "--gpu_parse" not in r0.stderr + r0.stdout
    return r0, r1, o1


def chunks_of(genome, files, batch):
    return sum(-(-os.path.getsize(genome["dir"] / f) // batch) for f in files)


@pytest.mark.parametrize("tag,files,args,passes", [
    ("bf", ["g1.fa"], ["--bf", 1 << 20], 1),
    ("ne", ["g1.fa"], ["--num_elements", 200000, "--hashes", 4], 1),
    ("sized", ["g1.fa"], [], 2),
    ("two", ["g1.fa", "g2.fa"], [], 2),
])
def test_the_tool_is_identical_with_the_flag(genome, tag, files, args, passes):
    batch = 1 << 16
    r0, r1, out = both_ways(genome, tag, files, args, batch)
    raw = sum(os.path.getsize(genome["dir"] / f) for f in files)
    lines = info_lines(r1)
    assert len(lines) == passes, r1.stderr
    for chunks, raw_bytes, text_bytes, handed_back, host_files in lines:
        assert (chunks, raw_bytes, handed_back, host_files) == (chunks_of(genome, files, batch), raw, 0, 0), r1.stderr
        assert 0 < text_bytes < raw
    if passes == 2:
        want = "Genome size (bp): %d" % sum(genome["bases"][f[:-3]] for f in files)
        assert want in r0.stdout and want in r1.stdout
    if tag == "bf":
        H.mkbf([str(genome["dir"] / "g1.fa")], str(genome["dir"] / "mk.bf"), k=K, hashes=3, nbytes=1 << 20)
        assert out.read_bytes() == (genome["dir"] / "mk.bf").read_bytes()


def test_the_default_batch_takes_a_small_file_in_one_chunk(genome):
    _, r1, _ = both_ways(genome, "one", ["g1.fa"], ["--bf", 1 << 18])
    assert [l[0] for l in info_lines(r1)] == [1]


def test_a_batch_smaller_than_the_longest_line(genome):
    batch = 40_000
    _, r1, _ = both_ways(genome, "long", ["long.fa"], [], batch)
    lines = info_lines(r1)
    assert len(lines) == 2 and "Genome size (bp): 305000" in r1.stdout
    for chunks, raw_bytes, _, handed_back, host_files in lines:
        assert (chunks, handed_back, host_files) == (chunks_of(genome, ["long.fa"], batch), 0, 0) and chunks >= 8


@pytest.mark.parametrize("block", [300, 65280])
def test_the_same_genome_as_bgzf(genome, block):
    d = genome["dir"]
    name = "g1_%d.fa.gz" % block
    batch = 1 << 16
    _, r1, out = both_ways(genome, "bgzf%d" % block, [name], [], batch)
    plain = tool(["--genome", d / "g1.fa", "-k", K, "-o", d / "plain.bf"])
    assert out.read_bytes() == (d / "plain.bf").read_bytes()
    assert "Genome size (bp): %d" % genome["bases"]["g1"] in r1.stdout
    raw = os.path.getsize(d / "g1.fa")
    lines = info_lines(r1)
    assert len(lines) == 2
    for chunks, raw_bytes, _, handed_back, host_files in lines:
        # whole members whose inflated sizes stay within the batch
        per_chunk = batch // block * block
        assert (raw_bytes, handed_back, host_files) == (raw, 0, 0) and chunks == -(-raw // per_chunk), r1.stderr
    members = -(-raw // block) + 1  # (and the empty member at the end)
    assert (r1.stderr + r1.stdout).count("BGZF: %d members of 1 file inflated on the device" % members) == 2, r1.stderr


# ---------------------------------------------------------------------------------- 4. hand-back and damage
def test_a_file_whose_second_half_is_crlf_is_handed_back(genome):
    _, r1, _ = both_ways(genome, "crlf", ["g1_crlf.fa"], [], 1 << 16)
    lines = info_lines(r1)
    assert len(lines) == 2 and all(l[3] == 1 and l[4] == 0 and l[0] >= 1 for l in lines), r1.stderr
    assert (r1.stderr + r1.stdout).count("1 file handed back to the host parser (a carriage return)") == 2


def test_a_single_stream_gz_is_left_to_the_host(genome):
    _, r1, _ = both_ways(genome, "stream", ["g1_stream.fa.gz"], [], 1 << 16)
    lines = info_lines(r1)
    assert len(lines) == 2 and all(l == (0, 0, 0, 0, 1) for l in lines), r1.stderr


def test_a_damaged_bgzf_file_fails_with_and_without_the_flag(genome):
    d = genome["dir"]
    blob = bytearray((d / "g1_65280.fa.gz").read_bytes())
    blob[1000] ^= 0x10  # (inside the first member's DEFLATE data)
    (d / "bad.fa.gz").write_bytes(bytes(blob))
    for flag in ([], ["--gpu_parse"]):
        for size in ([], ["--bf", 1 << 18]):
            r = tool(["--genome", d / "bad.fa.gz", "-k", K, "-o", d / "bad.bf"] + size + flag, ok=False)
            assert r.returncode == 1 and "make_genome_bf: error: " in r.stderr, (flag, size, r.stderr)
    assert "is damaged" in r.stderr


# ---------------------------------------------------------------------------------- 5. ntedit --genome
def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def polish_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_genome_polish")
    rng = np.random.default_rng(44)
    truth = H.random_genome(rng, 120000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:70000]), (b"ctg2", draft[70000:])], width=80)
    H.write_fasta(str(d / "truth1.fa"), [(b"t1", truth[:50000]), (b"t2", truth[50000:90000])], width=60)
    H.write_fasta(str(d / "truth2.fa"), [(b"t3", truth[89000:])])
    genomes = [d / "truth1.fa", d / "truth2.fa"]
    tool(["--genome"] + genomes + ["-k", K, "-o", d / "tool.bf"])
    return dict(dir=d, draft=d / "draft.fa", genomes=genomes, bf=d / "tool.bf")


@pytest.mark.parametrize("mode", ["default", "snv"])
def test_ntedit_genome_equals_the_tool_followed_by_ntedit_r(polish_case, mode):
    c = polish_case
    d = c["dir"]
    extra = ["-s", 1] if mode == "snv" else []

    def ntedit(args, prefix):
        r = subprocess.run([str(x) for x in [NTEDIT, "-f", c["draft"], "-b", prefix] + args + extra], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r

    ref = d / ("ref_" + mode)
    ntedit(["-r", c["bf"]], ref)
    for flag in ((), ("--gpu_parse", "--batch_bytes", 30000)):
        p = d / ("g_%s_%d" % (mode, len(flag)))
        r = ntedit(["--genome"] + c["genomes"] + ["-k", K, "--save_bf", str(p) + ".bf"] + list(flag), p)
        for suffix in ("_edited.fa", "_changes.tsv"):
            assert read(str(p) + suffix) == read(str(ref) + suffix), (suffix, flag)
        assert H.vcf_body(str(p) + "_variants.vcf") == H.vcf_body(str(ref) + "_variants.vcf")
        assert read(str(p) + ".bf") == read(c["bf"])
        lines = info_lines(r)
        if flag:
            raw = sum(os.path.getsize(g) for g in c["genomes"])
            assert len(lines) == 2 and all(l[1] == raw and l[3:] == (0, 0) and l[0] >= 4 for l in lines), r.stderr
        else:
            assert not lines and "--gpu_parse" not in r.stderr
