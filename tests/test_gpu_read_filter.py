"""--min_read_len, --min_mean_qual and --min_rq on the GPU: k_rp_qsum and the filtering k_rp_records of the text parser, and
k_bam_facts with the filtering k_bam_sums / k_bam_compact of the BAM unit, against their serial models and the twin's
counts at the shapes where a line index, a segmented sum or a quality address can go wrong; the same through BGZF; an
unclean chunk handed back; and the four front ends by the twin -- the filter built with the options from a file equals,
byte for byte, the filter built without them from the same reads with the dropped ones deleted
(tests/read_filter_twin.py; the CPU tier is tests/test_read_filter_cpu.py)."""
import ctypes
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_corpus as BAM
import helpers as H
import min_qual_twin as MQ
import parse_corpus as PC
import read_filter_twin as RF
from ntedit_amd import _lib
from reads_model import simulate_reads

pytestmark = pytest.mark.gpu

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
K = RF.K
Q = 20
R = 0.99
T = _lib.PARSE_TILE
GUARD = 256
FILTER_LINE = re.compile(r"read filter: (\d+) of (\d+) records dropped \(length (\d+), rq (\d+), mean quality (\d+)\)")


@pytest.fixture(scope="module")
def pol():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    yield p
    p._lib.ntedit_hip_reads_set_read_filter(p._h, 0, 0, 0.0)
    p._lib.ntedit_hip_reads_set_min_qual(p._h, 0)
    p._lib.ntedit_hip_reads_bam_set_segment(p._h, 0)
    p._lib.ntedit_hip_reads_bam_set_group_width(p._h, 0)
    p._lib.ntedit_hip_sketch_free(p._h)  # (the parser's scratch)
    p.close()


def stats(pol):
    st = _lib.ReadsReadFilterStats()
    assert pol._lib.ntedit_hip_reads_read_filter_info(pol._h, st) == 0
    return RF.stats_dict(st)


def grown(before, after):
    return {name: after[name] - before[name] for name in after}


def device_parse(pol, raw, k, L=0, Qm=0, q=0):
    """ntedit_hip_reads_parse_device under the filter -> (the result, the text when clean, what the counts grew by)"""
    import torch
    lib = pol._lib
    assert lib.ntedit_hip_reads_set_read_filter(pol._h, L, Qm, 0.0) == 0 and lib.ntedit_hip_reads_set_min_qual(pol._h, q) == 0
    cap = (len(raw) + 15) // 16 * 16
    text = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsParseResult()
    before = stats(pol)
    torch.cuda.synchronize()
    rc = lib.ntedit_hip_reads_parse_device(pol._h, raw, len(raw), 0, k, text.data_ptr(), cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(pol._h)
    torch.cuda.synchronize()
    host = bytes(text.cpu().numpy())
    assert host[cap:] == b"\xEE" * GUARD
    return res, host[:res.text_len] if res.clean else None, grown(before, stats(pol))


def check_parse(pol, recs, raw, k=K, L=0, Qm=Q, discriminating=True):
    """the device against the model -- text, reads, bases, counts -- and both against the twin"""
    lib = pol._lib
    if discriminating:
        RF.assert_discriminating(recs, k, [RF.MEAN_QUAL] + ([RF.LENGTH] if L else []), L=L, Q=Qm)
    mres, mtext, mst = RF.parse_model_f(lib, raw, k, 0, L, Qm)
    res, text, grew = device_parse(pol, raw, k, L, Qm)
    assert mres.clean == 1 and res.clean == 1, (res.broken, mres.broken)
    assert text == mtext and (res.reads, res.bases, res.text_len) == (mres.reads, mres.bases, mres.text_len)
    assert mtext == RF.text_of(recs, k, L=L, Q=Qm)
    assert grew == mst and RF.same_counts(grew, RF.counts(recs, k, L=L, Q=Qm)), (grew, mst)
    # ... and off is the text without the options, with nothing counted
    res, text, grew = device_parse(pol, raw, k)
    assert text == PC.model(lib, raw, k)[1] and not any(grew.values())


def records_of_size(rng, size):
    """FASTQ records of 100 bases, quality levels around Q, whose 4-line layout is exactly `size` bytes"""
    recs, used = [], 0
    while size - used > 500:
        recs.append(RF.draw_read(rng, b"s%d_" % len(recs), 100, Q))
        used = len(RF.fastq_of(recs))
    left = size - used  # one more record "@t..\nS\n+\nQ\n": name + 2 n + 6 bytes
    name = b"t" if left % 2 == 1 else b"tt"
    recs.append(RF.draw_read(rng, name, (left - 6 - len(name)) // 2, Q))
    assert len(RF.fastq_of(recs)) == size
    return recs


# ---------------------------------------------------------------------------------- 1. k_rp_qsum and k_rp_records
@pytest.mark.parametrize("size", [T - 1, T, T + 1])
def test_chunks_of_one_tile_and_its_neighbours(pol, size):
    recs = records_of_size(random.Random(size), size)
    check_parse(pol, recs, RF.fastq_of(recs))
    check_parse(pol, recs, RF.fastq_of(recs), Qm=Q + 1)


@pytest.mark.parametrize("where", ["starts_on_the_last_byte", "ends_on_the_last_byte"])
@pytest.mark.parametrize("level", [Q, Q - 1])
def test_a_quality_line_at_a_tile_boundary(pol, where, level):
    """a quality line whose first byte, or whose last byte, is a tile's last byte; all its bases at Q (kept) or one at
    Q - 1 (dropped), so that a byte lost or counted twice at the boundary changes the verdict"""
    rng = random.Random(7)
    first = RF.draw_reads(rng, 1, Q, lengths=(300, 300), tag=b"first")
    n = 200
    # "@" name "\n" n bases "\n+\n" then the quality line: its first byte at T - 1, or its last byte there
    at = T - 1 if where == "starts_on_the_last_byte" else T - n
    name = b"edge" + b"x" * (at - len(RF.fastq_of(first)) - 1 - 4 - 1 - n - 3)
    qual = bytearray([33 + Q]) * n
    if level != Q:
        qual[0 if where == "starts_on_the_last_byte" else n - 1] = 33 + level  # (the byte that lies on the boundary)
    recs = first + [(name, bytes(rng.choice(b"ACGT") for _ in range(n)), bytes(qual), None)] + RF.draw_reads(rng, 40, Q, tag=b"after")
    raw = RF.fastq_of(recs)
    assert raw[at:at + n] == bytes(qual) and raw[at + n] == 10
    assert RF.reason(recs[1], K, Q=Q) == (None if level == Q else RF.MEAN_QUAL)
    check_parse(pol, recs, raw)


@pytest.mark.parametrize("verdict", ["just_passing", "just_failing"])
def test_one_record_of_300_kb(pol, verdict):
    """its quality line spans 19 tiles: every lane's piece is one run of the line, every wavefront adds its sum by one
    atomic, and the sum is exact to the last unit -- at the threshold the read is kept, one unit above it is dropped"""
    rng = np.random.default_rng(4)
    n = 300_000
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    # S = n * E[Q] exactly: half the bases at Q + 1 and Q - 1 would not sum to it, so take all at Q ...
    qual = bytearray([33 + Q]) * n
    if verdict == "just_failing":
        qual[n // 2] = 33 + Q - 1  # ... and one base a step lower
    short = RF.draw_reads(random.Random(1), 6, Q, lengths=(50, 200), tag=b"short")
    recs = short[:3] + [(b"long", seq, bytes(qual), None)] + short[3:]
    assert RF.reason(recs[3], K, Q=Q) == (None if verdict == "just_passing" else RF.MEAN_QUAL)
    check_parse(pol, recs, RF.fastq_of(recs), discriminating=False)


@pytest.fixture(scope="module")
def ten_thousand():
    """10^4 reads of 1..400 bases, quality levels around Q: lanes cross several line ends within their 16 bytes"""
    return RF.draw_reads(random.Random(5), 10_000, Q, tag=b"read")


def test_ten_thousand_reads_of_every_length(pol, ten_thousand):
    check_parse(pol, ten_thousand, RF.fastq_of(ten_thousand))
    check_parse(pol, ten_thousand, RF.fastq_of(ten_thousand), L=120, Qm=Q + 1)


def test_the_same_through_bgzf(pol, ten_thousand, tmp_path):
    """the 10^4-read set as BGZF: the pass over the file, inflated and parsed in HBM with no chunk handed back -- its
    sketch is the sketch of the twin file (the kept reads, plain, without the options), its counts the twin's"""
    import bgzf_corpus as BZ
    lib, h = pol._lib, pol._h
    recs = ten_thousand
    f = dict(L=60, Q=Q)
    want = RF.assert_discriminating(recs, K, [RF.LENGTH, RF.MEAN_QUAL], **f)
    (tmp_path / "r.fq.gz").write_bytes(BZ.bgzf(RF.fastq_of(recs), block=20000))
    (tmp_path / "twin.fq").write_bytes(RF.fastq_of(RF.kept(recs, K, **f)))
    sketches = {}
    for name, path, parse, L, Qm in (("bgzf", "r.fq.gz", 1, 60, Q), ("twin", "twin.fq", 0, 0, 0)):
        assert lib.ntedit_hip_sketch_alloc(h, 1 << 22, 3, K) == 0
        assert lib.ntedit_hip_reads_set_device_parse(h, parse) == 0 and lib.ntedit_hip_reads_set_read_filter(h, L, Qm, 0.0) == 0
        assert lib.ntedit_hip_reads_set_min_qual(h, 0) == 0
        files = (ctypes.c_char_p * 1)(str(tmp_path / path).encode())
        st = _lib.ReadsPassStats()
        rc = lib.ntedit_hip_reads_pass(h, _lib.READS_PASS_COUNT, files, (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)((1 << 64) - 1), 1,
                                       1 << 18, 0, st, None, None)
        assert rc == 0, lib.ntedit_hip_reads_last_error(h)
        sk = np.zeros(1 << 22, dtype=np.uint8)
        assert lib.ntedit_hip_sketch_download(h, sk.ctypes.data) == 0
        sketches[name] = (sk, st.bases, stats(pol))
        if parse:
            ps, zs = _lib.ReadsParseStats(), _lib.ReadsInflateStats()
            assert lib.ntedit_hip_reads_parse_info(h, ps) == 0 and lib.ntedit_hip_reads_inflate_info(h, zs) == 0
            assert ps.fallback_chunks == 0 and ps.broken == 0 and ps.host_files == 0 and ps.device_chunks > 5
            assert zs.files == 1 and zs.handed_back == 0
        lib.ntedit_hip_sketch_free(h)
    lib.ntedit_hip_reads_set_device_parse(h, 0)
    assert (sketches["bgzf"][0] == sketches["twin"][0]).all() and sketches["bgzf"][0].any()
    assert sketches["bgzf"][1] == sketches["twin"][1] == sum(len(s) for _, s, _, _ in RF.kept(recs, K, **f))
    assert RF.same_counts(sketches["bgzf"][2], want) and not any(sketches["twin"][2].values())


def test_a_chunk_whose_last_line_has_no_newline(pol):
    """the last quality line ends with the chunk: its bytes are the last line's, and bytes past the chunk add nothing"""
    recs = RF.draw_reads(random.Random(8), 30, Q, lengths=(1, 200))
    for level in (Q, Q - 1):  # the last record at the threshold, and one step below it
        last = (b"last", b"ACGT" * 30, bytes([33 + Q]) * 119 + bytes([33 + level]), None)
        raw = RF.fastq_of(recs + [last], last_eol=False)
        assert raw[-1:] != b"\n" and RF.reason(last, K, Q=Q) == (None if level == Q else RF.MEAN_QUAL)
        check_parse(pol, recs + [last], raw)


def test_a_fasta_chunk_has_the_length_rule_alone(pol):
    raw = PC.well_formed()["fasta_wrapped_60"]
    res, text, grew = device_parse(pol, raw, 12, 100, 60)
    mres, mtext, mst = RF.parse_model_f(pol._lib, raw, 12, 0, 100, 60)
    assert res.clean == 1 and text == mtext == PC.model(pol._lib, raw, 100)[1] and grew == mst and grew["dropped_mean_qual"] == 0


def test_with_min_qual_the_mean_is_over_the_stored_qualities(pol, ten_thousand):
    recs = ten_thousand[:2000]
    raw = RF.fastq_of(recs)
    res, text, grew = device_parse(pol, raw, K, 0, Q, q=Q + 2)
    want = RF.text_of(recs, K, q=Q + 2, Q=Q)
    assert res.clean == 1 and text == want and b"N" in want and RF.same_counts(grew, RF.counts(recs, K, Q=Q))
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert pol._lib.ntedit_hip_reads_min_qual_info(pol._h, a, b) == 0  # (--min_qual's counts cover the reads that were copied)


def test_an_unclean_chunk_is_reported_as_without_the_options(pol):
    """a quality line one byte short, and a chunk whose lines are no multiple of 4: unclean as without the options (the
    sums have run by then, indexed by line and bounded), nothing counted, and the next chunk parses as ever"""
    tail = RF.fastq_of(RF.draw_reads(random.Random(1), 50, Q))
    for raw, bit in ((PC.odd()["fastq_quality_one_short"] + tail, "fq_qual"), (tail + b"@cut\nACGT\n+\n", "fq_lines")):
        off, _, _ = device_parse(pol, raw, 12)
        on, text, grew = device_parse(pol, raw, 12, 30, Q)
        assert off.clean == on.clean == 0 and off.broken == on.broken and on.broken & _lib.PARSE_BAD[bit] and text is None
        assert not any(grew.values())
    recs = RF.draw_reads(random.Random(9), 40, Q)
    check_parse(pol, recs, RF.fastq_of(recs))


# ---------------------------------------------------------------------------------- 2. k_bam_facts
def device_bam(pol, raw, segment, width, min_len=K, L=0, Qm=0, Rm=0.0, q=0):
    import torch
    lib, h = pol._lib, pol._h
    assert lib.ntedit_hip_reads_bam_set_segment(h, segment) == 0 and lib.ntedit_hip_reads_bam_set_group_width(h, width) == 0
    assert lib.ntedit_hip_reads_set_read_filter(h, L, Qm, Rm) == 0 and lib.ntedit_hip_reads_set_min_qual(h, q) == 0
    cap = len(raw)
    out = torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsBamResult()
    before = stats(pol)
    torch.cuda.synchronize()
    rc = lib.ntedit_hip_reads_bam_device(h, raw, len(raw), 0, 1, min_len, out.data_ptr() + GUARD, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(h)
    torch.cuda.synchronize()
    host = bytes(out.cpu().numpy())
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + cap:] == b"\xEE" * GUARD
    return BAM.result_dict(res), host[GUARD:GUARD + res.text_len], grown(before, stats(pol))


def bam_sets():
    """150-base reads; short reads of odd and even lengths; a 60 kb record beside 50-byte ones; in each a record with 0xFF
    qualities, a skipped secondary record, records without the tag, an rq behind every aux type, and a malformed aux"""
    rng = random.Random(21)
    sets = {}
    for name, lengths, n in (("reads_150", (150, 150), 150), ("short_odd_and_even", (1, 61), 300), ("long_beside_short", (10, 70), 120)):
        recs = RF.draw_reads(rng, n, Q, R=R, with_rq=True, lengths=lengths)
        seq = bytes(rng.choice(b"ACGT") for _ in range(lengths[1] | 1))
        recs.insert(1, (b"absent", seq, RF.NO_QUAL, 0.999))
        recs.insert(4, (b"secondary", seq, bytes([34]) * len(seq), 0.1))
        recs.insert(6, (b"all_aux_low", seq, bytes([33 + Q + 5]) * len(seq), BAM.all_aux() + b"rqf" + struct.pack("<f", 0.5)))
        recs.insert(8, (b"all_aux_high", seq, bytes([33 + Q + 5]) * len(seq), BAM.all_aux() + b"rqf" + struct.pack("<f", 0.999)))
        recs.insert(9, (b"malformed", seq, bytes([33 + Q + 5]) * len(seq), b"XZZno nul" + b"rqf" + struct.pack("<f", 0.5)))
        if name == "long_beside_short":
            for i, level in ((20, Q), (70, Q - 1)):  # a 60 kb record at the threshold, and one a step below it
                long_seq = bytes(rng.choice(b"ACGT") for _ in range(60_001))
                recs.insert(i, (b"long%d" % level, long_seq, bytes([33 + Q]) * 60_000 + bytes([33 + level]), 0.995))
        sets[name] = recs
    return sets


def bam_twin(recs, min_len, **f):
    """what the twin makes of the set: the raw-aux records by what their walk finds"""
    found = {b"all_aux_low": RF.f32(0.5), b"all_aux_high": RF.f32(0.999), b"malformed": None}
    primary = [r for r in recs if r[0] != b"secondary"]
    why = [RF.reason(r, min_len, found=found.get(r[0]), **f) for r in primary]
    c = dict(records=len(primary), dropped_length=why.count(RF.LENGTH), dropped_rq=why.count(RF.RQ),
             dropped_mean_qual=why.count(RF.MEAN_QUAL))
    return b"".join(r[1] + b"\n" for r, w in zip(primary, why) if w is None), c


@pytest.mark.parametrize("width", [8, 16, 64])
@pytest.mark.parametrize("segment", [64, 256, 4096])
@pytest.mark.parametrize("name", list(bam_sets()))
def test_the_bam_facts_equal_the_model(pol, name, segment, width):
    lib = pol._lib
    recs = bam_sets()[name]
    flags = [0x100 if r[0] == b"secondary" else 0 for r in recs]
    _, raw = RF.bam_of(recs, flags)
    min_len = 1 if name == "short_odd_and_even" else K
    assert any(len(r[1]) % 2 for r in recs)
    for f in (dict(L=0, Q=Q, R=R), dict(L=30, Q=Q, R=0.0), dict(L=0, Q=0, R=R)):
        twin_text, c = bam_twin(recs, min_len, **f)
        dropped = c[RF.LENGTH] + c[RF.RQ] + c[RF.MEAN_QUAL]
        assert 0.1 * c["records"] <= dropped <= 0.9 * c["records"], c
        assert (not f["Q"] or c[RF.MEAN_QUAL]) and (not f["R"] or c[RF.RQ]) and (not f["L"] or name == "reads_150" or c[RF.LENGTH])
        want, want_text, wst = RF.bam_model_f(lib, raw, min_len, 0, f["L"], f["Q"], f["R"])
        got, text, grew = device_bam(pol, raw, segment, width, min_len, f["L"], f["Q"], f["R"])
        assert got == BAM.result_dict(want) and text == want_text == twin_text, (name, f)
        assert grew == wst and RF.same_counts(grew, c), (grew, wst, c)
        assert grew["aux_malformed"] == (1 if f["R"] else 0) and got["skipped_flag"] == 1
        assert lib.ntedit_hip_reads_bam_group_width(pol._h) == width
    got, text, grew = device_bam(pol, raw, segment, width, min_len)
    assert text == BAM.model(lib, raw, 1, min_len)[2] and not any(grew.values())


def test_the_group_width_follows_the_mean_read_length(pol):
    lib, h = pol._lib, pol._h
    sets = bam_sets()
    rng = random.Random(3)
    long_reads = RF.draw_reads(rng, 6, Q, R=R, with_rq=True, lengths=(15_000, 20_000))
    for recs, want in ((sets["reads_150"], 8), (long_reads, 64), (RF.draw_reads(rng, 40, Q, lengths=(500, 900)), 16)):
        raw = RF.bam_of(recs, [0x100 if r[0] == b"secondary" else 0 for r in recs])[1]
        for _ in range(2):  # the second chunk goes by the mean length of the reads the first one kept
            got, text, grew = device_bam(pol, raw, 0, 0, K, 0, 1, 0.0)
        assert lib.ntedit_hip_reads_bam_group_width(h) == want
        assert text == RF.bam_model_f(lib, raw, K, 0, 0, 1, 0.0)[1]
    assert lib.ntedit_hip_reads_bam_set_group_width(h, 32) == _lib.E_ARG


def test_with_min_qual_the_bam_mean_is_over_the_stored_qualities(pol):
    recs = [r for r in bam_sets()["reads_150"] if not isinstance(r[3], bytes) and r[0] != b"secondary"]
    _, raw = RF.bam_of(recs)
    got, text, grew = device_bam(pol, raw, 4096, 16, K, 0, Q, R, q=Q + 2)
    want = RF.text_of(recs, K, q=Q + 2, Q=Q, R=R)
    assert text == want and b"N" in want and RF.same_counts(grew, RF.counts(recs, K, Q=Q, R=R))


# ---------------------------------------------------------------------------------- 3. the front ends, by the twin
def run(args, timeout=900):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def lines_of(r):
    return [tuple(int(x) for x in m) for m in FILTER_LINE.findall(r.stderr)]


def line_of(c):
    return (c[RF.LENGTH] + c[RF.RQ] + c[RF.MEAN_QUAL], c["records"], c[RF.LENGTH], c[RF.RQ], c[RF.MEAN_QUAL])


FLAGS = ["--min_read_len", 120, "--min_mean_qual", Q]
F = dict(L=120, Q=Q)


@pytest.fixture(scope="module")
def read_set(tmp_path_factory):
    """reads of 100..150 bases at 40x with per-read quality levels around Q and rq around R (drawn as RF.draw_read draws
    them, with numpy); the file, its twin (the kept reads), the same set as BAM with its own twin (rq applies there), and
    what the pass has to report"""
    d = tmp_path_factory.mktemp("read_filter")
    rng = np.random.default_rng(77)
    truth = H.random_genome(rng, 66_000)
    reads = simulate_reads(rng, truth, 40)
    count, width = reads.shape
    lengths = rng.choice(np.array([100, 119, 120, 150, 150, 150, 150, 150]), count)
    level = Q + rng.choice(np.array([-12, -3, -2, -1, 0, 0, 1, 2, 3, 15]), count)
    qual = (33 + np.clip(level[:, None] + rng.choice(np.array([-4, -1, 0, 0, 0, 1, 6]), reads.shape), 0, 93)).astype(np.uint8)
    rq = np.where(rng.random(count) < 0.1, np.float32(R), np.clip(R + rng.uniform(-0.02, 0.01, count), 0, 1).astype(np.float32))
    tagged = rng.random(count) < 0.85
    recs = [(b"r%d" % i, bytes(reads[i, :lengths[i]]), bytes(qual[i, :lengths[i]]), float(rq[i]) if tagged[i] else None)
            for i in range(count)]
    why_text, why_bam = [RF.reason(r, K, **F) for r in recs], [RF.reason(r, K, R=R, **F) for r in recs]
    c_text = RF.assert_discriminating(recs, K, [RF.LENGTH, RF.MEAN_QUAL], **F)
    c_bam = RF.assert_discriminating(recs, K, [RF.LENGTH, RF.RQ, RF.MEAN_QUAL], R=R, **F)
    kept_bam = [r for r, w in zip(recs, why_bam) if w is None]
    (d / "r.fq").write_bytes(RF.fastq_of(recs))
    (d / "twin.fq").write_bytes(RF.fastq_of([r for r, w in zip(recs, why_text) if w is None]))
    (d / "r.bam").write_bytes(RF.bam_of(recs)[0])
    (d / "bam_twin.fq").write_bytes(RF.fastq_of(kept_bam))
    (d / "all_twin.fq").write_bytes(MQ.fastq(MQ.mask_records(RF.three(kept_bam), Q + 2)))
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:40000]), (b"ctg2", draft[40000:])], width=80)
    return dict(dir=d, fq=d / "r.fq", twin=d / "twin.fq", bam=d / "r.bam", bam_twin=d / "bam_twin.fq", all_twin=d / "all_twin.fq",
                draft=d / "draft.fa", line=line_of(c_text), bam_line=line_of(c_bam))


BUILD = ["-k", K, "-c", 2, "--bf", 2_000_000]


def three_ways(read_set, tag, args, outputs=("",), k_args=BUILD):
    """the tool with the options on the file, host parser and --gpu_parse, and without them on the twin: every output equal"""
    d = read_set["dir"]
    runs = {}
    for name, src, flags in (("host", read_set["fq"], FLAGS), ("gpu", read_set["fq"], FLAGS + ["--gpu_parse"]), ("twin", read_set["twin"], [])):
        out = d / ("%s_%s.bf" % (tag, name))
        a = [str(x).replace("{out}", str(out)) for x in args]
        runs[name] = (run([TOOL, "--reads", src, "-o", out] + k_args + a + flags), out)
    for suffix in outputs:
        twin = open(str(runs["twin"][1]) + suffix, "rb").read()
        assert open(str(runs["host"][1]) + suffix, "rb").read() == twin, (tag, suffix, "host parser")
        assert open(str(runs["gpu"][1]) + suffix, "rb").read() == twin, (tag, suffix, "--gpu_parse")
    assert not lines_of(runs["twin"][0]) and "--min_mean_qual" not in runs["twin"][0].stdout
    for name in ("host", "gpu"):
        lines = lines_of(runs[name][0])
        assert lines and all(l == read_set["line"] for l in lines), (name, lines, read_set["line"])
        assert "--min_mean_qual %d" % Q in runs[name][0].stdout and "--min_read_len 120" in runs[name][0].stdout
    assert "unclean" not in runs["gpu"][0].stderr
    return runs


def test_the_filter_equals_the_twins(read_set):
    runs = three_ways(read_set, "cut", [])
    assert len(lines_of(runs["gpu"][0])) == 2  # (pass 1 and pass 2 both read the file)
    plain = read_set["dir"] / "plain.bf"  # the options matter: a k-mer of the whole set's filter is absent from the filtered one
    run([TOOL, "--reads", read_set["fq"], "-o", plain] + BUILD)
    a = np.frombuffer(plain.read_bytes(), dtype=np.uint8)
    b = np.frombuffer(runs["twin"][1].read_bytes(), dtype=np.uint8)
    assert a.size == b.size and int(np.bitwise_and(a, np.bitwise_not(b)).any())


def test_solid_and_hist_equal_the_twins(read_set):
    runs = three_ways(read_set, "solid", ["--solid", "--hist", "{out}.hist"], outputs=("", ".hist"), k_args=["-k", K, "--bf", 2_000_000])
    cut = {name: re.search(r"--solid: minimum k-mer count (\d+)", r.stderr).group(1) for name, (r, _) in runs.items()}
    assert len(set(cut.values())) == 1, cut


def test_the_reject_filter_equals_the_twins(read_set):
    three_ways(read_set, "reject", ["--reject_cutoff", 20, "--reject_bf", 500_000, "--reject_out", "{out}.reject"], outputs=("", ".reject"))


def test_the_bam_with_min_rq_equals_its_twin(read_set):
    d = read_set["dir"]
    run([TOOL, "--reads", read_set["bam_twin"], "-o", d / "bam_twin.bf"] + BUILD)
    r = run([TOOL, "--reads", read_set["bam"], "-o", d / "bam.bf", "--gpu_parse", "--min_rq", R] + FLAGS + BUILD)
    assert (d / "bam.bf").read_bytes() == (d / "bam_twin.bf").read_bytes()
    assert lines_of(r) == [read_set["bam_line"]] * 2 and "no record had an rq tag" not in r.stderr and "unclean" not in r.stderr
    # --min_rq on reads without the tag passes every record, and the pass line says that none had it
    run([TOOL, "--reads", read_set["twin"], "-o", d / "norq_twin.bf"] + BUILD)
    r = run([TOOL, "--reads", read_set["fq"], "-o", d / "norq.bf", "--min_rq", R] + FLAGS + BUILD)
    assert (d / "norq.bf").read_bytes() == (d / "norq_twin.bf").read_bytes()
    assert lines_of(r) == [read_set["line"]] * 2 and r.stderr.count("--min_rq: no record had an rq tag") == 2


def test_all_three_options_together_with_min_qual(read_set):
    """the twin: the kept reads (judged by their stored qualities) with the bases below --min_qual rewritten to N"""
    d = read_set["dir"]
    run([TOOL, "--reads", read_set["all_twin"], "-o", d / "all_twin.bf"] + BUILD)
    r = run([TOOL, "--reads", read_set["bam"], "-o", d / "all.bf", "--gpu_parse", "--min_rq", R, "--min_qual", Q + 2] + FLAGS + BUILD)
    assert (d / "all.bf").read_bytes() == (d / "all_twin.bf").read_bytes()
    assert lines_of(r) == [read_set["bam_line"]] * 2


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_ntedit_reads_equals_ntedit_with_the_twins_filter(read_set):
    d = read_set["dir"]
    twin_bf = d / "polish_twin.bf"
    run([TOOL, "--reads", read_set["twin"], "-o", twin_bf] + BUILD)
    run([NTEDIT, "-f", read_set["draft"], "-r", twin_bf, "-b", d / "by_filter"])
    for tag, flags in (("host", []), ("gpu", ["--gpu_parse"])):
        r = run([NTEDIT, "-f", read_set["draft"], "--reads", read_set["fq"], "-k", K, "--cutoff", 2, "--bf", 2_000_000,
                 "--save_bf", d / ("n_%s.bf" % tag), "-b", d / ("n_" + tag)] + FLAGS + flags)
        assert read(d / ("n_%s.bf" % tag)) == read(twin_bf)
        for suffix in ("_edited.fa", "_changes.tsv"):
            assert read(str(d / ("n_" + tag)) + suffix) == read(str(d / "by_filter") + suffix), (tag, suffix)
        assert lines_of(r) == [read_set["line"]]  # (pass 2 reads the store, which holds the reads that passed)


def test_the_cascade_filters_alike_in_every_round(read_set):
    """-k 40,25: both rounds equal the rounds run from the twin; the store is resident, the inputs parsed once"""
    d = read_set["dir"]
    common = ["-f", read_set["draft"], "-k", "40,25", "--cutoff", 2, "--bf", 2_000_000]
    run([NTEDIT] + common + ["--reads", read_set["twin"], "-b", d / "casc_twin"])
    r = run([NTEDIT] + common + ["--reads", read_set["fq"], "--gpu_parse", "-b", d / "casc"] + FLAGS)
    for suffix in ("_k40_edited.fa", "_k40_changes.tsv", "_edited.fa", "_changes.tsv"):
        assert read(str(d / "casc") + suffix) == read(str(d / "casc_twin") + suffix), suffix
    assert len(lines_of(r)) == 1 and "no read file was opened" in r.stdout


@pytest.fixture(scope="module")
def twin_filter(read_set):
    out = read_set["dir"] / "ranks_twin.bf"
    run([TOOL, "--reads", read_set["twin"], "-o", out] + BUILD)
    return out


@pytest.mark.parametrize("flags", [[], ["--gpu_parse"]], ids=["host_parser", "gpu_parse"])
def test_make_reads_at_world_2_filters_alike_on_every_rank(read_set, twin_filter, flags):
    """over gloo, the plain FASTQ cut into ranges: the bytes of the single-process tool on the twin; the ranks' counts sum"""
    from test_gpu_reads_multi import _driver
    out = read_set["dir"] / ("w2_%d.bf" % len(flags))
    r = _driver(2, ["--reads", str(read_set["fq"]), "-o", str(out)] + [str(x) for x in FLAGS + BUILD] + flags, "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert out.read_bytes() == twin_filter.read_bytes()
    by_rank = lines_of(r)
    assert len(by_rank) == 4 and "rank 1/2: read filter:" in r.stderr  # (two passes on each of two ranks)
    assert tuple(sum(col) for col in zip(*by_rank)) == tuple(2 * x for x in read_set["line"])


def test_run_reads_at_world_2_sums_the_ranks_counters(read_set, twin_filter):
    """python -m ntedit_amd.run --reads on two ranks over gloo: the filter and the polish of ntedit with the twin's filter,
    and the ranks' parse[pass]["read_filter"] counters sum to the twin's"""
    from test_gpu_reads_run import driver, reports
    d = read_set["dir"]
    run([NTEDIT, "-f", read_set["draft"], "-r", twin_filter, "-b", d / "w2_by_filter"])
    r = driver(2, ["-f", read_set["draft"], "--reads", read_set["fq"], "-k", K, "--cutoff", 2, "--bf", 2_000_000,
                   "--save_bf", d / "run2.bf", "-b", d / "run2", "--report"] + FLAGS, "gloo")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert read(d / "run2.bf") == read(twin_filter)
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(d / "run2") + suffix) == read(str(d / "w2_by_filter") + suffix), suffix
    got = [rep["reads"]["parse"]["1"]["read_filter"] for rep in reports(r)]
    total, records, by_len, by_rq, by_mq = read_set["line"]
    assert len(got) == 2 and all(g["records"] > 0 for g in got)
    assert tuple(sum(g[n] for g in got) for n in ("records", RF.LENGTH, RF.RQ, RF.MEAN_QUAL)) == (records, by_len, by_rq, by_mq)


def test_the_negative_zero_is_off_on_the_device(pol):
    lib, h = pol._lib, pol._h
    assert lib.ntedit_hip_reads_set_read_filter(h, 0, 0, -0.0) == 0
    a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_float(1.0)
    assert lib.ntedit_hip_reads_get_read_filter(h, a, b, c) == 0 and (a.value, b.value) == (0, 0)
    assert struct.pack("<f", c.value) == b"\0\0\0\0"
    recs = [r for r in bam_sets()["reads_150"] if r[0] != b"secondary"]
    got, text, grew = device_bam(pol, RF.bam_of(recs)[1], 4096, 0, K, 0, 0, -0.0)
    assert text == b"".join(r[1] + b"\n" for r in recs) and not any(grew.values())
    for bad in (-0.5, 1.5, float("nan")):
        assert lib.ntedit_hip_reads_set_read_filter(h, 0, 0, bad) == _lib.E_ARG


def test_run_reads_at_world_1_equals_ntedit_with_the_twins_filter(read_set, twin_filter):
    from test_gpu_reads_run import driver, reports
    d = read_set["dir"]
    run([NTEDIT, "-f", read_set["draft"], "-r", twin_filter, "-b", d / "ranks_by_filter"])
    r = driver(1, ["-f", read_set["draft"], "--reads", read_set["fq"], "-k", K, "--cutoff", 2, "--bf", 2_000_000,
                   "--save_bf", d / "run.bf", "-b", d / "run", "--report"] + FLAGS, "nccl")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-5000:]
    assert read(d / "run.bf") == read(twin_filter)
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(d / "run") + suffix) == read(str(d / "ranks_by_filter") + suffix), suffix
    got = reports(r)[0]["reads"]["parse"]["1"]["read_filter"]
    total, records, by_len, by_rq, by_mq = read_set["line"]
    assert (got["records"], got["dropped_length"], got["dropped_rq"], got["dropped_mean_qual"]) == (records, by_len, by_rq, by_mq)
    assert (got["min_read_len"], got["min_mean_qual"]) == (120, Q)
