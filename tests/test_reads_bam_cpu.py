"""--gpu_parse on BAM reads, the CPU tier: the serial host model (ntedit_hip_reads_bam_model, built from the functions of
nte_bam_grammar.h that the kernels use) against the Python restatement of tests/bam_corpus.py and against the text parser's
model on the twin FASTQ; the cut at every offset; every refusal; ntedit_hip_reads_is_bam; the front ends' refusal of a BAM
without --gpu_parse; and the header alone as a host program under AddressSanitizer and UBSan."""
import gzip
import os
import struct
import subprocess

import pytest

import bam_corpus as BAM
import helpers as H
import parse_corpus as PC
from ntedit_amd import _lib

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
HOST_SRC = os.path.join(H.ROOT, "tests", "bam", "model_host.cpp")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return BAM.corpus()


def small_case():
    """a header with one reference and five records: kept, secondary, short, odd length, kept"""
    recs = [BAM.record(b"a", 0, b"ACGTACGTACGTACGTACGTACGTACGTA", aux=BAM.all_aux()), BAM.record(b"b", 0x100, b"ACGT" * 10),
            BAM.record(b"c", 0, b"ACGT"), BAM.record(b"d", 0x10, b"N" * 31, cigar=(31 << 4,)), BAM.record(b"e", 0x4, b"ACGT" * 8)]
    return BAM.header(b"@HD\n", [(b"chr1", 1000)]), recs


def test_the_model_equals_the_restatement_on_the_corpus(lib, corpus):
    seen = set()
    for c in corpus:
        for min_len in (BAM.K, 1, 0):
            want, text = BAM.restate(c.raw, 1, min_len)
            rc, got, got_text = BAM.model(lib, c.raw, 1, min_len)
            assert rc == 0 and got == want and got_text == text, (c.name, min_len, got, want)
            assert want["clean"] == 1 and want["cut"] == len(c.raw) and want["header_len"] == c.header_len
            assert want["records"] == len(c.reads)
        seen.add(c.name)
    assert {"decoys", "header_only", "lengths_and_codes"} <= seen


def test_the_models_text_is_the_text_parsers_on_the_twin(lib, corpus):
    for c in corpus:
        _, _, text = BAM.model(lib, c.raw, 1, BAM.K)
        if not c.twin:
            assert text == b""
            continue
        res, twin_text = PC.model(lib, c.twin, BAM.K)
        assert res.clean == 1, (c.name, res.broken)
        assert text == twin_text, c.name
        # ... and the corpus itself says so: the kept reads, as written
        assert text == b"".join(s + b"\n" for _, f, s in c.reads if not f & 0x900 and len(s) >= BAM.K)


def test_the_cut_at_every_offset_of_a_small_case(lib):
    head, recs = small_case()
    raw = head + b"".join(recs)
    ends = [len(head)]
    for r in recs:
        ends.append(ends[-1] + len(r))
    for n in range(len(raw) + 1):
        rc, got, text = BAM.model(lib, raw[:n], 1, BAM.K)
        want, want_text = BAM.restate(raw[:n], 1, BAM.K)
        assert rc == 0 and got == want and text == want_text, n
        # the last record end at or before n; 0 while the header does not fit
        assert got["clean"] == 1 and got["cut"] == (max(e for e in ends if e <= n) if n >= len(head) else 0), n
    # a carried chunk: no header, a record start at byte 0, ended everywhere (inside block_size, the fixed fields, seq)
    body = raw[len(head):]
    for n in range(len(body) + 1):
        rc, got, text = BAM.model(lib, body[:n], 0, BAM.K)
        assert rc == 0 and (got, text) == BAM.restate(body[:n], 0, BAM.K)
        assert got["cut"] == max(e - len(head) for e in ends if e - len(head) <= n) and got["header_len"] == 0


def damaged_inputs():
    head, recs = small_case()
    raw = head + b"".join(recs)
    at = len(head) + len(recs[0])  # the second record
    put = lambda off, fmt, v: raw[:at + off] + struct.pack(fmt, v) + raw[at + off + struct.calcsize(fmt):]
    return {
        "magic": (b"BAM\2" + raw[4:], _lib.BAM_BAD_MAGIC, 0),
        "magic_in_two_bytes": (b"BX", _lib.BAM_BAD_MAGIC, 0),
        "negative_l_text": (raw[:4] + struct.pack("<i", -1) + raw[8:], _lib.BAM_BAD_HEADER, 0),
        "negative_n_ref": (BAM.header(b"@HD\n")[:-4] + struct.pack("<i", -5), _lib.BAM_BAD_HEADER, 0),
        "empty_reference_name": (b"BAM\1" + struct.pack("<iii", 0, 1, 0) + b"\0" * 8, _lib.BAM_BAD_HEADER, 0),
        "negative_block_size": (put(0, "<i", -8), _lib.BAM_BAD_SIZE, at),
        "block_size_2_30": (put(0, "<i", 1 << 30), _lib.BAM_BAD_SIZE, at),
        "block_size_below_the_fixed_bytes": (put(0, "<i", 31), _lib.BAM_BAD_RECORD, at),
        "empty_read_name": (put(12, "<B", 0), _lib.BAM_BAD_RECORD, at),
        "l_seq_past_the_block": (put(20, "<I", 4000), _lib.BAM_BAD_RECORD, at),
        "l_seq_2_32": (put(20, "<I", 0xFFFFFFFF), _lib.BAM_BAD_RECORD, at),
        "cigar_past_the_block": (put(16, "<H", 65535), _lib.BAM_BAD_RECORD, at),
    }


def test_every_refusal_is_raised_by_its_input(lib):
    seen = 0
    for name, (raw, bit, at) in damaged_inputs().items():
        rc, got, _ = BAM.model(lib, raw, 1, BAM.K)
        want, _ = BAM.restate(raw, 1, BAM.K)
        assert rc == 0 and got == want, name
        assert got["clean"] == 0 and got["broken"] == bit and got["cut"] == at, (name, got)
        seen |= bit
    assert seen == _lib.BAM_BAD_MAGIC | _lib.BAM_BAD_HEADER | _lib.BAM_BAD_RECORD | _lib.BAM_BAD_SIZE
    # an unclean record is unclean as soon as its fixed bytes are inside, whatever is cut behind them
    raw, bit, at = damaged_inputs()["empty_read_name"]
    assert BAM.model(lib, raw[:at + 36], 1, BAM.K)[1]["broken"] == bit
    assert BAM.model(lib, raw[:at + 35], 1, BAM.K)[1] == dict(BAM.restate(raw[:at + 35])[0], clean=1, cut=at)


def test_the_model_reports_a_text_that_does_not_fit(lib):
    head, recs = small_case()
    raw = head + b"".join(recs)
    res = _lib.ReadsBamResult()
    assert lib.ntedit_hip_reads_bam_model(raw, len(raw), 1, BAM.K, None, 0, res) == _lib.E_OVERFLOW
    assert res.text_len == BAM.restate(raw)[0]["text_len"]


def test_is_bam(lib, corpus, tmp_path):
    fq = corpus[0].twin
    files = {"x.bam": corpus[0].bam, "no_eof.bam": [c for c in corpus if c.name == "no_eof_member"][0].bam,
             "one_byte_members.bam": BAM.bgzf(corpus[0].raw[:3000], sizes=(4, 1, 1, 300)),
             "bgzf.fq.gz": BAM.bgzf(fq), "plain.fq.gz": gzip.compress(fq), "plain.fq": fq, "magic.txt": b"BAM\1 but not compressed",
             "empty": b"", "cut_member.bam": corpus[0].bam[:100],
             # a first member of fewer than four bytes, or of none, is legal BGZF: further members are inflated
             "three_byte_member.bam": BAM.bgzf(corpus[0].raw[:3000], sizes=(3, 300)),
             "members_of_1_1_1_1.bam": BAM.bgzf(corpus[0].raw[:3000], sizes=(1, 1, 1, 1, 300)),
             "empty_first_member.bam": BAM.EOF_MEMBER + BAM.bgzf(corpus[0].raw[:3000], sizes=(2, 300)),
             "three_bytes_and_no_more": BAM.bgzf(corpus[0].raw[:3], eof=False),
             "second_member_differs": BAM.bgzf(b"BAMX" + corpus[0].raw[4:3000], sizes=(3, 300))}
    is_a_bam = ("x.bam", "no_eof.bam", "one_byte_members.bam", "three_byte_member.bam", "members_of_1_1_1_1.bam",
                "empty_first_member.bam")
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        want = name in is_a_bam
        assert lib.ntedit_hip_reads_is_bam(str(tmp_path / name).encode()) == int(want), name
        assert lib.ntedit_hip_reads_is_gzip(str(tmp_path / name).encode()) == int(data[:2] == b"\x1f\x8b")
    assert lib.ntedit_hip_reads_is_bam(str(tmp_path / "missing").encode()) == 0


def run(args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_a_bam_without_gpu_parse_is_refused_before_anything_is_written(corpus, tmp_path):
    """the shared reads rules refuse it: no device is touched and no file written (before, the host parser read whatever
    '@' and '>' bytes the stream held, and the run ended with exit status 0)"""
    bam = tmp_path / "x.bam"
    bam.write_bytes(corpus[1].bam)
    fq = tmp_path / "ok.fq"
    fq.write_bytes(corpus[1].twin)
    line = "--reads %s: BAM needs --gpu_parse" % bam
    out = tmp_path / "out.bf"
    r = run([TOOL, "--reads", fq, bam, "-k", BAM.K, "-c", 2, "--bf", 100000, "-o", out, "--hist", tmp_path / "h.hist"])
    assert r.returncode != 0 and line in r.stderr.splitlines(), r.stderr[-3000:]
    draft = tmp_path / "draft.fa"
    draft.write_bytes(b">ctg\n" + b"ACGT" * 200 + b"\n")
    r = run([NTEDIT, "-f", draft, "--reads", bam, "-k", BAM.K, "--cutoff", 2, "--bf", 100000, "-b", tmp_path / "pol"])
    assert r.returncode != 0 and line in (r.stderr + r.stdout), (r.stdout + r.stderr)[-3000:]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["draft.fa", "ok.fq", "x.bam"]


# ---------------------------------------------------------------------------------- the header alone, as a host program
def build_host(out_dir, sanitize):
    exe = os.path.join(str(out_dir), "bam_model_host_san" if sanitize else "bam_model_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(H.ROOT, "ntedit_amd", "csrc"), "-o", exe,
                                                                         HOST_SRC], check=True)
    return exe


def host_cases(corpus):
    """[(kind, at_header, min_len, bytes)]: the corpus, the small case ended at every offset, the refusals, files' starts"""
    cases = [(0, 1, BAM.K, c.raw) for c in corpus] + [(0, 1, 0, c.raw) for c in corpus[:3]]
    head, recs = small_case()
    raw = head + b"".join(recs)
    cases += [(0, 1, BAM.K, raw[:n]) for n in range(len(raw) + 1)]
    cases += [(0, 0, 1, raw[len(head):][:n]) for n in range(len(raw) - len(head) + 1)]
    for c in corpus[:4]:  # the records' starts ended everywhere around a member's end
        cases += [(0, 1, BAM.K, c.raw[:n]) for n in range(c.header_len - 3, min(len(c.raw), c.header_len + 400))]
    cases += [(0, 1, BAM.K, d) for d, _, _ in damaged_inputs().values()]
    first = corpus[0].bam
    cases += [(1, 0, 0, first[:n]) for n in list(range(0, 64)) + [100, 1000, len(first)]]
    cases += [(1, 0, 0, c.bam) for c in corpus[:3]] + [(1, 0, 0, BAM.bgzf(corpus[0].twin)), (1, 0, 0, gzip.compress(corpus[0].twin))]
    tiny = BAM.EOF_MEMBER + BAM.bgzf(corpus[0].raw[:600], sizes=(1, 2, 1, 300))  # the magic over four members, one of them empty
    cases += [(1, 0, 0, tiny[:n]) for n in range(len(tiny) + 1)]
    return cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "address_undefined"])
def test_the_host_program(lib, corpus, tmp_path, sanitize):
    """tests/bam/model_host.cpp: nte_bam_grammar.h alone.  Under the sanitizers every input is a heap block of its exact
    size, so a hop that read a length before checking it against the bytes at hand would be reported."""
    cases = host_cases(corpus)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for kind, at_header, min_len, data in cases:
            f.write(struct.pack("<IIIQ", kind, at_header, min_len, len(data)) + data)
    r = subprocess.run([build_host(tmp_path, sanitize), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (kind, at_header, min_len, data), line in zip(cases, lines):
        if kind == 1:
            want = data[:4] == b"\x1f\x8b\x08\x04" and BAM.restate_first_member(data) == b"BAM\1"
            assert int(line) == int(want)
            continue
        want, text = BAM.restate(data, at_header, min_len)
        fold = 0
        for b in text:
            fold = (fold * 31 + b) & 0xFFFFFFFF
        assert [int(x) for x in line.split()] == [want[f] for f in BAM.FIELDS] + [fold], (len(data), at_header)
