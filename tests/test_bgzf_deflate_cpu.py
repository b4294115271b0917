"""The BGZF writer, the CPU tier: the encoder of nte_bgzf_deflate.h as the serial host model runs it
(ntedit_hip_bgzf_deflate_model) against Python's gzip and zlib and against the project's own decoder, on the corpus of
tests/deflate_corpus.py; the small calls around it; the size condition; and the stand-alone host program, plain and
under sanitizers.  The device runs the same functions (tests/test_gpu_bgzf_deflate.py)."""
import ctypes
import os
import re
import subprocess
import zlib

import pytest

import bgzf_corpus as BC
import deflate_corpus as DC
import helpers as H
from ntedit_amd import _lib

E_OVERFLOW = -4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def members():
    return DC.model_of_corpus()


def test_the_corpus_covers_what_it_should():
    sizes = {len(d) for _, d in DC.corpus()}
    assert set(range(1, 301)) <= sizes
    assert {DC.BLOCK - 1, DC.BLOCK, DC.BLOCK + 1, 2 * DC.BLOCK, 2 * DC.BLOCK + 1, 46366} <= sizes
    by_name = dict(DC.corpus())
    assert len(set(by_name["one_value"])) == 1 and len(by_name["one_value"]) == DC.BLOCK
    assert all(by_name["uniform_256x255"].count(bytes([v])) == 255 for v in range(256))
    assert len(set(by_name["fibonacci_21"])) == 21
    assert by_name["fasta_header_1"].startswith(b">h\n") and by_name["fasta_header_300"].startswith(b">" + b"h" * 300 + b"\n")
    assert len(by_name["demo_draft"]) == 4641752


def test_gzip_gives_the_plain_bytes_back(members):
    for name, data in DC.corpus():
        assert DC.gunzip(members[name]) == data, name


def test_every_member_walks_as_bgzf(members):
    """magic, FLG, XLEN, 'BC', BSIZE; CRC-32 and ISIZE against zlib.crc32 of the member's slice; a member is at most
    64 KiB; the stored fallback where it must be taken, and nowhere in DNA blocks of any size that pays"""
    stored = {}
    for name, data in DC.corpus():
        stored[name] = DC.check_members(members[name], data)
        assert all(len(m) <= 65536 for m, _, _, _ in DC.walk(members[name])), name
    for name in DC.STORED:
        assert stored[name] == 1 and len(members[name]) == 18 + 5 + DC.BLOCK + 8 == 65311, name
    assert stored["one_value"] == 0 and len(members["one_value"]) < 8300  # (a bit a byte: the two-symbol code)
    assert stored["fibonacci_21"] == 0 and stored["demo_draft"] == 0 and stored["fasta_39_blocks"] == 0
    assert stored["acgt_%d" % DC.BLOCK] == 0 and stored["acgt_300"] == 0
    assert stored["acgt_1"] == 1  # (no code beats five bytes on one byte)


def _code_lengths(payload):
    """the literal/length code lengths a dynamic block's header declares (zlib has accepted the block already)"""
    bits = int.from_bytes(payload[:600], "little")
    pos = 3

    def take(n):
        nonlocal pos
        v = (bits >> pos) & ((1 << n) - 1)
        pos += n
        return v
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = take(3)
    # canonical code of the code-length alphabet, decoded bit by bit
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in codes:
            c = c << 1 | take(1)
            n += 1
            assert n <= 7
        s = codes[(n, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:], cl


def test_the_length_limiter_makes_a_complete_code_of_15_bits(members):
    """21 byte values with Fibonacci counts and the end-of-block symbol: the unrestricted code is 21 deep"""
    (_, payload, _, _), = DC.walk(members["fibonacci_21"])
    lit, dist, cl = _code_lengths(payload)
    used = [n for n in lit if n]
    assert len(used) == 22 and max(used) == 15
    assert sum(2 ** (15 - n) for n in used) == 2 ** 15  # Kraft: exactly 1
    assert dist == [0]  # HDIST: one code of length 0
    assert sum(2 ** (7 - n) for n in cl if n) == 2 ** 7
    # ... and the two-symbol code of a block of one byte value
    (_, payload, _, _), = DC.walk(members["one_value"])
    lit, dist, _ = _code_lengths(payload)
    assert [n for n in lit if n] == [1, 1] and lit[ord("G")] == 1 and lit[256] == 1 and dist == [0]


def test_our_own_decoder_reads_the_members(lib, members):
    for name, data in DC.corpus():
        ms = [m for m, _, _, _ in DC.walk(members[name])]
        blob, table, n_out = BC.table_of(ms)
        status, out = BC.model(lib, blob, table, n_out)
        assert status == [0] * len(ms), name
        assert out == data, name
    # ... and the walker of the library finds them, with the EOF member behind
    rc, found, used = BC.walk(lib, members["fasta_39_blocks"] + DC.EOF_MEMBER)
    assert rc == _lib.BGZF_END and len(found) == 40 and used == len(members["fasta_39_blocks"]) + 28
    assert [m.n_out for m in found[:-1]] == [len(b) for b in DC.blocks(dict(DC.corpus())["fasta_39_blocks"])]


def test_bound_cap_empty_and_eof(lib):
    assert lib.ntedit_hip_bgzf_bound(0) == 0
    assert lib.ntedit_hip_bgzf_bound(1) == 32 and lib.ntedit_hip_bgzf_bound(DC.BLOCK) == 65311
    assert lib.ntedit_hip_bgzf_bound(DC.BLOCK + 1) == 65311 + 32
    n = ctypes.c_uint64(77)
    assert lib.ntedit_hip_bgzf_deflate_model(None, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert DC.model(lib, b"") == b""
    # a buffer too small: the bytes needed, nothing written behind the cap
    data = dict(DC.corpus())["acgt_%d" % (2 * DC.BLOCK + 1)]
    whole = DC.model_of_corpus()["acgt_%d" % (2 * DC.BLOCK + 1)]
    for cap in (0, 10, len(whole) - 1):
        out = ctypes.create_string_buffer(b"\xEE" * (cap + 64), cap + 64)
        assert lib.ntedit_hip_bgzf_deflate_model(data, len(data), out, cap, ctypes.byref(n)) == E_OVERFLOW
        assert n.value == len(whole) and out.raw[cap:] == b"\xEE" * 64
    assert DC.model(lib, data, cap=len(whole)) == whole
    # the random block needs exactly the bound
    assert len(DC.model_of_corpus()["random_65280"]) == lib.ntedit_hip_bgzf_bound(DC.BLOCK)
    k = ctypes.c_uint32()
    p = lib.ntedit_hip_bgzf_eof(ctypes.byref(k))
    assert k.value == 28 and ctypes.string_at(p, 28) == DC.EOF_MEMBER == BC.EOF_MEMBER
    assert DC.gunzip(DC.EOF_MEMBER) == b"" and lib.ntedit_hip_bgzf_eof(None) == p


def test_the_stats_struct_matches_the_header():
    text = open(os.path.join(H.ROOT, "include", "ntedit_hip.h")).read()
    body = re.search(r"typedef struct ntedit_hip_bgzf_stats\s*\{(.*?)\}\s*ntedit_hip_bgzf_stats;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    assert [(n, want[t]) for n, t in fields] == list(_lib.BgzfStats._fields_)
    assert [n for n, _ in fields] == ["ms_image", "ms_deflate", "ms_copy", "plain_bytes", "bgzf_bytes", "members", "stored_members"]
    assert ctypes.sizeof(_lib.BgzfStats) == 40
    assert [getattr(_lib.BgzfStats, n).offset for n, _ in fields] == [0, 4, 8, 16, 24, 32, 36]
    assert "#define NTEDIT_HIP_APPLY_BGZF 8u" in text and _lib.APPLY_BGZF == 8
    # (the older structs did not grow)
    assert ctypes.sizeof(_lib.ApplyStats) == 40 and ctypes.sizeof(_lib.QvRow) == 48


def _level6(data):
    total = 0
    for blk in DC.blocks(data):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        total += len(c.compress(blk) + c.flush())
    return total


def test_no_larger_than_zlib_level_6_on_dna(members):
    """a cap, not a measurement: on DNA the literal-only dynamic blocks take no more bytes than zlib's level 6 takes
    for the same 65,280-byte blocks (zlib's Z_HUFFMAN_ONLY stays inside level 6 by 4.6 % on the draft and 5.4 % on
    i.i.d. ACGT)"""
    import random
    draft = dict(DC.corpus())["demo_draft"]
    ours = sum(len(p) for _, p, _, _ in DC.walk(members["demo_draft"]))
    assert ours <= _level6(draft)
    iid = DC.acgt(random.Random(5), 1_000_000)
    ours = sum(len(p) for _, p, _, _ in DC.walk(DC.model(_lib.load(), iid)))
    assert ours <= _level6(iid)


# ------------------------------------------------------------------------------------------- the stand-alone program
def _run_host(exe, tmp_path):
    cases, out = str(tmp_path / "cases.bin"), str(tmp_path / "members.bin")
    DC.write_cases(cases, DC.corpus())
    r = subprocess.run([exe, cases, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    m = re.search(r"^cases (\d+) members (\d+) stored (\d+) bytes (\d+) mismatches 0\s*$", r.stdout.strip().splitlines()[-1])
    assert m, r.stdout[-400:]
    want = b"".join(DC.model_of_corpus()[name] for name, _ in DC.corpus())
    assert int(m.group(1)) == len(DC.corpus()) and int(m.group(4)) == len(want)
    assert int(m.group(2)) == sum(len(DC.blocks(d)) for _, d in DC.corpus())
    assert open(out, "rb").read() == want  # (the header compiled on its own writes what the library's model writes)


def test_the_host_program(tmp_path):
    """tests/bgzf/deflate_host.cpp: the header alone, one lane; every member through zlib's inflate and through
    nte_bgzf_inflate.h"""
    _run_host(DC.build_deflate_host(tmp_path), tmp_path)


def test_the_host_program_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own: blocks and slots are heap blocks of
    their exact sizes"""
    _run_host(DC.build_deflate_host(tmp_path, sanitize=True), tmp_path)
