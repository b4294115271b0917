"""--gpu_parse on BGZF reads, the CPU tier: the decoder of nte_bgzf_inflate.h as the serial host model runs it
(ntedit_hip_reads_inflate_model) against Python's zlib -- on the corpus, on damaged members and on seeded random
members -- the member walker, and the chunk cut's rule.  The device runs the same functions (tests/test_gpu_reads_inflate.py);
this tier exercises their bounds logic under the host build first."""
import ctypes
import random
import struct

import pytest

import bgzf_corpus as BC
import parse_corpus as PC
from ntedit_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return BC.corpus()


def test_the_corpus_covers_what_it_should(corpus):
    names = [n for n, _, _ in corpus]
    sizes = {len(d) for _, _, d in corpus}
    assert set(BC.SIZES) <= sizes
    for must in ("fastq_65536_l6", "fastq_65535_l1", "a_65536_l6", "random_65280_l0", "repeat32k_65536_l9", "hand_distance_32768", "two_65536_l6",
                 "fixed_fastq", "huffman_random", "rle_a", "flush_full", "flush_sync_stored", "fastq_0_l0"):
        assert must in names, must
    for _, m, d in corpus:
        assert BC.verdict(m) == d and len(m) <= 65536


def test_the_model_equals_zlib_on_the_corpus(lib, corpus):
    blob, members, n_out = BC.table_of([m for _, m, _ in corpus])
    status, out = BC.model(lib, blob, members, n_out)
    assert status == [0] * len(corpus), [(corpus[i][0], s) for i, s in enumerate(status) if s]
    assert out == b"".join(d for _, _, d in corpus)
    # ... and member by member, each with its own guard
    for name, m, d in corpus[::7]:
        blob, members, n_out = BC.table_of([m])
        assert BC.model(lib, blob, members, n_out) == ([0], d), name


def test_the_walker_finds_the_members_the_corpus_was_built_from(lib, corpus):
    ms = [m for _, m, _ in corpus]
    blob, members, n_out = BC.table_of(ms)
    rc, found, used = BC.walk(lib, blob)
    assert rc == _lib.BGZF_END and used == len(blob) and len(found) == len(ms)
    for a, b in zip(found, members):
        assert (a.in_off, a.out_off, a.n_in, a.n_out, a.crc) == (b.in_off, b.out_off, b.n_in, b.n_out, b.crc)
    # the EOF member is a member like any other
    rc, found, used = BC.walk(lib, ms[0] + BC.EOF_MEMBER)
    assert rc == _lib.BGZF_END and [m.n_out for m in found] == [len(corpus[0][2]), 0] and used == len(ms[0]) + 28
    # cap: stops full, at a member boundary
    rc, found, used = BC.walk(lib, blob, cap=3)
    assert rc == _lib.BGZF_FULL and len(found) == 3 and used == sum(len(m) for m in ms[:3])
    rc, found, used = BC.walk(lib, blob, cap=0)
    assert rc == _lib.BGZF_FULL and used == 0
    assert BC.walk(lib, b"") == (_lib.BGZF_END, [], 0)


def test_the_walker_on_buffers_cut_anywhere(lib):
    rng = random.Random(3)
    a, b = BC.member(BC.fastq_text(rng, 2000)), BC.member(BC.fastq_text(rng, 900), level=1)
    whole = a + b
    for cut in list(range(len(a), len(a) + BC.HEADER + 3)) + [len(a) + 100, len(whole) - 9, len(whole) - 8, len(whole) - 4, len(whole) - 1]:
        rc, found, used = BC.walk(lib, whole[:cut])
        assert len(found) == 1 and used == len(a), cut
        assert rc == (_lib.BGZF_END if cut == len(a) else _lib.BGZF_CUT), cut
    for cut in (1, 3, 11, 17, 18, 500, len(a) - 1):
        assert BC.walk(lib, a[:cut]) == (_lib.BGZF_CUT, [], 0), cut


def test_the_walker_stops_at_what_is_not_bgzf(lib):
    import gzip
    rng = random.Random(4)
    a, b = BC.member(BC.fastq_text(rng, 2000)), BC.member(BC.fastq_text(rng, 900))
    plain = gzip.compress(b"@r\nACGT\n+\nIIII\n")
    rc, found, used = BC.walk(lib, a + plain + b)
    assert rc == _lib.BGZF_NOT and len(found) == 1 and used == len(a)
    assert BC.walk(lib, plain)[0] == _lib.BGZF_NOT and BC.walk(lib, b"@r\nACGT\n")[0] == _lib.BGZF_NOT
    assert BC.walk(lib, a + b"\x1f")[0] == _lib.BGZF_CUT and BC.walk(lib, a + b"\x1f\x8c")[0] == _lib.BGZF_NOT
    # a 'BC' size smaller than the member's own header and trailer, an ISIZE over 64 KiB
    bad = bytearray(a)
    bad[16:18] = struct.pack("<H", 20)
    assert BC.walk(lib, bytes(bad))[0] == _lib.BGZF_NOT
    bad = bytearray(a)
    bad[-4:] = struct.pack("<I", 65537)
    assert BC.walk(lib, bytes(bad))[0] == _lib.BGZF_NOT


def same_verdict(lib, what, m):
    """the model's verdict on one member equals zlib's: both refuse, or both accept with the same bytes"""
    want = BC.verdict(m)
    isize = struct.unpack("<I", m[-4:])[0]
    if isize > 65536:  # (a flipped ISIZE: no BGZF member, the walker says so; zlib cannot make that many bytes of it)
        assert want is None and BC.walk(lib, m)[0] == _lib.BGZF_NOT, what
        return want
    blob, members, n_out = BC.table_of([m])
    status, out = BC.model(lib, blob, members, n_out)
    if want is None:
        assert status[0] != 0, what
    else:
        assert status[0] == 0 and out == want, (what, status)
    return want


def test_damaged_members_get_zlibs_verdict(lib):
    flips, cuts = BC.damaged()
    assert len(flips) == 2000 and len(cuts) == 300
    for what, m in flips:
        same_verdict(lib, what, m)
    for what, m in cuts:
        assert same_verdict(lib, what, m) is None, what


def test_a_flip_in_the_padding_behind_the_final_block_is_accepted(lib):
    found = 0
    for base in BC.damage_bases():
        m = bytearray(base)
        m[-9] ^= 0x80  # the last bit of the DEFLATE data
        if BC.verdict(bytes(m)) is not None:
            found += 1
            assert same_verdict(lib, "padding", bytes(m)) == BC.verdict(base)
    assert found >= 3


def test_every_reason_is_reported(lib):
    """hand-made streams, one per reason code"""
    def status_of(stream, data_len, crc=0):
        m = BC.member_of(stream, b"")[:-8] + struct.pack("<II", crc, data_len)
        blob, members, n_out = BC.table_of([m])
        return BC.model(lib, blob, members, n_out)[0][0]
    import zlib
    text = b"ACGTACGTACGTTTGACA" * 20
    good = BC.deflate(text)
    assert status_of(good, len(text), zlib.crc32(text)) == 0
    assert status_of(good, len(text), zlib.crc32(text) ^ 1) == 8           # CRC
    assert status_of(good, len(text) + 1, zlib.crc32(text)) == 6           # short output
    assert status_of(good, len(text) - 1, zlib.crc32(text)) == 4           # output overrun
    assert status_of(good + b"\0", len(text), zlib.crc32(text)) == 7       # left-over input
    assert status_of(good[:-3], len(text), zlib.crc32(text)) == 5          # input overrun
    assert status_of(b"\x07", 0) == 1                                      # block type 3
    assert status_of(b"\x01\x05\x00\xfa\xfe" + b"x" * 5, 5) == 9           # stored: LEN is not ~NLEN
    assert status_of(b"\x01\x05\x00\xfa\xff" + b"x" * 4, 5) == 5           # stored: bytes missing
    # fixed block, a match at distance 1 before any byte: length code 257 (0000001), distance code 0 (00000)
    assert status_of(bytes([0b00000011, 0b00000010, 0]), 3) == 3
    # dynamic block with 30 + 257 = 287 literal/length codes
    assert status_of(bytes([0b11110101, 0b00000000, 0, 0, 0]), 0) == 2
    assert status_of(b"", 0) == 5 and status_of(BC.deflate(b""), 0, 0) == 0


def test_seeded_random_members(lib):
    rng = random.Random(1951)
    done = 0
    while done < 3000:
        batch = [BC.random_member(rng) for _ in range(min(100, 3000 - done))]
        blob, members, n_out = BC.table_of([m for m, _ in batch])
        status, out = BC.model(lib, blob, members, n_out)
        assert status == [0] * len(batch), (done, status)
        assert out == b"".join(d for _, d in batch), done
        done += len(batch)


def test_members_outside_their_buffers_are_an_argument_error(lib):
    m = BC.member(b"ACGT" * 100)
    blob, members, n_out = BC.table_of([m])
    status = (ctypes.c_uint32 * 1)()
    out = ctypes.create_string_buffer(n_out)
    for field, value in (("in_off", len(blob)), ("n_in", len(blob)), ("out_off", 1), ("n_out", n_out + 1)):
        t = BC.table(members)
        setattr(t[0], field, value)
        assert lib.ntedit_hip_reads_inflate_model(blob, len(blob), t, 1, out, n_out, status) == _lib.E_ARG, field


def test_the_cut_rule_against_its_restatement(lib):
    bufs = list(PC.well_formed().items()) + list(PC.odd().items()) + [(str(i), raw) for i, (raw, _, _) in enumerate(PC.generated(60))]
    checked = hits = 0
    for name, raw in bufs:
        if not raw:
            continue
        for n in {len(raw), len(raw) - 1, len(raw) * 2 // 3, len(raw) // 2, 2, 1}:
            if n < 1:
                continue
            for kind in (ord(">"), ord("@")):
                want = BC.python_last_record_start(raw[:n], kind)
                got = lib.ntedit_hip_reads_last_record_start(raw, n, kind)
                assert got == (_lib.READS_NO_START if want is None else want), (name, n, chr(kind))
                checked += 1
                hits += want is not None
    assert checked > 300 and hits > 100


SANITIZED = r"""
// every case of a file through nte_bgzf_inflate.h, input and output in heap blocks of exactly n_in and n_out bytes
#include "nte_bgzf_inflate.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv)
{
	FILE* f = fopen(argv[1], "rb");
	uint32_t n = 0, head[3];
	if (!f || fread(&n, 4, 1, f) != 1) return 2;
	nte_bgzf::BzTables* t = new nte_bgzf::BzTables();
	for (uint32_t i = 0; i < n; i++) {
		if (fread(head, 4, 3, f) != 3) return 2;
		uint8_t* in = (uint8_t*)malloc(head[0] ? head[0] : 1);
		uint8_t* out = (uint8_t*)malloc(head[1] ? head[1] : 1);
		if (head[0] && fread(in, 1, head[0], f) != head[0]) return 2;
		uint8_t* in_exact = (uint8_t*)malloc(head[0]); // (a block of 0 bytes: any access is reported)
		memcpy(in_exact, in, head[0]);
		uint32_t st = nte_bgzf::bz_inflate(in_exact, head[0], out, head[1], t, 0, 1);
		if (st == 0) {
			uint32_t crc = 0;
			for (uint32_t lane = 0; lane < 64; lane++) crc ^= nte_bgzf::bz_crc_term(out, head[1], lane, 64);
			if (~crc != head[2]) st = nte_bgzf::BZ_BAD_CRC;
		}
		printf("%u\n", st);
		free(in), free(in_exact), free(out);
	}
	delete t;
	return 0;
}
"""


def test_the_decoder_under_address_and_undefined_behaviour_sanitizers(lib, corpus, tmp_path):
    """the header alone, built for the host with -fsanitize=address,undefined: the corpus, all the damaged members and
    300 random ones, every buffer a heap block of its exact size; the statuses are the library model's"""
    import shutil
    import subprocess
    import helpers as H
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    (tmp_path / "san.cpp").write_text(SANITIZED)
    exe = tmp_path / "san"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-I", H.ROOT + "/ntedit_amd/csrc", "-o", str(exe), str(tmp_path / "san.cpp")], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + build.stderr[-300:])
    flips, cuts = BC.damaged()
    rng = random.Random(8)
    cases = [m for _, m, _ in corpus] + [m for _, m in flips + cuts] + [BC.random_member(rng)[0] for _ in range(300)]
    cases = [m for m in cases if struct.unpack("<I", m[-4:])[0] <= 65536]
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for m in cases:
            crc, isize = struct.unpack("<II", m[-8:])
            f.write(struct.pack("<III", len(m) - BC.HEADER - 8, isize, crc) + m[BC.HEADER:-8])
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [int(x) for x in r.stdout.split()]
    blob, members, n_out = BC.table_of(cases)
    want, _ = BC.model(lib, blob, members, n_out)
    assert got == want
