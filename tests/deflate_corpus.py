"""Inputs of the BGZF writer's tests (CPU and GPU tier alike), seeded: the smallest inputs at which the encoder of
nte_bgzf_deflate.h can go wrong, the walk over the members it writes, and the library calls the tests share.  Test
infrastructure only."""
import ctypes
import functools
import gzip
import os
import random
import struct
import subprocess
import zlib

import helpers as H
from ntedit_amd import _lib

BLOCK = _lib.BGZF_BLOCK  # 65,280 plain bytes to a member
HEADER, TRAILER = 18, 8
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
DEMO_DRAFT = os.path.join(H.GOLDEN, "demo", "ecoliWithMismatches001Indels0001.fa.gz")
HOST_SRC = os.path.join(H.ROOT, "tests", "bgzf", "deflate_host.cpp")
# names of the entries that must come out as stored blocks, every member of them
STORED = ("uniform_256x255", "random_65280")
FIB_COUNTS = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711]


def acgt(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def fasta_text(rng, n, first_header=1):
    """one-line FASTA with lower case, N runs and IUPAC codes; the first header line is first_header bytes"""
    out = bytearray()
    i = 0
    while len(out) < n:
        name = b"c%d a contig" % i if i else (b"h" * first_header)
        seq = bytearray(acgt(rng, rng.randrange(50, 30000)))
        for _ in range(rng.randrange(0, 4)):
            q, n_low = rng.randrange(0, len(seq)), rng.randrange(1, 400)
            seq[q:q + n_low] = bytes(seq[q:q + n_low]).lower()
        for _ in range(rng.randrange(0, 3)):
            q, n_run = rng.randrange(0, len(seq)), rng.randrange(1, 200)
            seq[q:q + n_run] = b"N" * len(seq[q:q + n_run])
        for _ in range(rng.randrange(0, 12)):
            seq[rng.randrange(0, len(seq))] = rng.choice(b"RYSWKMBDHV")
        out += b">" + name + b"\n" + bytes(seq) + b"\n"
        i += 1
    return bytes(out[:n])


def huffman_depth(counts):
    """the unrestricted Huffman code's longest length over these counts (a heap of (weight, depth of the subtree))"""
    import heapq
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def demo_draft():
    """the E. coli demo draft as one-line FASTA"""
    return b"".join(b">" + name + b"\n" + seq + b"\n" for name, seq in H.read_fasta(DEMO_DRAFT))


@functools.lru_cache(maxsize=None)
def corpus():
    """((name, bytes), ...)"""
    rng = random.Random(20261019)
    out = [("acgt_%d" % n, acgt(rng, n)) for n in range(1, 301)]
    out += [("acgt_%d" % n, acgt(rng, n)) for n in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1)]
    out.append(("one_value", b"G" * BLOCK))
    out.append(("uniform_256x255", bytes(range(256)) * 255))
    out.append(("random_65280", rng.randbytes(BLOCK)))
    fib = bytearray()
    for i, c in enumerate(FIB_COUNTS):
        fib += bytes([33 + 7 * i]) * c
    rng.shuffle(fib)
    assert len(fib) == 46366 and huffman_depth(FIB_COUNTS + [1]) == 21  # (with the end-of-block symbol)
    out.append(("fibonacci_21", bytes(fib)))
    out.append(("fasta_header_1", fasta_text(rng, 40000, first_header=1)))
    out.append(("fasta_header_300", fasta_text(rng, 40000, first_header=300)))
    out.append(("fasta_39_blocks", fasta_text(rng, 2_500_000)))
    assert (len(out[-1][1]) + BLOCK - 1) // BLOCK == 39
    out.append(("demo_draft", demo_draft()))
    return tuple(out)


def blocks(data):
    return [data[i:i + BLOCK] for i in range(0, len(data), BLOCK)]


def walk(bgzf):
    """[(member, deflate payload, crc, isize)] of a series of BGZF members: magic, FLG, XLEN, 'BC', BSIZE checked"""
    out, o = [], 0
    while o < len(bgzf):
        head = bgzf[o:o + HEADER]
        assert head[:4] == b"\x1f\x8b\x08\x04" and head[10:16] == b"\x06\x00BC\x02\x00", (o, head)
        size = struct.unpack("<H", head[16:18])[0] + 1
        assert HEADER + TRAILER < size <= 65536 and o + size <= len(bgzf), (o, size)
        m = bgzf[o:o + size]
        crc, isize = struct.unpack("<II", m[-TRAILER:])
        out.append((m, m[HEADER:-TRAILER], crc, isize))
        o += size
    return out


def check_members(bgzf, plain):
    """every member against its slice of plain: CRC-32, ISIZE, the payload through zlib; -> the stored members"""
    ms = walk(bgzf)
    assert len(ms) == (len(plain) + BLOCK - 1) // BLOCK
    stored = 0
    for (m, payload, crc, isize), blk in zip(ms, blocks(plain)):
        assert isize == len(blk) and crc == zlib.crc32(blk)
        assert zlib.decompress(payload, -15) == blk
        is_stored = (payload[0] & 7) == 1  # BFINAL, BTYPE 00
        assert is_stored or (payload[0] & 7) == 5  # ... or BTYPE 10
        assert not is_stored or len(m) == HEADER + 5 + len(blk) + TRAILER
        stored += is_stored
    return stored


def model(lib, data, cap=None):
    """ntedit_hip_bgzf_deflate_model -> the members; a 0xEE guard behind cap is checked"""
    cap = lib.ntedit_hip_bgzf_bound(len(data)) if cap is None else cap
    guard = 64
    out = ctypes.create_string_buffer(b"\xEE" * (cap + guard), cap + guard)
    n = ctypes.c_uint64()
    rc = lib.ntedit_hip_bgzf_deflate_model(data, len(data), out, cap, ctypes.byref(n))
    assert out.raw[cap:] == b"\xEE" * guard
    assert rc == 0, (rc, n.value)
    return out.raw[:n.value]


@functools.lru_cache(maxsize=None)
def model_of_corpus():
    """{name: members}: the reference of both tiers, computed once"""
    lib = _lib.load()
    return {name: model(lib, data) for name, data in corpus()}


def gunzip(bgzf):
    return gzip.decompress(bgzf) if bgzf else b""


def write_cases(path, entries):
    """the corpus as the host program reads it: u32 count, then u32 length and the bytes of each entry"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(entries)))
        for _, data in entries:
            f.write(struct.pack("<I", len(data)) + data)


def build_deflate_host(out_dir, sanitize=False):
    """g++ build of tests/bgzf/deflate_host.cpp; returns its path"""
    exe = os.path.join(str(out_dir), "deflate_host_san" if sanitize else "deflate_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(H.ROOT, "ntedit_amd", "csrc"), "-o", exe,
                                                                         HOST_SRC, "-lz"], check=True)
    return exe
