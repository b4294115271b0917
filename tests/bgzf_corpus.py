"""Inputs of the BGZF tests of --gpu_parse (CPU and GPU tier alike): BGZF built with Python's zlib (raw deflate,
wbits = -15, the header with the 'BC' subfield, the CRC-32 / ISIZE trailer, the optional EOF member), the corpus of
members, the seeded damage, and the yardstick: Python's zlib on the same member (`verdict`)."""
import ctypes
import random
import struct
import zlib

from ntedit_amd import _lib

Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 2, 3, 4  # (zlib.h; not every Python names all three)
HEADER = 18  # of the members built here: 12 bytes, XLEN = 6, the one subfield
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZES = (0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65535, 65536)
COUNTS = (1, 2, 4, 5, 65, 257)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """the raw DEFLATE stream of data; flushes: [(offset, zlib.Z_FULL_FLUSH | zlib.Z_SYNC_FLUSH)] in mid-stream"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += c.compress(data[at:off]) + c.flush(mode)
        at = off
    return out + c.compress(data[at:]) + c.flush()


def member_of(stream, data):
    """the BGZF member around a DEFLATE stream of data; None when it would pass the format's 64 KiB"""
    total = HEADER + len(stream) + 8
    if total > 65536:
        return None
    head = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1)
    return head + stream + struct.pack("<II", zlib.crc32(data), len(data))


def member(data, **kw):
    return member_of(deflate(data, **kw), data)


def bgzf(data, block=65280, level=6, eof=True):
    """data as a BGZF file of members of `block` inflated bytes"""
    out = b"".join(member(data[i:i + block], level=level) for i in range(0, len(data), block))
    return out + (EOF_MEMBER if eof else b"")


def verdict(m):
    """Python's zlib on one member built by member_of: its inflated bytes, or None where the member is refused (a
    DEFLATE error, an end short of the data or before its end, output that is not ISIZE bytes, a CRC-32 mismatch)"""
    stream, (crc, isize) = m[HEADER:-8], struct.unpack("<II", m[-8:])
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, isize + 1)
        while not d.eof and d.unconsumed_tail and len(out) <= isize:
            tail = d.unconsumed_tail
            more = d.decompress(tail, isize + 1 - len(out))
            out += more
            if not more and d.unconsumed_tail == tail:
                break
    except zlib.error:
        return None
    if not d.eof or d.unused_data or d.unconsumed_tail or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


# ---------------------------------------------------------------------------------- contents
def fastq_text(rng, n):
    out = bytearray()
    i = 0
    while len(out) < n:
        ln = rng.randrange(40, 160)
        seq = "".join(rng.choice("ACGT") for _ in range(ln))
        qual = "".join(rng.choice("FFFFFF:,#") for _ in range(ln))
        out += ("@read%d/1\n%s\n+\n%s\n" % (i, seq, qual)).encode()
        i += 1
    return bytes(out[:n])


def content(kind, rng, n):
    if kind == "fastq":
        return fastq_text(rng, n)
    if kind == "a":
        return b"A" * n
    if kind == "random":
        return rng.randbytes(n)
    if kind == "repeat32k":  # (zlib itself looks back 32768 - 262 bytes at the most; hand_distance_32768 goes all the way)
        return (rng.randbytes(32000) * 3)[:n]
    if kind == "two":
        return bytes(rng.choice(b"AC") for _ in range(n))
    raise ValueError(kind)


CONTENTS = ("fastq", "a", "random", "repeat32k", "two")


def hand_distance_32768(rng):
    """32 KiB of random bytes, stored, then the same again as fixed-Huffman matches at distance 32768 (the format's
    largest, which zlib's own deflate never emits): 126 of length 258 and 2 of length 130"""
    half = rng.randbytes(32768)
    bits = []

    def code(value, n):  # a Huffman code: first bit first
        bits.extend((value >> (n - 1 - i)) & 1 for i in range(n))

    def extra(value, n):  # extra bits: lowest first
        bits.extend((value >> i) & 1 for i in range(n))

    extra(1, 1), extra(1, 2)  # BFINAL, fixed
    for length in [258] * 126 + [130] * 2:
        if length == 258:
            code(0b11000000 + 285 - 280, 8)
        else:
            code(0b11000000, 8), extra(130 - 115, 4)  # symbol 280: 115 .. 130
        code(29, 5), extra(32768 - 24577, 13)
    code(0, 7)  # end of block
    bits += [0] * (-len(bits) % 8)
    tail = bytes(sum(b << i for i, b in enumerate(bits[j:j + 8])) for j in range(0, len(bits), 8))
    stream = b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + half + tail
    return member_of(stream, half * 2), half * 2


def corpus():
    """[(name, member, data)]: every size at four levels, the strategies, flushes in mid-member, the five contents"""
    rng = random.Random(20261017)
    out = []

    def add(name, data, **kw):
        m = member(data, **kw)
        if m is not None:  # (65536 random or stored bytes do not fit one member)
            out.append((name, m, data))
        return m is not None

    text = fastq_text(rng, 65536)
    for n in SIZES:
        for level in (0, 1, 6, 9):
            add("fastq_%d_l%d" % (n, level), text[:n], level=level)
    assert sum(1 for name, _, _ in out if name.startswith("fastq_6553")) >= 6
    for kind in CONTENTS:
        for n in (65536, 65280, 4001):
            for level in (0, 1, 6, 9):
                add("%s_%d_l%d" % (kind, n, level), content(kind, rng, n), level=level)
    for name, strategy in (("fixed", Z_FIXED), ("huffman", Z_HUFFMAN_ONLY), ("rle", Z_RLE)):
        for kind in ("fastq", "random", "a", "two"):
            assert add("%s_%s" % (name, kind), content(kind, rng, 9001), strategy=strategy)
    for mode, tag in ((zlib.Z_FULL_FLUSH, "full"), (zlib.Z_SYNC_FLUSH, "sync")):
        assert add("flush_%s" % tag, text[:30000], flushes=[(10000, mode), (10000, mode), (20001, mode)])
        assert add("flush_%s_stored" % tag, text[:3000], level=0, flushes=[(1000, mode)])
    m, data = hand_distance_32768(rng)
    assert verdict(m) == data
    out.append(("hand_distance_32768", m, data))
    assert add("empty_stored", b"", level=0) and add("empty_fixed", b"", strategy=Z_FIXED)
    return out


def random_member(rng):
    """one seeded valid member: random level, strategy, content and size"""
    while True:
        kind = rng.choice(CONTENTS)
        n = rng.choice((rng.randrange(0, 600), rng.randrange(0, 600), rng.randrange(0, 9000), rng.randrange(0, 65537)))
        data = content(kind, rng, n)
        flushes = [(rng.randrange(0, n + 1), rng.choice((zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH)))] if rng.random() < 0.2 else []
        m = member(data, level=rng.choice((0, 1, 6, 9)),
                   strategy=rng.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED)), flushes=flushes)
        if m is not None:
            return m, data


def damage_bases():
    """the members the damage is done to: small, one of every block type and strategy"""
    rng = random.Random(5)
    text = fastq_text(rng, 3000)
    return [member(text, level=6), member(text, level=1), member(text, level=0), member(text, strategy=Z_FIXED),
            member(text, strategy=Z_HUFFMAN_ONLY), member(text[:1500], flushes=[(700, zlib.Z_SYNC_FLUSH)]),
            member(content("random", rng, 700), level=6), member(content("two", rng, 2000), level=9),
            member(b"A" * 2500, level=6), member(content("two", rng, 2000), strategy=Z_RLE)]


def damaged(n_flips=2000, n_cuts=300, seed=99):
    """[(what, member)]: single-bit flips over the DEFLATE data and the trailer, and truncations of the DEFLATE data (the
    trailer kept, the header's size corrected); the first cases of a longer list are the same cases"""
    rng = random.Random(seed)
    bases = damage_bases()
    out = []
    for _ in range(n_flips):
        j = rng.randrange(len(bases))
        m = bytearray(bases[j])
        bit = rng.randrange(HEADER * 8, len(m) * 8)
        m[bit >> 3] ^= 1 << (bit & 7)
        out.append(("flip %d of base %d" % (bit, j), bytes(m)))
    cuts = []
    for _ in range(n_cuts):
        j = rng.randrange(len(bases))
        m = bases[j]
        keep = rng.randrange(0, len(m) - HEADER - 8)
        cuts.append(("cut of base %d to %d" % (j, keep), member_of(m[HEADER:HEADER + keep], b"")[:-8] + m[-8:]))
    return out, cuts


# ---------------------------------------------------------------------------------- the library
def walk(lib, buf, cap=1 << 16):
    """ntedit_hip_bgzf_walk -> (why it stopped, the members, consumed)"""
    members = (_lib.BgzfMember * max(cap, 1))()
    n, used = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.ntedit_hip_bgzf_walk(buf, len(buf), members if cap else None, cap, n, used)
    assert rc >= 0
    return rc, [members[i] for i in range(n.value)], used.value


def table(members):
    return (_lib.BgzfMember * max(len(members), 1))(*members)


def table_of(ms):
    """the concatenation of members built by member_of and its table, made here (not by the walker)"""
    blob, t, out = bytearray(), [], 0
    for m in ms:
        isize = struct.unpack("<I", m[-4:])[0]
        t.append(_lib.BgzfMember(in_off=len(blob) + HEADER, out_off=out, n_in=len(m) - HEADER - 8, n_out=isize,
                                 crc=struct.unpack("<I", m[-8:-4])[0]))
        blob += m
        out += isize
    return bytes(blob), t, out


GUARD = 64


def model(lib, blob, members, n_out):
    """ntedit_hip_reads_inflate_model -> (statuses, the output bytes); the 0xEE guard behind out_cap is checked"""
    out = ctypes.create_string_buffer(b"\xEE" * (n_out + GUARD), n_out + GUARD)
    status = (ctypes.c_uint32 * max(len(members), 1))()
    rc = lib.ntedit_hip_reads_inflate_model(blob, len(blob), table(members), len(members), out, n_out, status)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    assert out.raw[n_out:] == b"\xEE" * GUARD
    return list(status)[:len(members)], out.raw[:n_out]


def python_last_record_start(buf, kind):
    """the chunk cut's rule: the last line start past byte 0 that starts a record, or None"""
    starts = [i + 1 for i, c in enumerate(buf[:-1]) if c == 10]  # the line starts inside the buffer, but the first
    for j in range(len(starts) - 1, -1, -1):
        s = starts[j]
        if kind == ord(">"):
            if buf[s] == ord(">"):
                return s
        elif buf[s] == ord("@") and j + 2 < len(starts) and buf[starts[j + 2]] == ord("+"):
            return s
    return None
