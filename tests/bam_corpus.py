"""Inputs of the BAM tests of --gpu_parse (CPU and GPU tier alike): a BAM writer (struct and zlib), the corpus of cases,
each with its BAM file bytes, its inflated bytes, its twin FASTQ and the expected result, and `restate`: the definition of
DESIGN.md 9.17 written a second time, in Python, independent of nte_bam_grammar.h."""
import ctypes
import random
import struct
import zlib

from ntedit_amd import _lib

K = 25
CODES = b"=ACMGRSVTWYHKDBN"
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FIELDS = ("clean", "broken", "header_len", "n_ref", "cut", "records", "kept", "skipped_flag", "skipped_short", "bases",
          "text_len")
ALIGN = 8192  # the decoys start at a multiple of it: a segment start at every segment size the tests force
GUARD = 64


# ---------------------------------------------------------------------------------------------- the writer
def member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    stream = c.compress(data) + c.flush()
    if 18 + len(stream) + 8 > 65536:
        return member(data[:len(data) // 2], level) + member(data[len(data) // 2:], level)
    head = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(stream) + 8 - 1)
    return head + stream + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(data, sizes=(65280,), eof=True):
    """data as BGZF members of the inflated sizes given (the last size repeats)"""
    out, at, i = [], 0, 0
    while at < len(data):
        n = sizes[min(i, len(sizes) - 1)]
        out.append(member(data[at:at + n]))
        at += n
        i += 1
    return b"".join(out) + (EOF_MEMBER if eof else b"")


def pack_seq(seq):
    codes = [CODES.index(bytes([b])) for b in seq] + [0]
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))


def record(name, flag, seq, qual=None, cigar=(), aux=b"", ref=-1, pos=-1):
    qual = b"\xff" * len(seq) if qual is None else qual
    assert len(qual) == len(seq) and 1 <= len(name) <= 254
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 30, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + qual + aux
    return struct.pack("<i", len(body)) + body


def header(text=b"", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def all_aux():
    """one tag of every type, the B arrays of every element type included"""
    out = b"XAAQ" + b"Xbc" + struct.pack("<b", -3) + b"XcC\x07" + b"Xds" + struct.pack("<h", -300) + b"XeS\x01\x02"
    out += b"Xfi" + struct.pack("<i", -70000) + b"XgI" + struct.pack("<I", 4000000000) + b"Xhf" + struct.pack("<f", 1.5)
    out += b"XiZa string @ > with\nmarks\0" + b"XjH1AE301\0"
    for t, fmt in ((b"c", "<b"), (b"C", "<B"), (b"s", "<h"), (b"S", "<H"), (b"i", "<i"), (b"I", "<I"), (b"f", "<f")):
        out += b"Y" + t + b"B" + t + struct.pack("<i", 5) + b"".join(struct.pack(fmt, v) for v in (1, 2, 3, 4, 5))
    return out


# ---------------------------------------------------------------------------------------------- the restatement
def restate(raw, at_header=1, min_len=K):
    """-> (the result fields as a dict, the text).  SAM specification 4.2, restated: see DESIGN.md 9.17."""
    n = len(raw)
    res = dict.fromkeys(FIELDS, 0)

    def unclean(bit, at):
        r = dict.fromkeys(FIELDS, 0)
        r.update(broken=bit, cut=at)
        return r, b""

    if n >= 1 << 31:
        return unclean(_lib.BAM_BAD_SIZE, 0)
    p = 0
    if at_header:
        if raw[:4] != b"BAM\1"[:min(n, 4)]:
            return unclean(_lib.BAM_BAD_MAGIC, 0)
        grows = dict(res, clean=1)  # a header that ends behind the bytes at hand: cut 0
        if n < 8:
            return grows, b""
        l_text, = struct.unpack_from("<i", raw, 4)
        if l_text < 0:
            return unclean(_lib.BAM_BAD_HEADER, 0)
        p = 8 + l_text
        if p + 4 > n:
            return grows, b""
        n_ref, = struct.unpack_from("<i", raw, p)
        if n_ref < 0:
            return unclean(_lib.BAM_BAD_HEADER, 0)
        p += 4
        for _ in range(n_ref):
            if p + 4 > n:
                return grows, b""
            l_name, = struct.unpack_from("<i", raw, p)
            if l_name < 1:
                return unclean(_lib.BAM_BAD_HEADER, 0)
            p += 4 + l_name + 4
            if p > n:
                return grows, b""
        res.update(header_len=p, n_ref=n_ref)
    text = []
    while p < n:
        if n - p < 4:
            break
        block, = struct.unpack_from("<i", raw, p)
        if block < 0 or block >= 1 << 30:
            return unclean(_lib.BAM_BAD_SIZE, p)
        if block < 32:
            return unclean(_lib.BAM_BAD_RECORD, p)
        if n - p < 36:
            break
        l_read_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHI", raw, p + 12)
        if l_read_name < 1 or 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block:
            return unclean(_lib.BAM_BAD_RECORD, p)
        if p + 4 + block > n:
            break
        res["records"] += 1
        if flag & 0x900:
            res["skipped_flag"] += 1
        elif l_seq < min_len:
            res["skipped_short"] += 1
        else:
            at = p + 36 + l_read_name + 4 * n_cigar
            packed = raw[at:at + (l_seq + 1) // 2]
            bases = bytes(CODES[b >> 4 if j % 2 == 0 else b & 15] for j, b in ((j, packed[j // 2]) for j in range(l_seq)))
            text.append(bases + b"\n")
            res["kept"] += 1
            res["bases"] += l_seq
        p += 4 + block
    text = b"".join(text)
    res.update(clean=1, cut=p, text_len=len(text))
    return res, text


def restate_first_member(data):
    """the first 4 inflated bytes of the BGZF members data starts with (as many as it takes, each completely inside),
    else None"""
    out = b""
    while len(out) < 4:
        m = _restate_member(data)
        if m is None:
            return None
        size, more = m
        out += more
        data = data[size:]
    return out[:4]


def _restate_member(data):
    """the size and the inflated bytes of the BGZF member data starts with when it lies completely inside, else None"""
    if len(data) < 20 or data[:4] != b"\x1f\x8b\x08\x04":
        return None
    xlen, = struct.unpack_from("<H", data, 10)
    extra, size, x = data[12:12 + xlen], None, 0
    if len(extra) < xlen:
        return None
    while x + 4 <= xlen:
        slen, = struct.unpack_from("<H", extra, x + 2)
        if extra[x:x + 2] == b"BC" and slen == 2 and x + 6 <= xlen:
            size = struct.unpack_from("<H", extra, x + 4)[0] + 1
        x += 4 + slen
    if size is None or size > len(data) or size < 12 + xlen + 8:
        return None
    try:
        out = zlib.decompressobj(-15).decompress(data[12 + xlen:size - 8])
    except zlib.error:
        return None
    return size, out


def twin(reads):
    """the FASTQ of the same reads in the same order: every read that is neither secondary nor supplementary (the empty
    ones left out: an empty line is outside the clean FASTQ grammar, and no parser keeps a read below k)"""
    return b"".join(b"@%s\n%s\n+\n%s\n" % (name.replace(b" ", b"_").replace(b"\n", b"_"), seq, b"I" * len(seq))
                    for name, flag, seq in reads if not flag & 0x900 and seq)


# ---------------------------------------------------------------------------------------------- the corpus
class Case:
    def __init__(self, name, head, recs, sizes=(65280,), eof=True, decoy=False):
        """recs: [(name, flag, seq, record bytes)]"""
        self.name, self.decoy = name, decoy
        self.raw = head + b"".join(r[3] for r in recs)
        self.bam = bgzf(self.raw, sizes, eof)
        self.reads = [r[:3] for r in recs]
        self.twin = twin(self.reads)
        self.header_len = len(head)
        self.starts = []
        at = len(head)
        for r in recs:
            self.starts.append(at)
            at += len(r[3])


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _rec(name, flag, seq, **kw):
    return (name, flag, seq, record(name, flag, seq, **kw))


def _plain(rng, count, tag=b"r", lengths=(100, 151), flags=(0,)):
    return [_rec(b"%s%d" % (tag, i), flags[i % len(flags)], _seq(rng, lengths[i % len(lengths)])) for i in range(count)]


def _decoy_chain(rng, count=5):
    """byte-exact images of `count` clean records, one behind the other"""
    return b"".join(record(b"d%d" % i, 0, _seq(rng, 30)) for i in range(count))


def _decoy_case(rng):
    recs = _plain(rng, 20, b"a")
    at = len(header()) + sum(len(r[3]) for r in recs)
    for round_, how in enumerate(("qual", "aux", "qual")):
        chain = _decoy_chain(rng)
        name = b"host%d" % round_
        for length in range(K, K + 3 * ALIGN):  # the length at which the image starts at a multiple of ALIGN
            if how == "qual":
                if length < len(chain):
                    continue
                inside = 36 + len(name) + 1 + (length + 1) // 2 + (length - len(chain))
            else:
                inside = 36 + len(name) + 1 + (length + 1) // 2 + length + 8  # (tag, 'B', 'C', the count)
            if (at + inside) % ALIGN == 0:
                break
        else:
            raise AssertionError("no length aligns the decoy")
        seq = _seq(rng, length)
        if how == "qual":
            rec = _rec(name, 0, seq, qual=b"\x21" * (length - len(chain)) + chain)
        else:
            rec = _rec(name, 0, seq, aux=b"ZDBC" + struct.pack("<i", len(chain)) + chain)
        assert rec[3].find(chain) == inside and (at + inside) % ALIGN == 0
        recs.append(rec)
        at += len(rec[3])
        more = _plain(rng, 12, b"b%d_" % round_)
        recs += more
        at += sum(len(r[3]) for r in more)
    return Case("decoys", header(), recs, decoy=True)


def corpus():
    rng = random.Random(42)
    cases = []
    flags = (0, 0x4, 0x10, 0x100, 0x800, 0x900, 0x4 | 0x10, 0x1 | 0x40, 0x1 | 0x80 | 0x10)
    cases.append(Case("unaligned_header", header(b"@HD\tVN:1.6\tSO:unknown\n"), _plain(rng, 300, flags=(0x4,))))
    cases.append(Case("one_reference", header(b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n", [(b"chr1", 100000)]),
                      _plain(rng, 200, flags=flags)))
    cases.append(Case("300_references", header(b"@HD\tVN:1.6\n", [(b"contig_%d" % i, 1000 + i) for i in range(300)]),
                      _plain(rng, 100, flags=flags), sizes=(700, 33, 4000)))
    cases.append(Case("header_longer_than_a_member", header(b"@CO\t" + _seq(rng, 150000, b"abcdefgh @>\n"), [(b"c", 5)]),
                      _plain(rng, 50, flags=flags)))
    # every length around k and the packing's parity, every nibble code, and a read of 70,000
    lens = (0, 1, 2, K - 1, K, K + 1, 151, 150, 70000, 33, 0, 64, 1)
    recs = [_rec(b"len%d_%d" % (i, n), flags[i % 3], _seq(rng, n, CODES if i % 2 else b"ACGT")) for i, n in enumerate(lens)]
    recs.append(_rec(b"codes", 0, CODES * 3))
    cases.append(Case("lengths_and_codes", header(), recs, sizes=(5000,)))
    # names of 1 and 254 characters, no and many CIGAR operations, every aux type
    recs = []
    for i in range(60):
        name = (b"n", b"N" * 254, b"read/%d" % i)[i % 3]
        cigar = ((), tuple((10 + j) << 4 | j % 9 for j in range(400)), (100 << 4,))[(i // 3) % 3]
        recs.append(_rec(name, flags[i % len(flags)], _seq(rng, 90 + i), cigar=cigar, aux=all_aux() if i % 2 else b"",
                         ref=0 if i % 4 else -1, pos=i * 10))
    cases.append(Case("names_cigars_aux", header(b"", [(b"chr1", 100000)]), recs, sizes=(1000,)))
    rs = random.Random(7)
    cases.append(Case("random_members", header(b"@HD\n"), _plain(rng, 1500, flags=flags),
                      sizes=(1, 2, 65280, 1, 3, 17) + tuple(rs.choice((1, 2, 3, 17, 300, 4000, rs.randrange(1, 65281)))
                                                            for _ in range(4000))))
    # a member boundary at each of the first 40 bytes of a record
    recs, sizes, at, last = _plain(rng, 41, b"cut"), [], len(header()), 0
    for i in range(40):
        sizes.append(at + i - last)
        last = at + i
        at += len(recs[i][3])
    cases.append(Case("members_cut_records", header(), recs, sizes=tuple(sizes) + (65280,)))
    cases.append(Case("no_eof_member", header(), _plain(rng, 150, flags=flags), sizes=(3000,), eof=False))
    cases.append(Case("long_reads", header(), _plain(rng, 6, b"hifi", lengths=(15000, 20000, 17001))))
    cases.append(Case("header_only", header(b"@HD\n", [(b"c", 9)]), []))
    cases.append(_decoy_case(rng))
    for c in cases:
        assert len(c.bam) < 600000, c.name
    return cases


def result_dict(res):
    return {f: getattr(res, f) for f in FIELDS}


def model(lib, raw, at_header=1, min_len=K):
    """ntedit_hip_reads_bam_model -> (rc, the result fields, the text); guard bytes behind the text are checked"""
    cap = len(raw) + 1
    out = ctypes.create_string_buffer(b"\xEE" * (cap + GUARD), cap + GUARD)
    res = _lib.ReadsBamResult()
    rc = lib.ntedit_hip_reads_bam_model(raw, len(raw), at_header, min_len, out, cap, res)
    assert out.raw[cap:] == b"\xEE" * GUARD
    r = result_dict(res)
    return rc, r, out.raw[:r["text_len"]] if r["clean"] else b""
