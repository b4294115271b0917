"""The twin of --min_qual (CPU and GPU tier alike): the definition written a second time, in Python, and the inputs the
tests share.  With --min_qual Q a base whose Phred quality is below Q enters the batch text as N, so a filter built WITH
the flag from a file equals, byte for byte, the filter built WITHOUT it from that file with those bases rewritten to N:
`mask` does the rewrite on 4-line FASTQ bytes, `mask_records` on (name, sequence, qualities) records that the writers
below lay out in the shapes the host parser has to follow by kseq's rules (multi-line, CR LF, gzip)."""
import ctypes
import random
import struct

import bam_corpus as BAM
from ntedit_amd import _lib

QS = (1, 20, 93)
K = 25
NO_QUAL = None  # a record's qualities: absent (a FASTA record; in BAM, 0xFF bytes)


def masked(seq, qual, q):
    """seq with every base whose quality character (Phred+33) is below 33 + q rewritten to N"""
    return bytes(78 if c < 33 + q else b for b, c in zip(seq, qual))


def mask(raw, q):
    """4-line FASTQ bytes ('\\n' or '\\r\\n' line ends, a last line with or without its line end) -> the same bytes
    with the masked bases rewritten; a record that starts with '>' (one-line FASTA) passes as it is"""
    lines = raw.split(b"\n")
    i = 0
    while i < len(lines):
        if lines[i].startswith(b"@") and i + 3 < len(lines):
            seq, qual = lines[i + 1], lines[i + 3]
            cr = seq.endswith(b"\r")
            body = seq[:-1] if cr else seq
            qual = qual[:-1] if qual.endswith(b"\r") else qual
            lines[i + 1] = masked(body, qual, q) + body[len(qual):] + (b"\r" if cr else b"")
            i += 4
        else:
            i += 1
    return b"\n".join(lines)


def records_of(raw):
    """clean 4-line FASTQ bytes ('\n' line ends) -> [(name, sequence, qualities)]; one-line FASTA records without qualities"""
    lines = raw.split(b"\n")
    out, i = [], 0
    while i < len(lines) and lines[i]:
        if lines[i].startswith(b"@"):
            out.append((lines[i][1:], lines[i + 1], lines[i + 3]))
            i += 4
        else:
            out.append((lines[i][1:], lines[i + 1] if i + 1 < len(lines) else b"", NO_QUAL))
            i += 2
    return out


def mask_records(records, q):
    return [(n, s if c is NO_QUAL else masked(s, c, q), c) for n, s, c in records]


def count_masked(records, q, k):
    """(bases that had a quality, those of them below q) over the records of k bases or more: what the pass reports"""
    kept = [(s, c) for _, s, c in records if c is not NO_QUAL and len(s) >= k]
    return sum(len(s) for s, _ in kept), sum(sum(1 for x in c if x < 33 + q) for _, c in kept)


def text_of(records, k):
    return b"".join(s + b"\n" for _, s, _ in records if len(s) >= k)


# ---------------------------------------------------------------------------------------------- records and writers
def draw_qual(rng, n, low=0.1, q=20):
    """n quality characters, a fraction `low` of them below 33 + q, the bytes 33 + q and 33 + q - 1 among them"""
    out = bytearray()
    for _ in range(n):
        if rng.random() < low:
            out.append(rng.choice((33, 33 + q - 1, rng.randrange(33, 33 + q))))
        else:
            out.append(rng.choice((33 + q, 126, rng.randrange(33 + q, 127))))
    return bytes(out)


def draw_records(rng, count, lengths=(1, 400), alphabet=b"ACGT", low=0.1, q=20, tag=b"r"):
    recs = []
    for i in range(count):
        n = rng.randint(*lengths)
        recs.append((b"%s%d" % (tag, i), bytes(rng.choice(alphabet) for _ in range(n)), draw_qual(rng, n, low, q)))
    return recs


def fastq(records, eol=b"\n", last_eol=True):
    """4-line FASTQ; a record without qualities as one-line FASTA.  Names are padded so that the line table (one line per
    8 raw bytes) holds the chunk, as tests/parse_corpus.py pads them."""
    out = []
    for name, seq, qual in records:
        lines = [b">" + name, seq] if qual is NO_QUAL else [b"@" + name, seq, b"+", qual]
        short = 8 * len(lines) - sum(len(x) + len(eol) for x in lines)
        if short > 0:
            lines[0] += b" " + b"p" * short
        out.append(b"".join(x + eol for x in lines))
    raw = b"".join(out)
    return raw if last_eol or not raw else raw[:-len(eol)]


def fastq_wrapped(records, width):
    """multi-line FASTQ: sequence and qualities wrapped at `width` (qualities at another width: kseq concatenates)"""
    wrap = lambda s, w: b"".join(s[i:i + w] + b"\n" for i in range(0, len(s), w))
    return b"".join(b"@%s\n%s+\n%s" % (n, wrap(s, width), wrap(c, width + 3)) for n, s, c in records if s)


def bam_of(records, flags=None, sizes=(65280,)):
    """-> (the BAM file's bytes, its inflated bytes): the records in order, qualities as Phred bytes (0xFF when absent);
    flags[i] (default 0) as given, so a secondary record can sit among them"""
    body = b""
    for i, (name, seq, qual) in enumerate(records):
        q = None if qual is NO_QUAL else bytes(c - 33 for c in qual)
        body += BAM.record(name, flags[i] if flags else 0, seq, qual=q)
    raw = BAM.header(b"@HD\tVN:1.6\tSO:unknown\n") + body
    return BAM.bgzf(raw, sizes), raw


# ---------------------------------------------------------------------------------------------- the host-only calls
def parse_model_q(lib, raw, k, q):
    cap = len(raw) + 16
    buf = ctypes.create_string_buffer(cap)
    res = _lib.ReadsParseResult()
    rc = lib.ntedit_hip_reads_parse_model_q(raw, len(raw), k, q, buf, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    return res, buf.raw[:res.text_len]


def bam_model_q(lib, raw, min_len, q, at_header=1):
    cap = len(raw) + 1
    buf = ctypes.create_string_buffer(b"\xEE" * (cap + 64), cap + 64)
    res = _lib.ReadsBamResult()
    rc = lib.ntedit_hip_reads_bam_model_q(raw, len(raw), at_header, min_len, q, buf, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    assert buf.raw[cap:] == b"\xEE" * 64
    return res, buf.raw[:res.text_len] if res.clean else b""


def range_text_q(lib, path, q, k=1):
    """the host parser over the whole file under min_qual -> the text of the reads of k bases or more"""
    import os
    u64 = ctypes.c_uint64
    cap = max(4 * os.path.getsize(path), 1 << 16)
    buf = ctypes.create_string_buffer(cap)
    n, reads, start, nxt = u64(), u64(), u64(), u64()
    rc = lib.ntedit_hip_reads_range_text_q(os.fsencode(str(path)), 0, (1 << 64) - 1, q, buf, cap, n, reads, start, nxt)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    text = buf.raw[:n.value]
    return b"".join(r + b"\n" for r in (text[:-1].split(b"\n") if text else []) if len(r) >= k)


def generated(n_files, seed=4321):
    """-> [(records, k)]: small read sets of 1..400 bases, FASTQ records and now and then one without qualities, k such
    that some records are dropped"""
    rng = random.Random(seed)
    out = []
    for _ in range(n_files):
        k = rng.choice((12, 25, 60))
        recs = draw_records(rng, rng.randint(1, 6), alphabet=rng.choice((b"ACGT", b"ACGTN", b"ACGTacgtRYn")),
                            low=rng.choice((0.0, 0.1, 0.5, 1.0)), q=rng.choice(QS))
        recs += draw_records(rng, 2, lengths=(k - 1, k), tag=b"edge")
        out.append((recs, k))
    return out


def pack_cases(cases):
    """the host program's input (tests/min_qual/min_qual_host.cpp): per case kind, k or min_len, min_qual, the bytes"""
    return b"".join(struct.pack("<IIIQ", kind, k, q, len(data)) + data for kind, k, q, data in cases)


def fold(text):
    f = 0
    for b in text:
        f = (f * 31 + b) & 0xFFFFFFFF
    return f
