"""The twin of --min_read_len, --min_mean_qual and --min_rq (CPU and GPU tier alike): the definition written a second time,
in Python integers, and the inputs the tests share.  A filter built WITH the options from a file equals, byte for byte,
the filter built WITHOUT them from the same reads with the dropped reads deleted: `kept` deletes them, `fastq_of` writes
what is left.  The table is recomputed here with `decimal`; an rq is compared as struct-packed float32.

A record is (name, sequence, qualities, rq): qualities as FASTQ characters (Phred+33) or NO_QUAL, rq a float, NO_RQ, or
raw aux bytes (for the aux edge cases)."""
import ctypes
import hashlib
import os
import random
import struct
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import bam_corpus as BAM
import min_qual_twin as MQ
from ntedit_amd import _lib

NO_QUAL = MQ.NO_QUAL
NO_RQ = None
K = 25
TABLE_SHA256 = "cfd0ffe5123fa55f1c535d4a7eac5ffb0a5f1f046d9e6fa4bad58b2e18c8b08f"
LENGTH, RQ, MEAN_QUAL = "dropped_length", "dropped_rq", "dropped_mean_qual"


def table():
    """E[q] = round(2^31 * 10^(-q/10)), q = 0..93, at 60 decimal digits"""
    getcontext().prec = 60
    return [int((Decimal(2) ** 31 * Decimal(10) ** (Decimal(-q) / Decimal(10))).to_integral_value(rounding=ROUND_HALF_EVEN))
            for q in range(94)]


E = table()
assert hashlib.sha256(",".join(map(str, E)).encode()).hexdigest() == TABLE_SHA256


def weight(q):
    return E[min(max(q, 0), 93)]


FASTQ_WEIGHT = [weight(c - 33) for c in range(256)]  # by the FASTQ character (Phred+33)


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_below(x):
    """the float32 next below the float32 x > 0"""
    return struct.unpack("<f", struct.pack("<I", struct.unpack("<I", struct.pack("<f", x))[0] - 1))[0]


def rq_aux(rq):
    return b"" if rq is NO_RQ else rq if isinstance(rq, bytes) else b"rqf" + struct.pack("<f", rq)


def rq_value(rq):
    """the float32 a well-formed aux walk finds, or None; raw aux bytes are the tests' own business (they pass `found`)"""
    return None if rq is NO_RQ or isinstance(rq, bytes) else f32(rq)


def reason(rec, k, L=0, Q=0, R=0.0, found=None):
    """None (kept) or the first rule that drops the record: length, rq, mean quality"""
    _, seq, qual, rq = rec
    if len(seq) < max(L, k):
        return LENGTH
    v = found if isinstance(rq, bytes) else rq_value(rq)
    if R and v is not None and not v >= f32(R):  # (a NaN is dropped)
        return RQ
    if Q and qual is not NO_QUAL and sum(map(FASTQ_WEIGHT.__getitem__, qual)) > len(seq) * E[Q]:
        return MEAN_QUAL
    return None


def kept(recs, k, **f):
    return [r for r in recs if reason(r, k, **f) is None]


def counts(recs, k, **f):
    out = dict(records=len(recs), dropped_length=0, dropped_rq=0, dropped_mean_qual=0)
    for r in recs:
        why = reason(r, k, **f)
        if why:
            out[why] += 1
    return out


def text_of(recs, k, q=0, **f):
    """the batch text: the kept records, masked by --min_qual q"""
    return b"".join((s if c is NO_QUAL or not q else MQ.masked(s, c, q)) + b"\n" for _, s, c, _ in kept(recs, k, **f))


def assert_discriminating(recs, k, reasons, **f):
    """a passing test cannot be one where nothing, or everything, was dropped: the twin drops between 10 % and 90 % of the
    records, and at least one per reason under test"""
    c = counts(recs, k, **f)
    dropped = sum(c[r] for r in (LENGTH, RQ, MEAN_QUAL))
    assert 0.1 * len(recs) <= dropped <= 0.9 * len(recs), c
    for r in reasons:
        assert c[r] >= 1, (r, c)
    return c


def three(recs):
    return [(n, s, c) for n, s, c, _ in recs]


def fastq_of(recs, **kw):
    return MQ.fastq(three(recs), **kw)


def bam_of(recs, flags=None, sizes=(65280,)):
    """-> (the BAM file's bytes, its inflated bytes); qualities as Phred bytes (0xFF when absent), rq as an aux field"""
    body = b""
    for i, (name, seq, qual, rq) in enumerate(recs):
        q = None if qual is NO_QUAL else bytes(c - 33 for c in qual)
        body += BAM.record(name, flags[i] if flags else 0, seq, qual=q, aux=rq_aux(rq))
    raw = BAM.header(b"@HD\tVN:1.6\tSO:unknown\n") + body
    return BAM.bgzf(raw, sizes), raw


# ---------------------------------------------------------------------------------------------- generated reads
def draw_read(rng, name, n, Q, R=0.0, with_rq=False):
    """a read whose quality level lies around Q (a few reads far off, most within 3 of it, bases scattered around the
    level), and whose rq, if any, lies around R"""
    level = Q + rng.choice((-12, -3, -2, -1, 0, 0, 1, 2, 3, 15))
    qual = bytes(33 + min(93, max(0, level + rng.choice((-4, -1, 0, 0, 0, 1, 6)))) for _ in range(n))
    rq = NO_RQ
    if with_rq and rng.random() < 0.85:
        rq = f32(R) if rng.random() < 0.1 else min(1.0, max(0.0, R + rng.uniform(-0.02, 0.01)))
    return (name, bytes(rng.choice(b"ACGT") for _ in range(n)), qual, rq)


def draw_reads(rng, count, Q, R=0.0, with_rq=False, lengths=(1, 400), tag=b"r"):
    return [draw_read(rng, b"%s%d" % (tag, i), rng.randint(*lengths), Q, R, with_rq) for i in range(count)]


def generated(n_files, seed=99):
    """-> [(records, k, L, Q)]: small FASTQ read sets of 1..400 bases, quality levels around Q"""
    rng = random.Random(seed)
    out = []
    for _ in range(n_files):
        k = rng.choice((12, 25, 60))
        Q = rng.choice((1, 7, 10, 20, 30, 60))
        L = rng.choice((0, 0, 40, 150))
        recs = draw_reads(rng, rng.randint(2, 7), Q)
        out.append((recs, k, L, Q))
    return out


# ---------------------------------------------------------------------------------------------- the host-only calls
def stats_dict(st):
    return {name: getattr(st, name) for name, _ in st._fields_}


def parse_model_f(lib, raw, k, q=0, L=0, Q=0):
    cap = len(raw) + 16
    buf = ctypes.create_string_buffer(cap)
    res, st = _lib.ReadsParseResult(), _lib.ReadsReadFilterStats()
    rc = lib.ntedit_hip_reads_parse_model_f(raw, len(raw), k, q, L, Q, 0.0, buf, cap, res, st)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    return res, buf.raw[:res.text_len], stats_dict(st)


def bam_model_f(lib, raw, min_len, q=0, L=0, Q=0, R=0.0, at_header=1):
    cap = len(raw) + 1
    buf = ctypes.create_string_buffer(b"\xEE" * (cap + 64), cap + 64)
    res, st = _lib.ReadsBamResult(), _lib.ReadsReadFilterStats()
    rc = lib.ntedit_hip_reads_bam_model_f(raw, len(raw), at_header, min_len, q, L, Q, R, buf, cap, res, st)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    assert buf.raw[cap:] == b"\xEE" * 64
    return res, buf.raw[:res.text_len] if res.clean else b"", stats_dict(st)


def range_text_f(lib, path, q=0, min_len=0, Q=0):
    """the host parser over the whole file -> (the text, the counts); min_len is the shortest record returned"""
    u64 = ctypes.c_uint64
    cap = max(4 * os.path.getsize(path), 1 << 16)
    buf = ctypes.create_string_buffer(cap)
    n, reads, start, nxt = u64(), u64(), u64(), u64()
    st = _lib.ReadsReadFilterStats()
    rc = lib.ntedit_hip_reads_range_text_f(os.fsencode(str(path)), 0, (1 << 64) - 1, q, min_len, Q, buf, cap, n, reads, start, nxt, st)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    return buf.raw[:n.value], stats_dict(st)


def same_counts(got, want):
    return all(got[name] == want[name] for name in want)


def pack_cases(cases):
    """the host program's input (tests/read_filter/read_filter_host.cpp)"""
    return b"".join(struct.pack("<IIIIIfQ", kind, k, q, L, Q, R, len(data)) + data for kind, k, q, L, Q, R, data in cases)
