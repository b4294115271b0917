"""Inputs of the --gpu_parse tests (CPU and GPU tier alike): the fixed corpus, the seeded generator, and the two host-side
references -- the host parser (ntedit_hip_reads_range_text, the ground truth) and the serial model of the clean grammar
(ntedit_hip_reads_parse_model)."""
import ctypes
import random

from ntedit_amd import _lib

WHOLE = (1 << 64) - 1
KS = (12, 25)


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _wrap(s, w):
    return "".join(s[i:i + w] + "\n" for i in range(0, len(s), w))


def well_formed():
    """name -> bytes: what the clean grammar must accept (and the host parser reads the same way)"""
    rng = random.Random(20261017)
    c = {}
    c["fasta_one_line"] = "".join(">r%d some comment\n%s\n" % (i, _seq(rng, 20 + 7 * i)) for i in range(12))
    for w in (60, 80):
        c["fasta_wrapped_%d" % w] = "".join(">w%d\n%s" % (i, _wrap(_seq(rng, 50 + 37 * i), w)) for i in range(10))
    c["fastq_4_line"] = "".join("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s))
                                for i, s in enumerate(_seq(rng, 15 + 5 * i) for i in range(12)))
    c["fastq_plus_repeats_name"] = "".join("@q%d x\n%s\n+q%d x\n%s\n" % (i, s, i, "F" * len(s))
                                           for i, s in enumerate(_seq(rng, 30 + i) for i in range(6)))
    c["fastq_quality_starts_like_a_record"] = "".join(
        "@q%d\n%s\n+\n%s\n" % (i, s, first + "#" * (len(s) - 1))
        for i, (s, first) in enumerate((_seq(rng, 26 + i), f) for i, f in enumerate("@+>@+>")))
    for k in KS:
        c["fasta_lengths_around_k%d" % k] = "".join(">l%d\n%s\n" % (n, _seq(rng, n)) for n in (k - 1, k, k + 1, k - 1, k))
        c["fastq_lengths_around_k%d" % k] = "".join("@l%d\n%s\n+\n%s\n" % (n, _seq(rng, n), "5" * n)
                                                    for n in (k + 1, k - 1, k, k - 1))
    c["fasta_n_iupac_lower"] = ">a\n%s\n>b\n%s\n" % (_seq(rng, 60, "ACGTNacgtnRYKMSWBDHVryk"), _seq(rng, 45, "acgtN"))
    c["fastq_n_iupac_lower"] = "@a\n%s\n+\n%s\n" % (_seq(rng, 60, "ACGTNacgtnRYKMSW"), "!" * 60)
    c["fasta_no_last_newline"] = ">a\n%s\n>b\n%s" % (_seq(rng, 40), _seq(rng, 33))
    c["fasta_wrapped_no_last_newline"] = (">a\n" + _wrap(_seq(rng, 150), 60))[:-1]
    c["fastq_no_last_newline"] = "@a\n%s\n+\n%s" % (_seq(rng, 40), "I" * 40)
    c["empty_file"] = ""
    c["fasta_one_record"] = ">only\n%s\n" % _seq(rng, 70)
    c["fastq_one_record"] = "@only\n%s\n+\n%s\n" % (_seq(rng, 70), "I" * 70)
    c["fasta_record_without_sequence"] = ">a\n>b\n%s\n>c\n>d\n%s\n>e\n" % (_seq(rng, 30), _seq(rng, 31))
    c["fasta_header_only"] = ">a"
    return {k: v.encode() for k, v in c.items()}


def odd():
    """name -> bytes: what the clean grammar must refuse (kseq reads these by rules the device does not follow)"""
    rng = random.Random(77)
    s = [_seq(rng, 40 + i) for i in range(4)]
    c = {}
    c["crlf_fasta"] = "".join(">r%d\r\n%s\r\n" % (i, x) for i, x in enumerate(s))
    c["crlf_fastq"] = "".join("@r%d\r\n%s\r\n+\r\n%s\r\n" % (i, x, "I" * len(x)) for i, x in enumerate(s))
    c["fastq_wrapped"] = "".join("@r%d\n%s+\n%s" % (i, _wrap(x, 25), _wrap("I" * len(x), 25)) for i, x in enumerate(s))
    c["mixed_fasta_then_fastq"] = ">a\n%s\n@b\n%s\n+\n%s\n" % (s[0], s[1], "I" * len(s[1]))
    c["mixed_fastq_then_fasta"] = "@b\n%s\n+\n%s\n>a\n%s\n" % (s[1], "I" * len(s[1]), s[0])
    c["fasta_sequence_line_starts_with_plus"] = ">a\n%s\n+%s\n" % (s[0], s[1])
    c["fasta_sequence_line_starts_with_at"] = ">a\n%s\n@%s\n" % (s[0], s[1])
    c["fastq_sequence_line_starts_with_at"] = "@a\n@%s\n+\n%s\n" % (s[0], "I" * (len(s[0]) + 1))
    c["fastq_sequence_line_starts_with_plus"] = "@a\n+%s\n+\n%s\n" % (s[0], "I" * (len(s[0]) + 1))
    c["fastq_quality_one_short"] = "@a\n%s\n+\n%s\n@b\n%s\n+\n%s\n" % (s[0], "I" * (len(s[0]) - 1), s[1], "I" * len(s[1]))
    c["fastq_quality_one_long"] = "@a\n%s\n+\n%s\n@b\n%s\n+\n%s\n" % (s[0], "I" * (len(s[0]) + 1), s[1], "I" * len(s[1]))
    c["junk_before_the_first_record_fasta"] = "junk line\n>a\n%s\n" % s[0]
    c["junk_before_the_first_record_fastq"] = "\n\n@a\n%s\n+\n%s\n" % (s[0], "I" * len(s[0]))
    c["plus_line_at_the_end_without_newline"] = "@a\n%s\n+\n%s\n@b\n%s\n+" % (s[0], "I" * len(s[0]), s[1])
    return {k: v.encode() for k, v in c.items()}


SEQ_ALPHABETS = ("ACGT", "ACGT", "ACGTN", "ACGTacgtNn", "ACGTRYKMSWBDHVN")
QUAL = "".join(chr(c) for c in range(33, 127))


def generated(n_cases, seed=1234):
    """-> [(raw bytes, k, mutated)]: small files from the grammar -- only what well_formed() covers --, every second one
    with one random mutation: a byte set to one of \\r \\n > @ +, a line deleted, or a line duplicated"""
    rng = random.Random(seed)
    out = []
    for case in range(n_cases):
        k = rng.choice(KS)
        alphabet = rng.choice(SEQ_ALPHABETS)
        fastq = rng.random() < 0.5
        recs = rng.randint(1, 8)
        parts = []
        for i in range(recs):
            n = rng.choice((k - 1, k, k + 1, rng.randint(1, 3 * k), rng.randint(1, 200)))
            if not fastq and rng.random() < 0.1:
                n = 0
            s = _seq(rng, n, alphabet)
            name = "r%d%s" % (i, rng.choice(("", " c", "/1 x=@y", "\tz")))
            if fastq:
                q = "".join(rng.choice(QUAL) for _ in range(n))
                rec = ["@" + name, s, "+" + rng.choice(("", name)), q]
            else:
                w = rng.choice((n or 1, 60, 80, rng.randint(1, 30)))
                rec = [">" + name] + [s[j:j + w] for j in range(0, n, w)]
            # the line table holds one line per 8 raw bytes: a longer name keeps the record within it
            short = 8 * len(rec) - sum(len(x) + 1 for x in rec)
            if short > 0:
                rec[0] += " " + "p" * short
            parts.append("".join(x + "\n" for x in rec))
        raw = "".join(parts)
        if rng.random() < 0.3 and raw.endswith("\n"):
            raw = raw[:-1]
        raw = raw.encode()
        mutated = case % 2 == 1
        if mutated and raw:
            what = rng.randrange(3)
            if what == 0:
                at = rng.randrange(len(raw))
                raw = raw[:at] + rng.choice(b"\r\n>@+").to_bytes(1, "little") + raw[at + 1:]
            else:
                lines = raw.split(b"\n")
                at = rng.randrange(len(lines))
                lines = lines[:at] + ([] if what == 1 else [lines[at]] * 2) + lines[at + 1:]
                raw = b"\n".join(lines)
        out.append((raw, k, mutated))
    return out


def host_text(lib, path, k):
    """the host parser over the whole file -> (text of the reads of k bases or more, reads, bases): what a pass feeds"""
    u64 = ctypes.c_uint64
    import os
    cap = os.path.getsize(path) + 16
    buf = ctypes.create_string_buffer(cap)
    n, reads, start, nxt = u64(), u64(), u64(), u64()
    rc = lib.ntedit_hip_reads_range_text(os.fsencode(path), 0, WHOLE, buf, cap, n, reads, start, nxt)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    text = buf.raw[:n.value]
    records = text[:-1].split(b"\n") if text else []
    assert len(records) == reads.value
    kept = [r for r in records if len(r) >= k]
    return b"".join(r + b"\n" for r in kept), len(kept), sum(len(r) for r in kept)


def model(lib, raw, k):
    """the serial model -> (ReadsParseResult, text)"""
    cap = len(raw) + 16
    buf = ctypes.create_string_buffer(cap)
    res = _lib.ReadsParseResult()
    rc = lib.ntedit_hip_reads_parse_model(raw, len(raw), k, buf, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    return res, buf.raw[:res.text_len]
