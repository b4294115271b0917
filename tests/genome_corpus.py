"""Inputs of the genome --gpu_parse tests (CPU and GPU tier alike): the fixed corpus, the seeded generator, the serial
model of the stateful genome grammar (ntedit_hip_genome_parse_model) over one chunk or over a cutting of a file, and the
split rule that ties its text to the host parser (ntedit_hip_reads_range_text, the ground truth)."""
import ctypes
import random

import parse_corpus as PC
from ntedit_amd import _lib

LINE_START, IN_HEADER, IN_SEQ = _lib.GENOME_LINE_START, _lib.GENOME_IN_HEADER, _lib.GENOME_IN_SEQ
STATES = (LINE_START, IN_HEADER, IN_SEQ)
NO_START = _lib.READS_NO_START
TABLE = _lib.PARSE_BAD["table"]
KS = (12, 25)


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _wrap(s, w):
    return "".join(s[i:i + w] + "\n" for i in range(0, len(s), w))


def well_formed():
    """name -> bytes: genome FASTA the grammar must accept whole (and the host parser reads the same way)"""
    rng = random.Random(20261018)
    c = {}
    c["wrapped_60"] = "".join(">chr%d assembled\n%s" % (i, _wrap(_seq(rng, 400 + 173 * i), 60)) for i in range(5))
    # one line per base: the header is long enough to keep the file within one line per 8 bytes
    c["wrapped_1"] = ">one_base_per_line " + "p" * 2400 + "\n" + _wrap(_seq(rng, 300), 1)
    c["unwrapped"] = "".join(">ctg%d\n%s\n" % (i, _seq(rng, 900 + 411 * i)) for i in range(4))
    c["header_of_20_kb"] = ">long " + "h" * 20000 + "\n" + _wrap(_seq(rng, 500), 60) + ">next\n" + _seq(rng, 70) + "\n"
    c["records_shorter_than_k"] = "".join(">s%d\n%s\n" % (n, _seq(rng, n)) for n in (1, 11, 12, 13, 24, 25, 26, 3, 200, 5))
    c["lower_case_and_n_runs"] = ">a\n%s>b\n%s\n" % (
        _wrap(_seq(rng, 200, "acgt") + "N" * 130 + _seq(rng, 150) + "n" * 40 + _seq(rng, 99, "ACGTacgtRYKM"), 60),
        "N" * 50 + _seq(rng, 80) + "N" * 50)
    c["last_line_without_newline"] = (">a\n" + _wrap(_seq(rng, 150), 60) + ">b\n" + _wrap(_seq(rng, 100), 60))[:-1]
    c["record_without_sequence"] = ">a\n>b\n%s\n>c\n>d\n%s\n>e\n" % (_seq(rng, 30), _seq(rng, 31))
    c["header_only_without_newline"] = ">a"
    c["empty_file"] = ""
    return {k: v.encode() for k, v in c.items()}


def odd():
    """name -> bytes: what the grammar must refuse"""
    rng = random.Random(78)
    s = [_seq(rng, 50 + i) for i in range(4)]
    c = {}
    c["crlf"] = "".join(">r%d\r\n%s\r\n" % (i, x) for i, x in enumerate(s))
    c["an_empty_line"] = ">a\n%s\n\n%s\n>b\n%s\n" % (s[0], s[1], s[2])
    c["an_empty_line_at_the_end"] = ">a\n%s\n\n" % s[0]
    c["a_line_starting_with_at"] = ">a\n%s\n@%s\n" % (s[0], s[1])
    c["a_line_starting_with_plus"] = ">a\n%s\n+%s\n" % (s[0], s[1])
    c["a_fastq_file"] = "".join("@q%d\n%s\n+\n%s\n" % (i, x, "I" * len(x)) for i, x in enumerate(s))
    c["junk_before_the_first_record"] = "junk line\n>a\n%s\n" % s[0]
    c["wrapped_1_over_the_line_bound"] = ">w\n" + _wrap(s[0], 1)
    return {k: v.encode() for k, v in c.items()}


SEQ_ALPHABETS = ("ACGT", "ACGT", "ACGTN", "ACGTacgtNn", "ACGTRYKMSWBDHVN")


def generated(n_cases, seed=4321, size=None):
    """-> [(raw bytes, k, mutated)]: small FASTA files from the grammar, every second one with one random mutation: a byte
    set to one of \\r \\n > @ +, a line deleted, or a line duplicated"""
    rng = random.Random(seed)
    out = []
    for case in range(n_cases):
        k = rng.choice(KS)
        alphabet = rng.choice(SEQ_ALPHABETS)
        parts = []
        for i in range(rng.randint(1, 6)):
            n = rng.choice((k - 1, k, k + 1, rng.randint(1, 3 * k), rng.randint(1, 300)))
            if rng.random() < 0.1:
                n = 0
            s = _seq(rng, n, alphabet)
            w = rng.choice((n or 1, 60, 80, rng.randint(1, 30)))
            rec = [">c%d%s" % (i, rng.choice(("", " c", "/1 x=@y", "\tz")))] + [s[j:j + w] for j in range(0, n, w)]
            # the grammar holds one line per 8 raw bytes: a longer name keeps the record within it
            short = 8 * len(rec) - sum(len(x) + 1 for x in rec)
            if short > 0:
                rec[0] += " " + "p" * short
            parts.append("".join(x + "\n" for x in rec))
        raw = "".join(parts)
        if rng.random() < 0.3:
            raw = raw[:-1]
        raw = raw.encode()
        mutated = case % 2 == 1
        if mutated:
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


def model(lib, raw, state=LINE_START, first_chunk=True):
    """the serial model over one chunk -> (GenomeParseResult, text)"""
    cap = len(raw) + 16
    buf = ctypes.create_string_buffer(cap)
    res = _lib.GenomeParseResult()
    rc = lib.ntedit_hip_genome_parse_model(raw, len(raw), state, int(first_chunk), buf, cap, res)
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    return res, buf.raw[:res.text_len]


def fields(res):
    return (res.clean, res.broken, res.state_out, res.text_len, res.bases, res.lines, res.last_header)


def run_chunks(parse, raw, cuts):
    """raw cut at `cuts` (ascending offsets), each chunk through parse(chunk, state, first_chunk) -> (res, text) and
    entered with its predecessor's exit state -> dict(text, bases, last_header as a file offset, state, broken: the
    OR over the chunks)"""
    edges = [0] + list(cuts) + [len(raw)]
    text, bases, last_header, state, broken = [], 0, NO_START, LINE_START, 0
    for a, b in zip(edges, edges[1:]):
        res, t = parse(raw[a:b], state, a == 0)
        text.append(t)
        bases += res.bases
        broken |= res.broken
        if res.last_header != NO_START:
            last_header = a + res.last_header
        state = res.state_out
    return dict(text=b"".join(text), bases=bases, last_header=last_header, state=state, broken=broken)


def records_of_text(text, k):
    """the split rule: the pieces of k bytes or more between the text's '\\n', in order"""
    return [p for p in text.split(b"\n") if len(p) >= k]


def host_records(lib, path, k):
    """the host parser's reads of k bases or more, in order, and the bases of all records"""
    text, _, _ = PC.host_text(lib, path, k)
    _, _, all_bases = PC.host_text(lib, path, 1)
    return (text[:-1].split(b"\n") if text else []), all_bases
