"""--min_read_len, --min_mean_qual and --min_rq on the CPU tier: the table against `decimal`; each rule at its boundary; the
aux walk's edge cases; the two serial models and the host parser against the twin of tests/read_filter_twin.py (the same
reads with the dropped ones deleted, read without the options); off means unchanged; every refusal through the rules in
both dialects and through the front ends without a device; and the models and the filtering FastaReader as a host program
of their own under AddressSanitizer and UBSan."""
import ctypes
import gzip
import hashlib
import os
import random
import re
import struct
import subprocess
import sys

import pytest

import bam_corpus as BAM
import helpers as H
import min_qual_twin as MQ
import parse_corpus as PC
import read_filter_twin as RF
from ntedit_amd import _lib

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
HOST_SRC = os.path.join(H.ROOT, "tests", "read_filter", "read_filter_host.cpp")
GRAMMAR = os.path.join(H.ROOT, "ntedit_amd", "csrc", "nte_reads_grammar.h")
NO_DEVICE = "no usable HIP device"
SEQ = b"ACGTTGCAACGTAGCTAGCTAGGATCCATGCA" * 4  # 128 bases


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------- the table
def test_the_table_is_the_one_decimal_computes():
    text = open(GRAMMAR).read()
    body = re.search(r"RP_QUAL_WEIGHT\[94\] = \{(.*?)\};", text, re.S).group(1)
    values = [int(x) for x in re.findall(r"(\d+)u", body)]
    assert values == RF.E and len(values) == 94
    assert hashlib.sha256(",".join(map(str, values)).encode()).hexdigest() == RF.TABLE_SHA256
    samples = {0: 2147483648, 1: 1705806895, 7: 428479319, 10: 214748365, 20: 21474836, 30: 2147484, 40: 214748, 60: 2147,
               92: 1, 93: 1}
    assert all(values[q] == v for q, v in samples.items())
    assert "pow(" not in text  # a list of literals: no pow at run time


def one(seq, qual, rq=RF.NO_RQ, name=b"b"):
    return [(name, seq, qual, rq)]


def all_three(lib, recs, k, tmp_path, q=0, L=0, Q=0):
    """the text model, the BAM model and the host parser on the same records -> their texts and counts"""
    raw = RF.fastq_of(recs)
    (tmp_path / "b.fq").write_bytes(raw)
    _, t0, s0 = RF.parse_model_f(lib, raw, k, q, L, Q)
    _, t1, s1 = RF.bam_model_f(lib, RF.bam_of(recs)[1], k, q, L, Q)
    t2, s2 = RF.range_text_f(lib, tmp_path / "b.fq", q, max(L, k), Q)
    return (t0, t1, t2), (s0, s1, s2)


# ---------------------------------------------------------------------------------- --min_mean_qual at its boundary
@pytest.mark.parametrize("Q", [1, 7, 20, 60])
def test_the_boundary_of_the_mean_quality(lib, Q, tmp_path):
    """a read whose bases all have quality Q is kept; the same read with one base at Q - 1 is dropped"""
    at_q = bytes([33 + Q]) * len(SEQ)
    below = at_q[:40] + bytes([33 + Q - 1]) + at_q[41:]
    for qual, want in ((at_q, SEQ + b"\n"), (below, b"")):
        assert RF.reason(one(SEQ, qual)[0], 12, Q=Q) == (None if want else RF.MEAN_QUAL)
        texts, stats = all_three(lib, one(SEQ, qual), 12, tmp_path, Q=Q)
        assert texts == (want, want, want), (Q, texts)
        for st in stats:
            assert (st["records"], st["dropped_mean_qual"], st["dropped_length"]) == (1, 0 if want else 1, 0)


def test_every_q_at_its_boundary_in_the_text_model(lib):
    for Q in range(1, 61):
        at_q = bytes([33 + Q]) * len(SEQ)
        raw = RF.fastq_of(one(SEQ, at_q) + one(SEQ, at_q[:-1] + bytes([33 + Q - 1]), name=b"c"))
        _, text, st = RF.parse_model_f(lib, raw, 12, Q=Q)
        assert text == SEQ + b"\n" and st["dropped_mean_qual"] == 1, Q


def test_quality_bytes_are_clamped(lib, tmp_path):
    """a FASTQ byte below 33 counts as quality 0, a quality above 93 as 93: decisions that differ from any other reading"""
    # Q = 1 on two bases: (byte 32, Phred 5) is kept with the byte at quality 0, (byte 32, byte 33) is dropped
    for qual, kept in ((bytes([32, 38]), True), (bytes([32, 33]), False), (bytes([11, 38]), True), (bytes([1, 33]), False)):
        raw = b"@c padding padding padding\nAC\n+\n" + qual + b"\n"
        (tmp_path / "c.fq").write_bytes(raw)
        want = b"AC\n" if kept else b""
        assert RF.reason((b"c", b"AC", qual, None), 1, Q=1) == (None if kept else RF.MEAN_QUAL)
        assert RF.parse_model_f(lib, raw, 1, Q=1)[1] == want
        assert RF.range_text_f(lib, tmp_path / "c.fq", 0, 1, 1)[0] == want
    # qualities above 93 weigh what 93 weighs, in FASTQ (bytes 127 .. 255) and in BAM (94 .. 254): one base at quality 0
    # among n - 1 such bases is kept at Q = 60 iff E[0] + (n - 1) * E[93] <= n * E[60]
    n = RF.E[0] // (RF.E[60] - 1) + 2
    for high in (127, 200, 255):
        for length, kept in ((n, True), (n - 3, False)):
            seq, qual = b"A" * length, bytes([33]) + bytes([high]) * (length - 1)
            assert RF.reason((b"h", seq, qual, None), 1, Q=60) == (None if kept else RF.MEAN_QUAL)
            want = seq + b"\n" if kept else b""
            assert RF.parse_model_f(lib, RF.fastq_of(one(seq, qual)), 1, Q=60)[1] == want
            body = BAM.record(b"h", 0, seq, qual=bytes([0]) + bytes([min(high - 33, 254)]) * (length - 1))
            assert RF.bam_model_f(lib, BAM.header() + body, 1, Q=60)[1] == want


# ---------------------------------------------------------------------------------- --min_rq at its boundary, and the aux walk
def bam_one(lib, aux, R=0.99, seq=SEQ, Q=0, qual=None):
    raw = BAM.header() + BAM.record(b"r", 0, seq, qual=qual, aux=aux)
    res, text, st = RF.bam_model_f(lib, raw, 12, Q=Q, R=R)
    assert res.clean == 1 and st["records"] == 1
    return text, st


def test_the_boundary_of_rq(lib):
    """an rq equal to R is kept, one float below R is dropped; two IEEE floats compare, and a NaN is dropped"""
    for R in (0.99, 0.5, 1.0, 1e-30):
        at = RF.f32(R)
        text, st = bam_one(lib, b"rqf" + struct.pack("<f", at), R)
        assert text == SEQ + b"\n" and (st["rq_tagged"], st["dropped_rq"]) == (1, 0), R
        text, st = bam_one(lib, b"rqf" + struct.pack("<f", RF.f32_below(at)), R)
        assert text == b"" and (st["rq_tagged"], st["dropped_rq"]) == (1, 1), R
    for nan in (b"\x00\x00\xc0\x7f", b"\x01\x00\x80\x7f", b"\x00\x00\xc0\xff"):
        text, st = bam_one(lib, b"rqf" + nan)
        assert text == b"" and st["dropped_rq"] == 1
    text, st = bam_one(lib, b"rqf" + struct.pack("<f", float("inf")))
    assert text == SEQ + b"\n"
    text, st = bam_one(lib, b"")  # no tag: the record passes
    assert text == SEQ + b"\n" and (st["rq_tagged"], st["dropped_rq"], st["aux_malformed"]) == (0, 0, 0)


def test_rq_of_another_type_and_behind_every_aux_type(lib):
    low = struct.pack("<f", 0.5)
    for other in (b"rqZ0.5\0", b"rqi" + struct.pack("<i", 0), b"rqC\0", b"rqBf" + struct.pack("<i", 1) + low):
        text, st = bam_one(lib, other)  # not an rq:f field: no tag
        assert text == SEQ + b"\n" and (st["rq_tagged"], st["aux_malformed"]) == (0, 0), other
        text, st = bam_one(lib, other + b"rqf" + low)  # ... and walked past to the one that is
        assert text == b"" and (st["rq_tagged"], st["dropped_rq"]) == (1, 1), other
    text, st = bam_one(lib, BAM.all_aux() + b"rqf" + low)
    assert text == b"" and (st["rq_tagged"], st["dropped_rq"], st["aux_malformed"]) == (1, 1, 0)
    text, st = bam_one(lib, BAM.all_aux() + b"rqf" + struct.pack("<f", 0.999))
    assert text == SEQ + b"\n" and st["rq_tagged"] == 1
    text, st = bam_one(lib, b"rqf" + low + BAM.all_aux())
    assert text == b"" and st["dropped_rq"] == 1
    # the kinetics arrays of a PacBio record are skipped by their counts
    text, st = bam_one(lib, b"ipBC" + struct.pack("<i", 5000) + bytes(5000) + b"rqf" + low)
    assert text == b"" and st["dropped_rq"] == 1


def test_a_truncated_or_unknown_aux_field_ends_the_walk(lib):
    low = b"rqf" + struct.pack("<f", 0.5)
    broken = [b"rq", b"rqf", b"rqf\0\0\0", b"XZZno nul", b"XiI\1\2", b"XbBC" + struct.pack("<i", 9) + b"12345678", b"XbBC\1",
              b"XbBx" + struct.pack("<i", 1) + b"\0", b"XbBA" + struct.pack("<i", 1) + b"\0", b"Xq?\0\0\0\0",
              b"XbBi" + struct.pack("<I", 0xFFFFFFFF) + b"\0\0\0\0"]
    for aux in broken:
        # the record counts as having no tag, and as aux_malformed -- also when an rq:f field follows the broken one
        for tail in (b"", low) if not aux.startswith(b"rq") else (b"",):
            text, st = bam_one(lib, aux + tail)
            assert text == SEQ + b"\n" and (st["rq_tagged"], st["dropped_rq"], st["aux_malformed"]) == (0, 0, 1), aux
    # without --min_rq nothing is walked and nothing counted; an rq in front of the broken field is found first
    raw = BAM.header() + BAM.record(b"r", 0, SEQ, aux=b"XZZno nul")
    assert RF.bam_model_f(lib, raw, 12, L=20)[2]["aux_malformed"] == 0
    text, st = bam_one(lib, low + b"XZZno nul")
    assert text == b"" and (st["dropped_rq"], st["aux_malformed"]) == (1, 0)
    # the walk ends with the record: a second record's bytes are never an aux field of the first
    two = BAM.header() + BAM.record(b"r", 0, SEQ, aux=b"XZZabc") + BAM.record(b"rqf", 0, SEQ, aux=low)
    res, text, st = RF.bam_model_f(lib, two, 12, R=0.99)
    assert text == SEQ + b"\n" and (st["records"], st["dropped_rq"], st["aux_malformed"], st["rq_tagged"]) == (2, 1, 1, 1)


def test_a_record_that_fails_two_rules_is_counted_once_under_the_first(lib, tmp_path):
    low_q = bytes([33 + 2]) * 20
    short_low = (b"a", SEQ[:20], low_q, 0.5)           # length, rq and mean quality all fail: length
    long_low_rq = (b"b", SEQ, bytes([35]) * 128, 0.5)  # rq and mean quality fail: rq
    long_low_q = (b"c", SEQ, bytes([35]) * 128, 0.999)
    fine = (b"d", SEQ, bytes([73]) * 128, 0.999)
    secondary = (b"e", SEQ[:20], low_q, 0.5)           # the flag comes first, and is in no count here
    recs = [short_low, long_low_rq, long_low_q, fine, secondary]
    _, raw = RF.bam_of(recs, flags=[0, 0, 0, 0, 0x100])
    res, text, st = RF.bam_model_f(lib, raw, 12, L=50, Q=20, R=0.99)
    assert text == SEQ + b"\n" and res.skipped_flag == 1 and res.skipped_short == 1 and res.kept == 1 and res.records == 5
    assert st == dict(records=4, dropped_length=1, dropped_rq=1, dropped_mean_qual=1, rq_tagged=3, aux_malformed=0)  # (the short one is not looked into)
    assert RF.counts(recs[:4], 12, L=50, Q=20, R=0.99) == {k: st[k] for k in ("records", RF.LENGTH, RF.RQ, RF.MEAN_QUAL)}
    raw = RF.fastq_of(recs[:4])
    _, text, st = RF.parse_model_f(lib, raw, 12, L=50, Q=20)
    assert text == SEQ + b"\n" and (st["records"], st["dropped_length"], st["dropped_mean_qual"]) == (4, 1, 2)
    (tmp_path / "t.fq").write_bytes(raw)
    text, st = RF.range_text_f(lib, tmp_path / "t.fq", 0, 50, 20)
    assert text == SEQ + b"\n" and (st["records"], st["dropped_length"], st["dropped_mean_qual"]) == (4, 1, 2)


def test_min_read_len_is_the_larger_of_l_and_k(lib):
    recs = [(b"r%d" % n, SEQ[:n], bytes([70]) * n, None) for n in (11, 12, 29, 30, 31, 128)]
    raw, braw = RF.fastq_of(recs), RF.bam_of(recs)[1]
    for k, L in ((12, 30), (30, 12), (12, 1), (31, 31)):
        want = RF.text_of(recs, k, L=L)
        assert want == b"".join(s + b"\n" for _, s, _, _ in recs if len(s) >= max(k, L))
        assert RF.parse_model_f(lib, raw, k, L=L)[1] == want and RF.bam_model_f(lib, braw, k, L=L)[1] == want
        st = RF.parse_model_f(lib, raw, k, L=L)[2]
        assert st["dropped_length"] == sum(1 for _, s, _, _ in recs if len(s) < max(k, L))


def test_min_qual_masks_the_kept_reads_and_the_mean_is_over_the_stored_qualities(lib, tmp_path):
    rng = random.Random(8)
    recs = RF.draw_reads(rng, 60, 15)
    RF.assert_discriminating(recs, 25, [RF.MEAN_QUAL], Q=15)
    want = RF.text_of(recs, 25, q=20, Q=15)
    assert b"N" in want and want != RF.text_of(recs, 25, Q=15)
    texts, _ = all_three(lib, recs, 25, tmp_path, q=20, Q=15)
    assert texts == (want, want, want)


# ---------------------------------------------------------------------------------- the models and the host parser against the twin
def test_the_models_equal_the_twin_on_the_fixed_corpora(lib, tmp_path):
    changed = 0
    for name, raw in sorted(PC.well_formed().items()):
        recs = [(n, s, c, None) for n, s, c in MQ.records_of(raw)] if raw[:1] == b"@" else None
        (tmp_path / "f.txt").write_bytes(raw)
        for k in PC.KS:
            for L, Q in ((0, 30), (40, 0), (40, 41), (0, 60), (0, 1)):
                res, text, st = RF.parse_model_f(lib, raw, k, L=L, Q=Q)
                host, hst = RF.range_text_f(lib, tmp_path / "f.txt", 0, max(L, k), Q)
                assert res.clean == 1 and text == host and RF.same_counts(hst, {n: st[n] for n in ("records", RF.LENGTH, RF.MEAN_QUAL)})
                if recs is not None:
                    assert text == RF.text_of(recs, k, L=L, Q=Q), (name, k, L, Q)
                    assert RF.same_counts(st, RF.counts(recs, k, L=L, Q=Q)), (name, k, L, Q)
                    # the twin file: the kept reads, read without the options
                    assert text == PC.model(lib, RF.fastq_of(RF.kept(recs, k, L=L, Q=Q)), k)[1]
                else:  # a FASTA input has no qualities: the length rule alone
                    assert text == PC.model(lib, raw, max(L, k))[1]
                changed += text != PC.model(lib, raw, k)[1]
    assert changed > 20
    for case in BAM.corpus():
        for L in (0, 120, 151):
            res, text, st = RF.bam_model_f(lib, case.raw, BAM.K, L=L, R=0.99)  # (no record has an rq; every aux field is walked)
            primary = [(n, s, None, None) for n, f, s in case.reads if not f & 0x900]
            assert res.clean == 1 and text == RF.text_of(primary, BAM.K, L=L), (case.name, L)
            assert RF.same_counts(st, RF.counts(primary, BAM.K, L=L)) and st["aux_malformed"] == 0, case.name
            assert text == BAM.model(lib, case.raw, 1, max(L, BAM.K))[2]


def test_the_models_and_the_host_parser_equal_the_twin_on_generated_files(lib, tmp_path):
    total = dict(records=0, dropped_length=0, dropped_rq=0, dropped_mean_qual=0)
    for i, (recs, k, L, Q) in enumerate(RF.generated(300)):
        raw = RF.fastq_of(recs, last_eol=i % 3 != 0)
        want, c = RF.text_of(recs, k, L=L, Q=Q), RF.counts(recs, k, L=L, Q=Q)
        res, text, st = RF.parse_model_f(lib, raw, k, L=L, Q=Q)
        assert res.clean == 1 and text == want and RF.same_counts(st, c), i
        assert (res.reads, res.bases) == (want.count(b"\n"), len(want) - want.count(b"\n"))
        path, twin = tmp_path / "g.fq", tmp_path / "g_twin.fq"
        path.write_bytes(raw)
        twin.write_bytes(RF.fastq_of(RF.kept(recs, k, L=L, Q=Q)))
        host, hst = RF.range_text_f(lib, path, 0, max(L, k), Q)
        assert host == want and RF.same_counts(hst, c), i
        assert RF.range_text_f(lib, twin, 0, 0, 0)[0] == want  # the kept reads, read without the options
        assert RF.bam_model_f(lib, RF.bam_of(recs)[1], k, L=L, Q=Q)[1] == want, i
        for name in total:
            total[name] += c[name]
    dropped = total[RF.LENGTH] + total[RF.MEAN_QUAL]
    assert 0.1 * total["records"] <= dropped <= 0.9 * total["records"] and total[RF.LENGTH] > 50 and total[RF.MEAN_QUAL] > 50, total


def test_the_bam_model_equals_the_twin_with_all_three_rules(lib):
    rng = random.Random(21)
    recs = RF.draw_reads(rng, 200, 20, R=0.99, with_rq=True, lengths=(10, 300))
    recs.insert(5, (b"absent", SEQ, RF.NO_QUAL, 0.999))
    recs.insert(9, (b"secondary", SEQ, bytes([34]) * 128, 0.1))
    flags = [0x100 if n == b"secondary" else 0 for n, _, _, _ in recs]
    primary = [r for r, f in zip(recs, flags) if not f]
    f = dict(L=60, Q=20, R=0.99)
    c = RF.assert_discriminating(primary, 25, [RF.LENGTH, RF.RQ, RF.MEAN_QUAL], **f)
    res, text, st = RF.bam_model_f(lib, RF.bam_of(recs, flags)[1], 25, **f)
    assert res.clean == 1 and res.skipped_flag == 1 and text == RF.text_of(primary, 25, **f) and RF.same_counts(st, c)
    assert st["rq_tagged"] == sum(1 for r in primary if r[3] is not None and len(r[1]) >= 60) and SEQ + b"\n" in text
    # the twin file: the kept reads as FASTQ, through the text model without the options
    assert text == PC.model(lib, RF.fastq_of([(n, s, b"~" * len(s) if q is None else q, r) for n, s, q, r in RF.kept(primary, 25, **f)]), 25)[1]


def test_the_host_parser_on_the_shapes_the_device_hands_back(lib, tmp_path):
    """multi-line FASTQ (concatenated first), CR LF line ends, a single-stream .gz, a FASTA record between FASTQ records"""
    rng = random.Random(5)
    recs = RF.draw_reads(rng, 60, 20)
    c = RF.assert_discriminating(recs, 25, [RF.LENGTH, RF.MEAN_QUAL], L=60, Q=20)
    want = RF.text_of(recs, 25, L=60, Q=20)
    three = RF.three(recs)
    shapes = {"wrapped_60.fq": MQ.fastq_wrapped(three, 60), "wrapped_7.fq": MQ.fastq_wrapped(three, 7),
              "crlf.fq": MQ.fastq(three, eol=b"\r\n"), "plain.fq": MQ.fastq(three),
              "single_stream.fq.gz": gzip.compress(MQ.fastq(three))}
    for name, data in shapes.items():
        (tmp_path / name).write_bytes(data)
        text, st = RF.range_text_f(lib, tmp_path / name, 0, 60, 20)
        assert text == want and RF.same_counts(st, c), name
    mixed = recs[:5] + [(b"fa", b"ACGTNACGT" * 9, RF.NO_QUAL, None)] + recs[5:9]
    (tmp_path / "mixed.fq").write_bytes(RF.fastq_of(mixed))
    assert RF.range_text_f(lib, tmp_path / "mixed.fq", 0, 25, 20)[0] == RF.text_of(mixed, 25, Q=20)
    assert b"ACGTNACGT" * 9 + b"\n" in RF.text_of(mixed, 25, Q=20)


# ---------------------------------------------------------------------------------- off means unchanged
def test_zero_and_the_old_entry_points_are_the_text_without_the_options(lib, tmp_path):
    zero = dict(records=0, dropped_length=0, dropped_rq=0, dropped_mean_qual=0, rq_tagged=0, aux_malformed=0)
    for name, raw in sorted(PC.well_formed().items()):
        for q in (0, 20):
            res, text = MQ.parse_model_q(lib, raw, 12, q)
            res0, text0, st = RF.parse_model_f(lib, raw, 12, q)
            assert text == text0 and (res.clean, res.reads, res.bases) == (res0.clean, res0.reads, res0.bases) and st == zero, name
            (tmp_path / "x.txt").write_bytes(raw)
            text, st = RF.range_text_f(lib, tmp_path / "x.txt", q)
            nonempty = b"".join(r + b"\n" for r in text.split(b"\n") if r)  # (range_text_q leaves the empty reads out)
            assert MQ.range_text_q(lib, tmp_path / "x.txt", q) == nonempty and st == zero
    for case in BAM.corpus()[:6]:
        res, text, st = RF.bam_model_f(lib, case.raw, BAM.K)
        assert text == BAM.model(lib, case.raw, 1, BAM.K)[2] and st == zero
    res = _lib.ReadsParseResult()
    for bad in ((1 << 31, 0, 0.0), (0, 61, 0.0), (0, 0, 1.5), (0, 0, -0.5), (0, 0, float("nan"))):
        assert lib.ntedit_hip_reads_parse_model_f(b"@a\nA\n+\nI\n", 9, 1, 0, bad[0], bad[1], bad[2], None, 0, res, None) == _lib.E_ARG
    # a minimum rq that is not above 0 is off, the negative zero included: nothing is walked, nothing counted
    raw = BAM.header() + BAM.record(b"r", 0, SEQ, aux=b"rqf" + struct.pack("<f", float("nan")) + b"XZZno nul")
    for off in (0.0, -0.0):
        _, text, st = RF.bam_model_f(lib, raw, 12, R=off)
        assert text == SEQ + b"\n" and st == zero
    assert lib.ntedit_hip_reads_set_read_filter(None, 1, 1, 0.5) == _lib.E_ARG
    assert lib.ntedit_hip_reads_read_filter_info(None, None) == _lib.E_ARG


def test_the_build_id_does_not_move(lib):
    """everything the options touch lies outside the sources the build id is made of"""
    text = open(os.path.join(H.ROOT, "ntedit_amd", "csrc", "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:?=(.*(?:\\\n.*)*)", text, re.M).group(1)
    for unit in ("nte_reads_parse", "nte_reads_bam", "nte_reads_grammar", "nte_bam_grammar", "nte_reads_model"):
        assert unit not in ksrc


# ---------------------------------------------------------------------------------- refusals
def check(lib, dialect, given, final=1):
    o = _lib.ReadsFilterOptions(**{name: text.encode() for name, text in given.items()})
    r = _lib.ReadsFilterRules()
    rc = lib.ntedit_hip_reads_filter_options_check(o, dialect, final, r)
    return rc, lib.ntedit_hip_reads_last_error(None).decode() if rc else "", r


RANGES = {"min_read_len": ("the minimum read length must be between 1 and 2147483647", ("1", "150", "2147483647"),
                           ("0", "2147483648", "99999999999")),
          "min_mean_qual": ("the minimum mean read quality must be between 1 and 60", ("1", "7", "60"), ("0", "61", "93")),
          "min_rq": ("the minimum read accuracy must be above 0 and at most 1", ("0.99", "1", "1.0", "1e-3", ".5"),
                     ("0", "0.0", "1.0001", "2", "1e-50"))}


def test_the_rules_refuse_in_both_dialects(lib):
    for dialect, dot in ((_lib.READS_DIALECT_TOOL, "."), (_lib.READS_DIALECT_POLISHER, "")):
        rc, _, r = check(lib, dialect, {})
        assert rc == 0 and (r.min_read_len, r.min_mean_qual, r.min_rq) == (0, 0, 0.0)
        for name, (sentence, good, bad) in RANGES.items():
            for text in good:
                rc, _, r = check(lib, dialect, {name: text})
                assert rc == 0 and getattr(r, name) == (RF.f32(float(text)) if name == "min_rq" else int(text))
            for text in bad:
                rc, why, _ = check(lib, dialect, {name: text})
                assert rc == _lib.READS_REFUSED and why == "--%s %s: %s%s" % (name, text, sentence, dot)
                assert check(lib, dialect, {name: text}, 0)[0] == 0  # (a range is no matter of the option itself)
            # (--min_rq is a decimal: strtof alone would take leading blanks, a sign, a hex float, "inf" and "nan")
            malformed = (("x", "", "20x", "0.99x", "0,99", " 0.5", "0x1p-1", "+0.5", "-0.5", "nan", "inf", "0.5 ") if name == "min_rq"
                         else ("x", "", "-3", "2.5", "20x"))
            for text in malformed:  # refused at the option (final = 0)
                for final in (0, 1):
                    rc, why, _ = check(lib, dialect, {name: text}, final)
                    assert rc == _lib.READS_NOT_A_NUMBER
                    assert why == ("--%s: not a number: '%s'" % (name, text) if dot else "invalid option: `--%s %s'" % (name, text))
        # the order: length, rq, mean quality
        rc, why, _ = check(lib, dialect, dict(min_read_len="0", min_mean_qual="0", min_rq="0"))
        assert why.startswith("--min_read_len 0")
        rc, why, _ = check(lib, dialect, dict(min_mean_qual="0", min_rq="0"))
        assert why.startswith("--min_rq 0")


def run(args, cwd):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=str(cwd))


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "r.fq").write_text("@r1\n" + "ACGTACGTAC" * 5 + "\n+\n" + "I" * 50 + "\n")
    (tmp_path / "f.bf").write_text("not a filter\n")
    return tmp_path


T = [TOOL, "--reads", "r.fq", "-k", 25, "-c", 2, "--bf", 4096]
N = [NTEDIT, "-f", "d.fa", "--reads", "r.fq", "-k", 25, "--cutoff", 2, "--bf", 4096]
CLI_REFUSALS = {
    "tool: length": (T + ["--min_read_len", 0], "--min_read_len 0: the minimum read length must be between 1 and 2147483647."),
    "tool: mean quality": (T + ["--min_mean_qual", 61], "--min_mean_qual 61: the minimum mean read quality must be between 1 and 60."),
    "tool: rq": (T + ["--min_rq", "1.5"], "--min_rq 1.5: the minimum read accuracy must be above 0 and at most 1."),
    "tool: malformed length": ([TOOL, "--reads", "r.fq", "--min_read_len", "1k", "-k", 25], "--min_read_len: not a number: '1k'"),
    "tool: malformed rq": ([TOOL, "--reads", "r.fq", "--min_rq", "Q20", "-k", 25], "--min_rq: not a number: 'Q20'"),
    "tool: behind --min_qual": (T + ["--min_rq", "0", "--min_qual", 94], "--min_qual 94: the minimum base quality"),
    "ntedit: length": (N + ["--min_read_len", 0], "--min_read_len 0: the minimum read length must be between 1 and 2147483647"),
    "ntedit: mean quality": (N + ["--min_mean_qual", 0], "--min_mean_qual 0: the minimum mean read quality must be between 1 and 60"),
    "ntedit: rq": (N + ["--min_rq", "0"], "--min_rq 0: the minimum read accuracy must be above 0 and at most 1"),
    "ntedit: malformed": (N + ["--min_mean_qual", "2x"], "invalid option: `--min_mean_qual 2x'"),
    "ntedit: malformed rq": (N + ["--min_rq", "0.9.9"], "invalid option: `--min_rq 0.9.9'"),
    "ntedit: length without --reads": ([NTEDIT, "-f", "d.fa", "-r", "f.bf", "--min_read_len", 20], "--min_read_len: only with --reads"),
    "ntedit: rq without --reads": ([NTEDIT, "-f", "d.fa", "-r", "f.bf", "--min_rq", "0.99"], "--min_rq: only with --reads"),
    "ntedit: mean quality with --genome": ([NTEDIT, "-f", "d.fa", "--genome", "d.fa", "-k", 25, "--min_mean_qual", 20],
                                           "--min_mean_qual: only with --reads (--genome builds"),
    "ntedit: rq with --genome": ([NTEDIT, "-f", "d.fa", "--genome", "d.fa", "-k", 25, "--min_rq", "0.99"],
                                 "--min_rq: only with --reads (--genome builds"),
}


@pytest.mark.parametrize("name", list(CLI_REFUSALS))
def test_the_binaries_refuse_before_the_device_is_opened(inputs, name):
    args, message = CLI_REFUSALS[name]
    before = sorted(os.listdir(inputs))
    r = run(args, inputs)
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert NO_DEVICE not in r.stderr and "no HIP device" not in r.stderr
    assert sorted(os.listdir(inputs)) == before


def test_the_python_drivers_refuse_before_any_device(inputs):
    env = dict(os.environ, PYTHONPATH=H.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    mr = ["ntedit_amd.make_reads", "--reads", "r.fq", "-k", "25", "-c", "2", "--bf", "4096"]
    rn = ["ntedit_amd.run", "-f", "d.fa", "--reads", "r.fq", "-k", "25", "--cutoff", "2", "--bf", "4096"]
    cases = [(mr + ["--min_mean_qual", "61"], "--min_mean_qual 61: the minimum mean read quality must be between 1 and 60."),
             (mr + ["--min_rq", "q"], "--min_rq: not a number: 'q'"),
             (mr + ["--min_read_len", "0"], "--min_read_len 0: the minimum read length must be between 1 and 2147483647."),
             (rn + ["--min_rq", "1.01"], "--min_rq 1.01: the minimum read accuracy must be above 0 and at most 1"),
             (rn + ["--min_mean_qual", "0"], "--min_mean_qual 0: the minimum mean read quality must be between 1 and 60"),
             (["ntedit_amd.run", "-f", "d.fa", "-r", "f.bf", "--min_mean_qual", "20"], "--min_mean_qual: only with --reads"),
             (["ntedit_amd.run", "-f", "d.fa", "-r", "f.bf", "--min_read_len", "20"], "--min_read_len: only with --reads")]
    for args, message in cases:
        before = sorted(os.listdir(inputs))
        r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=300, cwd=str(inputs), env=env)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr[-2000:])
        assert sorted(os.listdir(inputs)) == before


def test_the_help_texts_describe_the_options(inputs):
    r = run([NTEDIT, "--help-read-filter"], inputs)
    assert r.returncode == 0
    for words in ("--min_read_len L", "--min_rq R", "--min_mean_qual Q", "mean error probability", "S <= len * E[Q]",
                  "flag (BAM), length, rq, mean quality", "Phred+64, trimming, other BAM tags (np, ec), a maximum read length"):
        assert words in r.stderr, words
    r = run([TOOL, "--help"], inputs)
    assert r.returncode == 0 and all(o in r.stderr for o in ("--min_read_len", "--min_mean_qual", "--min_rq"))
    from ntedit_amd import make_reads
    assert all(o in make_reads.USAGE for o in ("--min_read_len", "--min_mean_qual", "--min_rq"))


def test_the_new_structs_are_as_the_header_has_them(tmp_path):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text("""#include "ntedit_hip.h"
#include <cstdio>
#include <cstddef>
int main() { printf("%zu %zu %zu %zu %zu\\n", sizeof(ntedit_hip_reads_filter_options), sizeof(ntedit_hip_reads_filter_rules),
                    offsetof(ntedit_hip_reads_filter_rules, min_rq), sizeof(ntedit_hip_reads_read_filter_stats),
                    offsetof(ntedit_hip_reads_read_filter_stats, aux_malformed)); }
""")
    subprocess.run(["c++", "-std=c++17", "-I", os.path.join(H.ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    want = [ctypes.sizeof(_lib.ReadsFilterOptions), ctypes.sizeof(_lib.ReadsFilterRules), _lib.ReadsFilterRules.min_rq.offset,
            ctypes.sizeof(_lib.ReadsReadFilterStats), _lib.ReadsReadFilterStats.aux_malformed.offset]
    assert [int(x) for x in out.split()] == want


# ---------------------------------------------------------------------------------- the host program, sanitized
def build_host(out_dir, sanitize):
    exe = os.path.join(str(out_dir), "read_filter_host_san" if sanitize else "read_filter_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    host = os.path.join(H.ROOT, "ntedit_amd", "host")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(H.ROOT, "ntedit_amd", "csrc"), "-o", exe, HOST_SRC,
                                                             os.path.join(host, "fasta.cpp"), os.path.join(host, "gunzip.cpp"),
                                                             "-lz", "-lpthread"], check=True)
    return exe


def host_cases():
    """[(kind, k, q, L, Q, R, bytes)]: the corpus through all three readers, and truncated files: a quality string cut
    short at every length, a BAM cut inside its qualities and inside its aux fields, broken aux fields"""
    cases = []
    for name, raw in sorted(PC.well_formed().items()):
        cases += [(kind, 12, q, L, Q, 0.0, raw) for kind in (0, 2) for q, L, Q in ((0, 0, 30), (20, 40, 20), (0, 0, 0))]
    for name, raw in sorted(PC.odd().items()):
        cases += [(0, 12, 0, 0, 20, 0.0, raw), (2, 12, 0, 0, 20, 0.0, raw)]
    rng = random.Random(3)
    recs = RF.draw_reads(rng, 8, 20, lengths=(20, 90))
    raw = RF.fastq_of(recs)
    cases += [(kind, 25, 0, 0, 20, 0.0, raw[:n]) for n in range(len(raw) - 200, len(raw) + 1) for kind in (0, 2)]
    cases += [(2, 12, 0, 30, 20, 0.0, MQ.fastq_wrapped(RF.three(recs), 7)[:n]) for n in range(0, 400, 3)]
    cases += [(2, 1, 0, 0, 20, 0.0, b"@a\nACGTACGT\n+\nIIII"), (2, 1, 0, 0, 20, 0.0, b"@a\nACGTACGT\n+\n"),
              (0, 1, 0, 0, 20, 0.0, b"@a\nACGTACGT\n+\nIIII\n"), (0, 1, 0, 0, 20, 0.0, b"@a\nACGTACGT\n+\n")]
    brecs = RF.draw_reads(rng, 12, 20, R=0.99, with_rq=True, lengths=(20, 200))
    brecs.append((b"all", SEQ, bytes([60]) * 128, BAM.all_aux() + b"rqf" + struct.pack("<f", 0.5)))
    brecs.append((b"noqual", SEQ, RF.NO_QUAL, b"XZZno nul"))
    _, braw = RF.bam_of(brecs)
    cases += [(1, RF.K, q, L, Q, R, braw) for q, L, Q, R in ((0, 0, 20, 0.99), (20, 60, 20, 0.99), (0, 0, 0, 0.99), (0, 0, 20, 0.0))]
    cases += [(1, 1, 0, 0, 20, 0.99, braw[:n]) for n in range(len(braw) - 400, len(braw) + 1)]
    for aux in (b"rq", b"rqf\0", b"XZZabc", b"XbBC" + struct.pack("<i", 1 << 30), b"XbBi" + struct.pack("<I", 0xFFFFFFFF), b"X"):
        cases.append((1, 1, 0, 0, 20, 0.99, BAM.header() + BAM.record(b"t", 0, SEQ, qual=bytes([30]) * 128, aux=aux)))
    return cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "address_undefined"])
def test_the_host_program(lib, tmp_path, sanitize):
    cases = host_cases()
    (tmp_path / "cases.bin").write_bytes(RF.pack_cases(cases))
    r = subprocess.run([build_host(tmp_path, sanitize), str(tmp_path / "cases.bin"), str(tmp_path / "scratch.fq")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    path = tmp_path / "again.fq"
    dropped = 0
    for (kind, k, q, L, Q, R, data), line in zip(cases, lines):
        got = [int(x) for x in line.split()]
        if kind == 0:
            res, text, st = RF.parse_model_f(lib, data, k, q, L, Q)
            assert got == [res.clean, res.broken, res.text_len, res.reads, MQ.fold(text), st["records"], st["dropped_length"],
                           st["dropped_mean_qual"]]
        elif kind == 1:
            res, text, st = RF.bam_model_f(lib, data, k, q, L, Q, R)
            assert got == [res.clean, res.broken, res.cut, res.kept, res.text_len, MQ.fold(text), st["records"], st["dropped_length"],
                           st["dropped_rq"], st["dropped_mean_qual"], st["rq_tagged"], st["aux_malformed"]]
            dropped += st["dropped_rq"] + st["dropped_mean_qual"]
        else:
            path.write_bytes(data)
            text, st = RF.range_text_f(lib, path, q, max(L, k), Q)
            assert got[:6] == [text.count(b"\n"), len(text), MQ.fold(text), st["records"], st["dropped_length"], st["dropped_mean_qual"]]
            dropped += st["dropped_mean_qual"]
    assert dropped > 100
