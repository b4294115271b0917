"""--gpu_parse for genome FASTA without a GPU: the serial model of the stateful genome grammar
(ntedit_hip_genome_parse_model, built from the functions the kernels use) against the host parser
(ntedit_hip_reads_range_text) by the split rule; that no cutting of a file changes its text; the model under the
address and undefined-behaviour sanitizers; and what the two front ends refuse before they open a device."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import genome_corpus as GC
import helpers as H
from ntedit_amd import _lib

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
MKBF = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-genome-bf")


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(NTEDIT) and os.path.exists(MKBF)):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return _lib.load()


# ---------------------------------------------------------------------------------- the model against the host parser
def against_the_host_parser(lib, path, raw, res, text):
    """the split rule: the text's pieces of k bytes or more are the host parser's reads, `bases` its genome size"""
    path.write_bytes(raw)
    for k in GC.KS:
        reads, all_bases = GC.host_records(lib, str(path), k)
        assert GC.records_of_text(text, k) == reads, (k, raw[:200])
        assert res.bases == all_bases == len(text) - text.count(b"\n")


@pytest.mark.parametrize("name", sorted(GC.well_formed()))
def test_well_formed_files_are_clean_and_hold_the_host_parsers_records(lib, tmp_path, name):
    raw = GC.well_formed()[name]
    res, text = GC.model(lib, raw)
    assert res.clean == 1 and res.broken == 0, (name, res.broken)
    against_the_host_parser(lib, tmp_path / "in.fa", raw, res, text)
    assert res.lines == raw.count(b"\n") + (1 if raw and not raw.endswith(b"\n") else 0)
    heads = [i for i in range(len(raw)) if raw[i:i + 1] == b">" and (i == 0 or raw[i - 1:i] == b"\n")]
    assert res.last_header == (heads[-1] if heads else GC.NO_START)
    assert text.count(b"\n") == len(heads)


@pytest.mark.parametrize("name", sorted(GC.odd()))
def test_odd_files_are_not_clean(lib, name):
    res, _ = GC.model(lib, GC.odd()[name])
    assert res.clean == 0 and res.broken != 0, name


def test_each_rule_names_its_bit(lib):
    bad = _lib.PARSE_BAD
    odd = GC.odd()
    for name, bit in (("crlf", "cr"), ("an_empty_line", "empty"), ("an_empty_line_at_the_end", "empty"),
                      ("a_line_starting_with_at", "seq_start"), ("a_line_starting_with_plus", "seq_start"),
                      ("junk_before_the_first_record", "first"), ("wrapped_1_over_the_line_bound", "table")):
        assert GC.model(lib, odd[name])[0].broken == bad[bit], name
    assert GC.model(lib, odd["a_fastq_file"])[0].broken == bad["first"] | bad["seq_start"]
    # a first byte '\n' is an empty line under LINE_START only; line 0 of a continued line may start with anything
    assert GC.model(lib, b"\nACGTACGTACGT\n", GC.LINE_START, False)[0].broken == bad["empty"]
    for state in (GC.IN_HEADER, GC.IN_SEQ):
        for raw in (b"\nACGTACGTACGT\n", b"+CGTACGTACGT\n", b"@CGTACGTACGT\n", b">CGTACGTACGT\n"):
            assert GC.model(lib, raw, state, False)[0].clean == 1, (state, raw)
    # only the file's first chunk has to start with '>'
    assert GC.model(lib, b"ACGTACGT\n", GC.LINE_START, False)[0].clean == 1
    assert GC.model(lib, b"ACGTACGT\n", GC.LINE_START, True)[0].broken == bad["first"]


def test_entry_and_exit_states(lib):
    m = lambda raw, state: GC.model(lib, raw, state, False)
    # an empty chunk keeps its entry state
    for state in GC.STATES:
        res, text = m(b"", state)
        assert (res.clean, res.state_out, res.text_len, res.lines, res.last_header) == (1, state, 0, 0, GC.NO_START)
    # the middle of a header: no text, still inside the header
    res, text = m(b"chr1 some words", GC.IN_HEADER)
    assert (res.clean, res.state_out, text, res.lines, res.last_header) == (1, GC.IN_HEADER, b"", 1, GC.NO_START)
    # the same bytes inside a sequence line are sequence
    res, text = m(b"ACGTNNNNacgt", GC.IN_SEQ)
    assert (res.clean, res.state_out, text, res.bases) == (1, GC.IN_SEQ, b"ACGTNNNNacgt", 12)
    # only the '\n' that ends a sequence line
    res, text = m(b"\n", GC.IN_SEQ)
    assert (res.clean, res.state_out, text, res.lines) == (1, GC.LINE_START, b"", 1)
    # a header that begins in the chunk gives one '\n', its continued part nothing
    res, text = m(b"rest of a header\nACGT\n>next one", GC.IN_HEADER)
    assert (res.clean, res.state_out, text, res.bases, res.last_header) == (1, GC.IN_HEADER, b"ACGT\n", 4, 22)


def test_generated_files_against_the_host_parser(lib, tmp_path):
    cases = GC.generated(3000)
    clean_mutated = unclean = 0
    for i, (raw, k, mutated) in enumerate(cases):
        res, text = GC.model(lib, raw)
        if not mutated:
            # (so that "everything is unclean" cannot pass)
            assert res.clean == 1, (i, res.broken, raw)
        if res.clean:
            against_the_host_parser(lib, tmp_path / "case.fa", raw, res, text)
            clean_mutated += mutated
        else:
            unclean += 1
    # some mutations stay inside the grammar (a byte of a header, a duplicated line): they are compared too
    assert clean_mutated > 50 and unclean > 100


# ---------------------------------------------------------------------------------- chunking changes nothing
# The line bound (more than n / 8 + 1 lines) is the one rule that depends on the cuts: a line cut in two counts in both
# chunks and every chunk has its own "+ 1", so a small chunk of short lines breaks it where the whole file does not (and
# a file just over it may be cut into chunks within it).  It is set aside here and checked on its own below; every other
# rule must be reported by some chunk exactly when the whole file breaks it -- a '\r' is caught wherever the cuts fall,
# an empty line cut between its two '\n' by the first byte '\n' under LINE_START.
def same_as_whole(lib, raw, cuts):
    def parse(chunk, state, first):
        res, text = GC.model(lib, chunk, state, first)
        # the line bound, restated: each chunk reports it exactly when its own lines are over its own n / 8 + 1
        lines = chunk.count(b"\n") + (1 if chunk and not chunk.endswith(b"\n") else 0)
        assert bool(res.broken & GC.TABLE) == (lines > len(chunk) // 8 + 1), (cuts, len(chunk), lines)
        return res, text

    whole, wtext = GC.model(lib, raw)
    parse(raw, GC.LINE_START, True)
    got = GC.run_chunks(parse, raw, cuts)
    assert got["text"] == wtext, cuts
    assert (got["bases"], got["last_header"], got["state"]) == (whole.bases, whole.last_header, whole.state_out), cuts
    assert (got["broken"] & ~GC.TABLE != 0) == (whole.broken & ~GC.TABLE != 0), (cuts, got["broken"], whole.broken)
    if whole.broken & _lib.PARSE_BAD["cr"]:
        assert got["broken"] & _lib.PARSE_BAD["cr"]
    return got, whole


def test_a_file_cut_in_two_at_every_position(lib):
    rng = random.Random(5)
    raw = (">first record\n" + GC._wrap(GC._seq(rng, 200), 60) + ">second, with a longer header line\n" + GC._seq(rng, 130) +
           "\n>third\n>fourth\n" + GC._wrap(GC._seq(rng, 170, "ACGTNacgt"), 37)).encode()
    assert 550 < len(raw) < 650
    for cut in range(len(raw) + 1):
        got, whole = same_as_whole(lib, raw, [cut])
        # every line of this file has 8 bytes or more: no cutting in two is over the line bound, so clean stays clean
        assert whole.clean == 1 and got["broken"] == 0, cut
    # ... and the same file with a damaged byte at every tenth position is caught at every cut around it
    for at in range(5, len(raw), 45):
        for ch in (b"\r", b"\n", b"+", b"@"):
            bad = raw[:at] + ch + raw[at + 1:]
            for cut in {0, at - 1, at, at + 1, at + 2, len(bad) // 2, len(bad)}:
                same_as_whole(lib, bad, [cut])


def test_random_files_cut_in_three(lib):
    rng = random.Random(6)
    unclean = 0
    for raw, _, mutated in GC.generated(2000, seed=99):
        cuts = sorted(rng.randint(0, len(raw)) for _ in range(2))
        _, whole = same_as_whole(lib, raw, cuts)
        unclean += not whole.clean
    assert unclean > 50  # (so that the cuttings of unclean files are compared too)


def test_the_line_bound_is_each_chunks_own(lib):
    # a chunk of 7 bytes with a '\n' in its middle has 2 lines, over 7 / 8 + 1: unclean, and still parsed
    res, text = GC.model(lib, b"ACG\nTGA", GC.IN_SEQ, False)
    assert (res.clean, res.broken, text, res.state_out, res.lines) == (0, GC.TABLE, b"ACGTGA", GC.IN_SEQ, 2)
    # only over the table itself the chunk is not looked at: more lines than (n + 2^20) / 8 + 1
    raw = b">a\n" + b"A\n" * 200_000
    res, text = GC.model(lib, raw)
    assert (res.clean, res.broken, res.text_len, res.lines) == (0, GC.TABLE, 0, 200_001)
    res, text = GC.model(lib, b">a\n" + b"A\n" * 100_000)
    assert (res.clean, res.broken, res.text_len, res.bases) == (0, GC.TABLE, 100_001, 100_000)


# ---------------------------------------------------------------------------------- the model under the sanitizers
SANITIZED = r"""
// every case of a file through gp_model (nte_genome_grammar.h), raw and text in heap blocks of exactly their sizes
#include "nte_genome_grammar.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv)
{
	FILE* f = fopen(argv[1], "rb");
	uint32_t n = 0, head[4];
	if (!f || fread(&n, 4, 1, f) != 1) return 2;
	for (uint32_t i = 0; i < n; i++) {
		if (fread(head, 4, 4, f) != 4) return 2; // raw bytes, entry state, first chunk, text bytes
		char* raw = (char*)malloc(head[0]); // (a block of 0 bytes: any access is reported)
		if (head[0] && fread(raw, 1, head[0], f) != head[0]) return 2;
		char* out = (char*)malloc(head[3]);
		nte_parse::GpResult r;
		const bool fits = nte_parse::gp_model(raw, head[0], (int)head[1], (int)head[2], out, head[3], &r);
		unsigned long long sum = 0;
		for (uint64_t b = 0; fits && b < r.text_len; b++) sum = sum * 131 + (unsigned char)out[b];
		printf("%d %d %u %d %llu %llu %llu %llu %llu\n", (int)fits, r.clean, r.broken, r.state_out, (unsigned long long)r.text_len,
		       (unsigned long long)r.bases, (unsigned long long)r.lines, (unsigned long long)r.last_header, sum);
		free(raw), free(out);
	}
	return 0;
}
"""


def test_the_model_under_address_and_undefined_behaviour_sanitizers(lib, tmp_path):
    """the grammar header alone, built for the host with -fsanitize=address,undefined: the corpus in every entry state,
    cut and whole, and 300 generated files, the raw bytes and the text each in a heap block of its exact size (the text
    block: exactly text_len bytes, and once one byte less); the results are the library's"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    flags = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
    # only a compiler that cannot build an empty program with the sanitizers skips: an error in the header must fail
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run(flags + ["-o", str(tmp_path / "probe"), str(tmp_path / "probe.cpp")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + probe.stderr[-300:])
    (tmp_path / "san.cpp").write_text(SANITIZED)
    exe = tmp_path / "san"
    build = subprocess.run(flags + ["-I", H.ROOT + "/ntedit_amd/csrc", "-o", str(exe), str(tmp_path / "san.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = list(GC.well_formed().values()) + list(GC.odd().values()) + [raw for raw, _, _ in GC.generated(300, seed=7)]
    cases, want = [], []
    for raw in files:
        for chunk in (raw, raw[:len(raw) // 2], raw[len(raw) // 2:], raw[len(raw) // 3:len(raw) // 3 + 7]):
            for state in GC.STATES:
                for first in (0, 1):
                    res, text = GC.model(lib, chunk, state, first)
                    for cap in {res.text_len, max(res.text_len, 1) - 1}:
                        cases.append((chunk, state, first, cap))
                        fits = cap >= res.text_len
                        s = 0
                        for b in text if fits else b"":
                            s = (s * 131 + b) % (1 << 64)
                        want.append((int(fits),) + GC.fields(res)[:1] + GC.fields(res)[1:] + (s,))
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for chunk, state, first, cap in cases:
            f.write(struct.pack("<IIII", len(chunk), state, first, cap) + chunk)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(want) > 5000
    assert got == want


# ---------------------------------------------------------------------------------- the tool's new flags
def run(exe, args, cwd):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_the_tools_help_lists_the_flag(lib, tmp_path):
    r = run(MKBF, ["--help"], tmp_path)
    assert r.returncode == 0 and "--gpu_parse" in r.stderr


@pytest.mark.parametrize("args,why", [
    (["--gpu_parse", "-k", "1"], "--gpu_parse: -k must be within"),
    (["--gpu_parse", "-k", "300"], "--gpu_parse: -k must be within"),
    (["--gpu_parse", "-k", "25", "--batch_bytes", "0"], "--batch_bytes: at least 1"),
    (["--gpu_parse", "-k", "25", "--batch_bytes"], "Too few arguments for '--batch_bytes'"),
])
def test_the_tool_refuses_before_the_device(lib, tmp_path, args, why):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    before = sorted(os.listdir(tmp_path))
    r = run(MKBF, ["--genome", "g.fa"] + args, tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr
    assert why in r.stderr and "HIP device" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == before


# ---------------------------------------------------------------------------------- ntedit --genome
def test_the_polishers_help_lists_the_genome_options(lib, tmp_path):
    r = run(NTEDIT, ["--help"], tmp_path)
    assert r.returncode == 0 and "--genome FILE..." in r.stderr and "ntedit-make-genome-bf" in r.stderr


G = ["--genome", "g.fa"]


@pytest.mark.parametrize("args,why", [
    (G + ["-k", "25", "-r", "x.bf"], "--genome and -r: give one of them"),
    (G + ["-k", "25", "--reads", "g.fa"], "--genome and --reads: give one of them"),
    (G + ["-k", "25", "--shard", "0/2"], "--genome and --shard: "),
    (["--genome", "-k", "25"], "--genome: 1 or more files expected"),
    (G, "-k: required with --genome"),
    (G + ["-k", "11"], "-k 11: k must be between 12 and 200"),
    (G + ["-k", "201"], "-k 201: k must be between 12 and 200"),
    (G + ["-k", "2x"], "-k 2x: k must be between 12 and 200"),
    (G + ["-k", "25", "--hashes", "0"], "--hashes 0: the number of hash functions must be between 1 and 8"),
    (G + ["-k", "25", "--hashes", "9"], "--hashes 9: the number of hash functions must be between 1 and 8"),
    (G + ["-k", "25", "--bf", "0"], "--bf / --num_elements: the filter would be empty"),
    (G + ["-k", "25", "--cutoff", "2"], "--cutoff: only with --reads"),
    (G + ["-k", "25", "--solid"], "--solid: only with --reads"),
    (G + ["-k", "25", "--counts"], "--counts: only with --reads"),
    (G + ["-k", "25", "--hist", "h.txt"], "--hist: only with --reads"),
    (G + ["-k", "25", "--reject_cutoff", "3"], "--reject_cutoff: only with --reads"),
    (G + ["-k", "25", "--reject_bf", "4096"], "--reject_bf: only with --reads"),
    (G + ["-k", "25", "--reject_num_elements", "100"], "--reject_num_elements: only with --reads"),
    (G + ["-k", "25", "--save_reject_bf", "r.bf"], "--save_reject_bf: only with --reads"),
    (G + ["-k", "25", "--resident_cap", "0"], "--resident_cap: only with --reads"),
    (G + ["-k", "25", "--bf", "12x"], "invalid option: `--bf 12x'"),
    (["--genome", "missing.fa", "-k", "25"], "`missing.fa': No such file or directory"),
    # the genome options without --genome are refused as the reads options are
    (["-r", "x.bf", "--hashes", "3"], "--hashes: only with --reads or --genome"),
    (["-r", "x.bf", "--fpr", "0.01"], "--fpr: only with --reads or --genome"),
    (["-r", "x.bf", "--bf", "4096"], "--bf: only with --reads or --genome"),
    (["-r", "x.bf", "--num_elements", "100"], "--num_elements: only with --reads or --genome"),
    (["-r", "x.bf", "--save_bf", "s.bf"], "--save_bf: only with --reads or --genome"),
    (["-r", "x.bf", "--gpu_parse"], "--gpu_parse: only with --reads or --genome"),
    (["-r", "x.bf", "--cutoff", "2"], "--cutoff: only with --reads"),
])
def test_the_polisher_refuses_before_the_device(lib, tmp_path, args, why):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "g.fa").write_text(">g\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "x.bf").write_bytes(b"")
    before = sorted(os.listdir(tmp_path))
    r = run(NTEDIT, ["-f", "d.fa", "-b", "out"] + args, tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr
    assert why in r.stderr and "HIP device" not in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
