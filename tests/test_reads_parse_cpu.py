"""--gpu_parse without a GPU: the flag's surface on the front ends, and the clean grammar's serial model
(ntedit_hip_reads_parse_model, built from the functions the kernels use) against the host parser
(ntedit_hip_reads_range_text): a chunk declared clean has exactly the host parser's text."""
import os
import subprocess

import pytest

import helpers as H
import parse_corpus as PC
from ntedit_amd import _lib, make_reads

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
MKRBF = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(NTEDIT) and os.path.exists(MKRBF)):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return _lib.load()


# ---------------------------------------------------------------------------------- the flag
def test_help_of_both_binaries_lists_the_flag(lib, tmp_path):
    for exe in (NTEDIT, MKRBF):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 0
        assert "--gpu_parse" in r.stderr, exe
    assert "--gpu_parse" in make_reads.USAGE


def test_without_reads_the_polisher_refuses_it_before_the_device(lib, tmp_path):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "x.bf").write_bytes(b"")
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([NTEDIT, "-f", "d.fa", "-b", "out", "-r", "x.bf", "--gpu_parse"], capture_output=True, text=True,
                       timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--gpu_parse: only with --reads" in r.stderr
    assert "HIP device" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_the_python_driver_refuses_it_without_reads(lib, tmp_path):
    from ntedit_amd import run
    with pytest.raises(make_reads.Refused, match="--gpu_parse: only with --reads"):
        run.parse(["-f", "d.fa", "-r", "x.bf", "--gpu_parse"])


@pytest.mark.parametrize("dialect,given", [(_lib.READS_DIALECT_TOOL, dict(k="25", cutoff="2", bf="4096")),
                                           (_lib.READS_DIALECT_POLISHER, dict(k="25", cutoff="2", bf="4096"))])
def test_the_rules_return_the_flag_in_both_dialects(lib, dialect, given):
    for flag in (False, True):
        a = make_reads.check_options(dialect, given, True, (), False, "", flag)
        assert a["gpu_parse"] is flag


def test_the_tool_dialect_front_end_takes_the_flag(lib, tmp_path):
    a = make_reads.parse(["--reads", "r.fq", "-k", "25", "-c", "2", "--bf", "4096", "--gpu_parse"])
    assert a["gpu_parse"] is True
    assert make_reads.parse(["--reads", "r.fq", "-k", "25", "-c", "2", "--bf", "4096"])["gpu_parse"] is False


# ---------------------------------------------------------------------------------- the fixed corpus
def _both(lib, tmp_path, raw, k):
    path = tmp_path / "in.txt"
    path.write_bytes(raw)
    return PC.host_text(lib, str(path), k), PC.model(lib, raw, k)


@pytest.mark.parametrize("k", PC.KS)
@pytest.mark.parametrize("name", sorted(PC.well_formed()))
def test_well_formed_inputs_are_clean_and_equal_the_host_parser(lib, tmp_path, name, k):
    raw = PC.well_formed()[name]
    (text, reads, bases), (res, mtext) = _both(lib, tmp_path, raw, k)
    assert res.clean == 1 and res.broken == 0, (name, res.broken)
    assert mtext == text
    assert (res.reads, res.bases, res.text_len) == (reads, bases, len(text))
    if raw:
        assert res.kind == raw[0]


@pytest.mark.parametrize("k", PC.KS)
@pytest.mark.parametrize("name", sorted(PC.odd()))
def test_odd_inputs_are_not_clean(lib, name, k):
    res, _ = PC.model(lib, PC.odd()[name], k)
    assert res.clean == 0 and res.broken != 0, name


def test_the_line_table_bound_is_part_of_the_grammar(lib):
    # one line per 8 raw bytes (+ 1): 2-byte lines are far over it
    res, _ = PC.model(lib, b">a\n" + b"A\n" * 64, 12)
    assert res.clean == 0 and res.broken & _lib.PARSE_BAD["table"]
    res, _ = PC.model(lib, b">a\n" + (b"ACGTACGT" * 2 + b"\n") * 64, 12)
    assert res.clean == 1


# ---------------------------------------------------------------------------------- generated cases
def test_generated_cases_clean_means_the_host_parsers_text(lib, tmp_path):
    cases = PC.generated(3000)
    assert len(cases) >= 2000
    path = tmp_path / "case.txt"
    clean_mutated = 0
    for i, (raw, k, mutated) in enumerate(cases):
        res, mtext = PC.model(lib, raw, k)
        if not mutated:
            # (so that "everything is unclean" cannot pass)
            assert res.clean == 1, (i, res.broken, raw)
        if res.clean:
            path.write_bytes(raw)
            text, reads, bases = PC.host_text(lib, str(path), k)
            assert mtext == text, (i, mutated, raw)
            assert (res.reads, res.bases) == (reads, bases), (i, raw)
            clean_mutated += mutated
    # some mutations stay inside the grammar (a byte of a header, a duplicated FASTA line): they are compared too
    assert clean_mutated > 50
