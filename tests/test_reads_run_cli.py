"""`python -m ntedit_amd.run --reads` without a GPU: every refusal of `ntedit --reads` (and the reads options without
--reads) happens before any device is opened, names the option, exits with status 1 and writes no file; without
--reads the driver's argument handling is what it was; and the reads arguments size the sketch and the filter exactly
as ntedit_amd.make_reads and the one-process tools do."""
import os
import subprocess
import sys

import pytest

import helpers as H


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "r.fq").write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return tmp_path


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=H.ROOT)
    return subprocess.run([sys.executable, "-m", "ntedit_amd.run"] + [str(a) for a in args], capture_output=True,
                          text=True, timeout=120, cwd=str(cwd), env=env)


def _main(args, cwd, monkeypatch, capsys):
    from ntedit_amd import run
    monkeypatch.chdir(cwd)
    rc = run.main([str(a) for a in args])
    return rc, capsys.readouterr().err


BASE = ["-k", "25", "--cutoff", "2", "--bf", "4096"]

REFUSALS = [
    (["--reads", "r.fq", "-r", "r.fq"] + BASE, "--reads and -r"),
    (["--reads", "r.fq", "--cutoff", "2", "--bf", "4096"], "-k: required"),
    (["--reads", "r.fq", "-k", "11", "--cutoff", "2", "--bf", "4096"], "-k 11: k must be between 12 and 200"),
    (["--reads", "r.fq", "-k", "201", "--cutoff", "2", "--bf", "4096"], "-k 201: k must be between 12 and 200"),
    (["--reads", "r.fq", "-k", "x25", "--cutoff", "2", "--bf", "4096"], "-k x25"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--solid", "--bf", "4096"], "--cutoff and --solid"),
    (["--reads", "r.fq", "-k", "25", "--bf", "4096"], "--cutoff or --solid"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "0", "--bf", "4096"], "--cutoff 0: the minimum count"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "256", "--bf", "4096"], "--cutoff 256: the minimum count"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "x", "--bf", "4096"], "--cutoff x"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--hashes", "0", "--bf", "4096"], "--hashes 0"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--hashes", "9", "--bf", "4096"], "--hashes 9"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--fpr", "1.5", "--num_elements", "100"], "--fpr 1.5"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2"], "--bf or --num_elements"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--bf", "0"], "--bf / --num_elements: the filter would be empty"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--num_elements", "0"], "--bf / --num_elements"),
    (["--reads", "r.fq", "--batch_bytes", "100"] + BASE, "--batch_bytes: at least 4096"),
    (["--reads", "-k", "25", "--cutoff", "2", "--bf", "4096"], "--reads: 1 or more files"),
    (["--reads", "missing.fq"] + BASE, "missing.fq"),
    (["-r", "r.fq", "--solid"], "--solid: only with --reads"),
    (["-r", "r.fq", "--cutoff", "2"], "--cutoff: only with --reads"),
    (["-r", "r.fq", "--save_bf", "s.bf"], "--save_bf: only with --reads"),
    (["-r", "r.fq", "--no-split"], "--no-split: only with --reads"),
    (["-r", "r.fq", "--resident_cap", "0"], "--resident_cap: only with --reads"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_refusals_come_before_the_device_and_write_nothing(inputs, monkeypatch, capsys, args, message):
    before = sorted(os.listdir(inputs))
    extra = ["--save_bf", "s.bf"] if "--reads" in args else []
    rc, err = _main(["-f", "d.fa", "-b", "out"] + args + extra, inputs, monkeypatch, capsys)
    assert rc == 1, err
    assert message in err, err
    assert "HIP device" not in err
    assert sorted(os.listdir(inputs)) == before


def test_a_refusal_exits_with_status_1_from_the_command_line(inputs):
    r = _run(["-f", "d.fa", "--reads", "r.fq", "-k", "25", "--solid", "--cutoff", "2", "--save_bf", "s.bf"], inputs)
    assert r.returncode == 1, r.stderr
    assert "--cutoff and --solid" in r.stderr and "HIP device" not in r.stderr
    assert sorted(os.listdir(inputs)) == ["d.fa", "r.fq"]


def test_help_lists_the_reads_options(inputs):
    r = _run(["--help"], inputs)
    assert r.returncode == 0
    for opt in ("--reads", "--cutoff", "--solid", "--counts", "--hashes", "--fpr", "--bf", "--num_elements",
                "--sketch_bytes", "--hist", "--save_bf", "--no-split"):
        assert opt in r.stdout, opt
    assert "--batch_bytes" not in r.stdout and "--resident_cap" not in r.stdout


def test_without_reads_the_arguments_are_handled_as_before():
    from ntedit_amd import run
    a = run.parse(["-f", "d.fa", "-r", "x.bf", "-k", "31", "-p", "2", "--report"])
    assert (a.draft, a.bf, a.k_ignored, a.min_threshold, a.report, a.reads_args) == ("d.fa", "x.bf", 31, 2, True, None)
    # -r stays required and -k an (ignored) integer: argparse's own messages and status
    for argv, message in ((["-f", "d.fa"], "the following arguments are required: -r"),
                          (["-f", "d.fa", "-r", "x.bf", "-k", "x"], "argument -k: invalid int value")):
        r = subprocess.run([sys.executable, "-c", "import sys; from ntedit_amd import run; run.parse(sys.argv[1:])"] +
                           argv, capture_output=True, text=True, timeout=60, cwd=H.ROOT)
        assert r.returncode == 2 and message in r.stderr, r.stderr


def test_the_reads_arguments_size_as_make_reads_does(inputs):
    from ntedit_amd import _lib, make_reads, run
    lib = _lib.load()
    r = str(inputs / "r.fq")
    cases = [
        (["-k", "31", "--cutoff", "3", "--bf", "100000", "--hashes", "4"],
         ["-k", "31", "-c", "3", "--bf", "100000", "--hashes", "4"]),
        (["-k", "25", "--cutoff", "2", "--num_elements", "5000000", "--fpr", "0.02"],
         ["-k", "25", "-c", "2", "--num_elements", "5000000", "--fpr", "0.02"]),
        (["-k", "25", "--solid", "--counts", "--sketch_bytes", "1000003", "--hist", "h"],
         ["-k", "25", "--solid", "--counts", "--sketch_bytes", "1000003", "--hist", "h"]),
        (["-k", "25", "--cutoff", "2", "--hist", "h", "--no-split", "--batch_bytes", "65536"],
         ["-k", "25", "-c", "2", "--hist", "h", "--no-split", "--batch_bytes", "65536"]),
    ]
    for ours, tools in cases:
        a = run.parse(["-f", str(inputs / "d.fa"), "--reads", r, r] + ours).reads_args
        b = make_reads.parse(["--reads", r, r] + tools)
        for key in ("reads", "k", "cmin", "solid", "hist", "counts", "hashes", "fpr", "bf", "num_elements",
                    "sketch_bytes", "batch_bytes", "no_split", "gather_hist", "size_from_hist"):
            assert a[key] == b[key], (key, ours)
        assert make_reads.sizes(lib, a) == make_reads.sizes(lib, b), ours
    a = run.parse(["-f", str(inputs / "d.fa"), "--reads", r] + BASE).reads_args
    assert a["store_cap"] == make_reads.RESIDENT_CAP_DEFAULT == 48 << 30
    a = run.parse(["-f", str(inputs / "d.fa"), "--reads", r, "--resident_cap", "0"] + BASE).reads_args
    assert a["store_cap"] == 0
