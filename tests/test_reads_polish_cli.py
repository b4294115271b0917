"""`ntedit --reads` without a GPU: the usage text lists the reads options, and every refusal of the one-step mode
happens before the device is opened, names the option, exits with status 1 and writes no file."""
import os
import subprocess

import pytest

import helpers as H

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")


@pytest.fixture(scope="module")
def ntedit():
    if not os.path.exists(NTEDIT):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return NTEDIT


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "r.fq").write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return tmp_path


def _run(ntedit, args, cwd):
    return subprocess.run([ntedit] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_reads_options(ntedit, tmp_path):
    r = _run(ntedit, ["--help"], tmp_path)
    assert r.returncode == 0
    for opt in ("--reads", "--cutoff", "--solid", "--counts", "--hashes", "--fpr", "--bf", "--num_elements",
                "--sketch_bytes", "--hist", "--save_bf"):
        assert opt in r.stderr, opt
    # the options that only tests use stay out of the usage text
    assert "--batch_bytes" not in r.stderr and "--resident_cap" not in r.stderr


BASE = ["-k", "25", "--cutoff", "2", "--bf", "4096"]


@pytest.mark.parametrize("args,message", [
    (["--reads", "r.fq", "-r", "r.fq"] + BASE, "--reads and -r"),
    (["--reads", "r.fq", "--shard", "0/2"] + BASE, "--reads and --shard"),
    (["--reads", "r.fq", "--cutoff", "2", "--bf", "4096"], "-k: required"),
    (["--reads", "r.fq", "-k", "11", "--cutoff", "2", "--bf", "4096"], "-k 11: k must be between 12 and 200"),
    (["--reads", "r.fq", "-k", "201", "--cutoff", "2", "--bf", "4096"], "-k 201: k must be between 12 and 200"),
    (["--reads", "r.fq", "-k", "x25", "--cutoff", "2", "--bf", "4096"], "-k x25"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--solid", "--bf", "4096"], "--cutoff and --solid"),
    (["--reads", "r.fq", "-k", "25", "--bf", "4096"], "--cutoff or --solid"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "0", "--bf", "4096"], "--cutoff 0: the minimum count"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "256", "--bf", "4096"], "--cutoff 256: the minimum count"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--hashes", "0", "--bf", "4096"], "--hashes 0"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--hashes", "9", "--bf", "4096"], "--hashes 9"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2"], "--bf or --num_elements"),
    (["--reads", "r.fq", "-k", "25", "--cutoff", "2", "--bf", "0"], "--bf / --num_elements"),
    (["--reads", "-k", "25", "--cutoff", "2", "--bf", "4096"], "--reads: 1 or more files"),
    (["--reads", "missing.fq"] + BASE, "missing.fq"),
    (["-r", "r.fq", "--solid"], "--solid: only with --reads"),
])
def test_refusals_come_before_the_device_and_write_nothing(ntedit, inputs, args, message):
    before = sorted(os.listdir(inputs))
    extra = ["--save_bf", "s.bf"] if "--reads" in args else []
    r = _run(ntedit, ["-f", "d.fa", "-b", "out"] + args + extra, inputs)
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    # (a device opened here would have failed with "no usable HIP device" on a machine without one)
    assert "HIP device" not in r.stderr
    assert sorted(os.listdir(inputs)) == before


def test_without_reads_k_is_still_accepted_and_ignored(ntedit, inputs):
    # -k with -r stays accepted as before: the run goes past the argument checks (to the missing filter file here)
    r = _run(ntedit, ["-f", "d.fa", "-r", "no.bf", "-k", "x"], inputs)
    assert r.returncode == 1 and "no.bf" in r.stderr and "-k" not in r.stderr
