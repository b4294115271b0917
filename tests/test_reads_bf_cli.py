"""ntedit-make-reads-bf without a GPU: the binary is built, its usage text, the argument checks that run before any
device is opened, and the loud failure (no output file) when there is no device."""
import os
import subprocess

import pytest

import helpers as H

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return TOOL


@pytest.fixture()
def reads(tmp_path):
    f = tmp_path / "r.fq"
    f.write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return str(f)


def _run(tool, *args, cwd=None):
    return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


def test_binary_is_built(tool):
    assert os.access(tool, os.X_OK)


def test_help(tool):
    r = _run(tool, "--help")
    assert r.returncode == 0
    for opt in ("--reads", "-k", "-c", "--counts", "--hashes", "--fpr", "--bf", "--num_elements", "--sketch_bytes"):
        assert opt in r.stderr
    # no parity claim with the CPU counters of the reference's pipeline
    assert "Neither" in r.stderr and "ntHits" in r.stderr and "ntStat" in r.stderr


def test_usage_without_arguments(tool):
    r = _run(tool)
    assert r.returncode != 0
    assert "--reads" in r.stderr and "Usage" in r.stderr


@pytest.mark.parametrize("args,message", [
    (["-k", "11", "-c", "2", "--bf", "4096"], "between 12 and 200"),
    (["-k", "201", "-c", "2", "--bf", "4096"], "between 12 and 200"),
    (["-k", "x25", "-c", "2", "--bf", "4096"], "not a number"),
    (["-c", "2", "--bf", "4096"], "-k: required"),
    (["-k", "25", "-c", "0", "--bf", "4096"], "between 1 and 255"),
    (["-k", "25", "-c", "256", "--bf", "4096"], "between 1 and 255"),
    (["-k", "25", "--bf", "4096"], "-c: required"),
    (["-k", "25", "-c", "2", "--hashes", "9", "--bf", "4096"], "between 1 and 8"),
    (["-k", "25", "-c", "2", "--hashes", "0", "--bf", "4096"], "between 1 and 8"),
    (["-k", "25", "-c", "2"], "--bf or --num_elements"),
    (["-k", "25", "-c", "2", "--bf", "0"], "empty"),
    (["-k", "25", "-c", "2", "--bf", "4096", "--bogus"], "Unknown argument"),
])
def test_bad_arguments_are_refused(tool, reads, tmp_path, args, message):
    out = tmp_path / "o.bf"
    r = _run(tool, "--reads", reads, "-o", str(out), *args)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert not out.exists()


def test_no_reads_is_refused(tool):
    r = _run(tool, "-k", "25", "-c", "2", "--bf", "4096")
    assert r.returncode != 0 and "--reads" in r.stderr


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly_and_writes_nothing(tool, reads, tmp_path):
    out = tmp_path / "o.bf"
    r = _run(tool, "--reads", reads, "-k", "25", "-c", "2", "--bf", "4096", "-o", str(out), cwd=str(tmp_path))
    assert r.returncode != 0 and "error" in r.stderr
    assert not out.exists()
    assert os.listdir(tmp_path) == ["r.fq"]


def test_library_exports_the_reads_calls():
    from ntedit_amd import _lib
    lib = _lib.load()
    for s in ("ntedit_hip_sketch_alloc", "ntedit_hip_sketch_count", "ntedit_hip_filter_insert_solid",
              "ntedit_hip_filter_alloc_counting"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    # a null context is an argument error, not a crash
    assert lib.ntedit_hip_sketch_alloc(None, 1 << 20, 3, 25) != 0
    assert lib.ntedit_hip_sketch_count(None, b"ACGT", 4, 0) != 0
    assert lib.ntedit_hip_filter_insert_solid(None, 0, b"ACGT", 4, 0, 2) != 0
