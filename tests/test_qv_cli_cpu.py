"""--qv without a GPU: the QV formula, the refusals (before any device call), the row struct, the usage text."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest

import helpers as H
from ntedit_amd import _lib

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")


def formula(absent, kmers, k):
    if kmers == 0:
        return float("nan")
    if absent == 0:
        return float("inf")
    return -10.0 * math.log10(1.0 - (1.0 - absent / kmers) ** (1.0 / k))


@pytest.mark.parametrize("k", [12, 25, 200])
@pytest.mark.parametrize("absent,kmers", [(0, 1000), (1000, 1000), (1, 10 ** 9), (0, 0), (5, 0), (123, 4567), (3, 10 ** 12)])
def test_qv_value(absent, kmers, k):
    lib = _lib.load()
    got, want = lib.ntedit_hip_qv_value(absent, kmers, k), formula(absent, kmers, k)
    if kmers == 0:
        assert math.isnan(got) and math.isnan(want)
    elif absent == 0:
        assert got == float("inf")
    elif absent == kmers:
        assert got == pytest.approx(0.0, abs=1e-9)  # (every k-mer wrong: error rate 1, QV 0)
    else:
        assert got == pytest.approx(want, rel=1e-12)
        assert got > 0


def test_qv_rows_as_text():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    row = _lib.QvRow(1000, 1001, 976, 30, 977, 0)
    assert lib.ntedit_hip_qv_format_row(b"ctg 1", ctypes.byref(row), 25, buf, len(buf)) == 0
    assert buf.value.decode() == "ctg 1\t1000\t1001\t976\t30\t%.2f\t977\t0\tinf\n" % formula(30, 976, 25)
    row = _lib.QvRow(10, 10, 0, 0, 0, 0)
    assert lib.ntedit_hip_qv_format_row(b"short", ctypes.byref(row), 25, buf, len(buf)) == 0
    assert buf.value.decode() == "short\t10\t10\t0\t0\tNA\t0\t0\tNA\n"
    assert lib.ntedit_hip_qv_header().decode().rstrip("\n").split("\t") == [
        "name", "len_before", "len_after", "kmers_before", "absent_before", "qv_before", "kmers_after", "absent_after", "qv_after"]
    assert lib.ntedit_hip_qv_format_row(b"x", ctypes.byref(row), 25, buf, 4) == -4  # NTEDIT_E_OVERFLOW


def test_row_struct_matches_the_header():
    """ntedit_hip_qv_row in include/ntedit_hip.h: six uint64_t in the order of the ctypes mirror"""
    text = open(os.path.join(H.ROOT, "include", "ntedit_hip.h")).read()
    body = re.search(r"typedef struct ntedit_hip_qv_row\s*\{(.*?)\}\s*ntedit_hip_qv_row;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t "), decl
            fields += [f.strip() for f in decl[len("uint64_t "):].split(",")]
    assert fields == [f for f, _ in _lib.QvRow._fields_]
    assert ctypes.sizeof(_lib.QvRow) == 48
    assert [getattr(_lib.QvRow, f).offset for f in fields] == [0, 8, 16, 24, 32, 40]
    import numpy as np
    assert np.dtype(_lib.QV_DTYPE).itemsize == 48
    stats = re.search(r"typedef struct ntedit_hip_apply_stats\s*\{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"\b(ms_\w+|pieces|bytes|events_applied)\b", stats) == [f for f, _ in _lib.ApplyStats._fields_]


def test_qv_with_shard_is_refused(tmp_path):
    draft = tmp_path / "d.fa"
    draft.write_text(">a\nACGT\n")
    r = subprocess.run([NTEDIT, "-f", str(draft), "-r", str(tmp_path / "missing.bf"), "-b", str(tmp_path / "o"), "--qv",
                        "--shard", "0/2"], capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--qv and --shard" in lines[0], r.stderr
    assert not list(tmp_path.glob("o*"))  # (nothing was written; the filter file was never looked at)


def test_run_qv_is_refused(tmp_path):
    draft = tmp_path / "d.fa"
    draft.write_text(">a\nACGT\n")
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", str(draft), "-r", str(tmp_path / "missing.bf"), "--qv"],
                       capture_output=True, text=True, cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--qv" in lines[0] and "out of scope" in lines[0], r.stderr


def test_usage_names_qv():
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert "--qv" in r.stderr + r.stdout
    assert "_qv.tsv" in r.stderr + r.stdout
