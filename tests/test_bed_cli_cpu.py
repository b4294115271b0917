"""--bed without a GPU: the flag's value, the BED row formatter (host only), the refusals (one line, before the device is
opened and before a file is written), the pinned --help and the option's own paragraph."""
import ctypes
import json
import os
import re
import subprocess
import sys

import helpers as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_cli_transcripts as R  # noqa: E402

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
HEADER = os.path.join(H.ROOT, "include", "ntedit_hip.h")


def _inputs(tmp_path):
    draft, bf = tmp_path / "d.fa", tmp_path / "f.bf"
    draft.write_text(">a\nACGT\n")
    bf.write_text("not a filter: only its being readable is looked at before the refusal\n")
    return str(draft), str(bf)


def test_flag_matches_the_header_and_overlaps_no_other():
    from ntedit_amd import _lib
    import ntedit_amd
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NTEDIT_HIP_(APPLY_[A-Z]+) (\d+)u", open(HEADER).read())}
    assert flags["APPLY_TRACK"] == 16 == _lib.APPLY_TRACK == ntedit_amd.APPLY_TRACK
    assert len(flags) == 5
    for name, value in flags.items():
        assert getattr(_lib, name) == value and value & (value - 1) == 0, name
    assert len(set(flags.values())) == len(flags)
    assert ctypes.sizeof(_lib.TrackInterval) == 16


def _row(name, entry, begin, end, absent, cap=256):
    from ntedit_amd import _lib
    lib = _lib.load()
    iv = _lib.TrackInterval(entry, begin, end, absent)
    buf = ctypes.create_string_buffer(cap)
    return lib.ntedit_hip_track_format_row(name, ctypes.byref(iv), buf, cap), buf.value


def test_format_row():
    assert _row(b"chr1 some description", 0, 5, 54, 25) == (0, b"chr1\t5\t54\t25\n")
    assert _row(b"ctg7\tlen=100 x", 3, 0, 49, 25) == (0, b"ctg7\t0\t49\t25\n")
    assert _row(b"plain", 9, 0, 2 ** 32 - 1, 2 ** 32 - 25) == (0, b"plain\t0\t4294967295\t4294967271\n")
    rc, text = _row(b"plain", 9, 4294967294, 2 ** 32 - 1, 1)
    assert rc == 0 and text.count(b"\t") == 3 and text.endswith(b"\n")
    # a buffer that is too small is refused, not overrun
    rc, _ = _row(b"a_long_sequence_name", 0, 1, 2, 3, cap=16)
    assert rc == -4


def _refused(args, tmp_path):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1, r.stderr
    assert "no usable HIP device" not in r.stderr
    assert not list(tmp_path.glob("o*"))
    return lines[0]


def test_bed_without_qv_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    line = _refused([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--bed"], tmp_path)
    assert "--bed" in line and "only with --qv" in line


def test_bed_with_shard_is_refused(tmp_path):
    """--qv --bed --shard answers what --qv --shard answers; without --qv the answer is --bed's own"""
    draft, bf = _inputs(tmp_path)
    base = [NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--qv", "--shard", "0/2"]
    a = subprocess.run(base, capture_output=True, text=True)
    b = subprocess.run(base + ["--bed"], capture_output=True, text=True)
    assert (a.returncode, a.stderr) == (b.returncode, b.stderr) and "--qv and --shard" in _refused(base + ["--bed"], tmp_path)
    line = _refused([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--bed", "--shard", "0/2"], tmp_path)
    assert "--bed" in line and "only with --qv" in line


def test_run_bed_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--bed"], capture_output=True, text=True,
                       cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--bed" in lines[0] and "one GPU" in lines[0], r.stderr
    # ... behind the older ones
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--bed", "--qv"], capture_output=True,
                       text=True, cwd=H.ROOT)
    assert r.returncode == 1 and "--qv:" in r.stderr and "--bed:" not in r.stderr


def test_help_is_the_recorded_one_and_the_option_has_its_own_paragraph():
    gold = {c["name"]: c for c in json.load(open(R.GOLDEN))["cases"]}["help"]
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (gold["status"], gold["stdout"], gold["stderr"])
    assert "--bed" not in r.stderr
    r = subprocess.run([NTEDIT, "--help-bed"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    for word in ("--bed", "--qv", "_absent_before.bed", "_absent_after.bed", "_edited.fa", "--shard", "--report", "--help-bed"):
        assert word in r.stderr, word
