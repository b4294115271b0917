"""--bgzip without a GPU: the two refusals (one line, before the device is opened and before a file is written), the
pinned --help, and the option's own paragraph."""
import json
import os
import subprocess
import sys

import helpers as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_cli_transcripts as R  # noqa: E402

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")


def _inputs(tmp_path):
    draft, bf = tmp_path / "d.fa", tmp_path / "f.bf"
    draft.write_text(">a\nACGT\n")
    bf.write_text("not a filter: only its being readable is looked at before the refusal\n")
    return str(draft), str(bf)


def test_bgzip_with_shard_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    r = subprocess.run([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--bgzip", "--shard", "0/2"],
                       capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--bgzip and --shard" in lines[0], r.stderr
    assert "no usable HIP device" not in r.stderr
    assert not list(tmp_path.glob("o*"))


def test_older_refusals_come_first(tmp_path):
    """--qv --shard --bgzip answers what --qv --shard answers"""
    draft, bf = _inputs(tmp_path)
    base = [NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--qv", "--shard", "0/2"]
    a = subprocess.run(base, capture_output=True, text=True)
    b = subprocess.run(base + ["--bgzip"], capture_output=True, text=True)
    assert (a.returncode, a.stderr) == (b.returncode, b.stderr) and "--qv and --shard" in a.stderr


def test_run_bgzip_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--bgzip"], capture_output=True, text=True,
                       cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--bgzip" in lines[0] and "one GPU" in lines[0], r.stderr
    # ... behind the older ones
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--bgzip", "--qv"], capture_output=True,
                       text=True, cwd=H.ROOT)
    assert r.returncode == 1 and "--qv" in r.stderr and "--bgzip" not in r.stderr


def test_help_is_the_recorded_one_and_the_option_has_its_own_paragraph():
    gold = {c["name"]: c for c in json.load(open(R.GOLDEN))["cases"]}["help"]
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (gold["status"], gold["stdout"], gold["stderr"])
    assert "--bgzip" not in r.stderr
    r = subprocess.run([NTEDIT, "--help-bgzip"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    for word in ("--bgzip", "_edited.fa.gz", "BGZF", "--shard", "--report"):
        assert word in r.stderr, word
