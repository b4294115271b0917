"""`ntedit` command lines that end before the device is opened, replayed against the built binary: exit status, stdout and
stderr equal, whole, what the build before the command line was split into units (cli_options.cpp, ...) answered.  The
expected values were recorded from that build by tests/tools/record_cli_transcripts.py and are never taken from the build
under test: where a case differs, the code is wrong."""
import json
import os
import subprocess
import sys

import pytest

import helpers as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_cli_transcripts as R  # noqa: E402

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
GOLD = json.load(open(R.GOLDEN))["cases"]


@pytest.fixture(scope="module")
def ntedit():
    if not os.path.exists(NTEDIT):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return NTEDIT


@pytest.fixture(scope="module")
def where(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli"))
    R.make_inputs(d)
    return d


def test_the_fixture_holds_the_recorders_list():
    assert len(GOLD) >= 60
    assert [(c["name"], c["args"]) for c in GOLD] == [(n, a) for n, a in R.CASES.items()]
    # (only command lines that end before the device is opened: the fixture reads the same on a GPU machine)
    assert not any("no usable HIP device" in c["stderr"] for c in GOLD)
    assert {c["status"] for c in GOLD} == {0, 1}


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_the_transcript_is_the_recorded_one(ntedit, where, case):
    got = R.transcript(ntedit, case["args"], where)
    assert got["stderr"] == case["stderr"]
    assert got["stdout"] == case["stdout"]
    assert got["status"] == case["status"]
