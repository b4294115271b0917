"""settle_event() (ntedit_amd/csrc/nte_settle.h) against the event machine, on the CPU: tests/settle/settle_host.cpp runs
every event of its planted and seeded random cases through MachineT::run + finish and through settle_event(); wherever
settle_event() accepts, the four items, the cover end and the flags are the machine's byte for byte, and a decline
writes nothing.  No GPU."""
import re
import subprocess

import pytest

import settle_case as S


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return S.build_settle_host(str(tmp_path_factory.mktemp("settle")))


@pytest.fixture(scope="module")
def selftest(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_settled_events_equal_the_machine(selftest):
    """planted cases (two substitutions at every distance 1 .. 2k + 2; one at every distance from a contig's end and
    start, contigs of 2k .. 4k bases; a lower-case error base, N / IUPAC codes at every window offset; decoy candidates
    in front of and behind the true base, with their own k-mer only and fully supported; exactly one missing k-mer
    start + i, i = 1 .. k) and seeded random drafts, for k in 12, 25, 32, 33, 64 x jump 1, 3 x h 1, 3, 4, start grids
    256 and 4, filters of 100003 bytes and of 2^17"""
    events, settled, mismatches = S.tally(selftest)
    assert mismatches == 0
    assert events > 400000 and settled > 30000
    rows = re.findall(r"^k (\d+) jump (\d+) h (\d+) grid (\d+) filter (\d+) bytes: events (\d+) settled (\d+) mismatches 0$", selftest, re.M)
    assert len(rows) == 5 * 2 * 3 * 2
    assert {int(r[0]) for r in rows} == {12, 25, 32, 33, 64} and {int(r[3]) for r in rows} == {256, 4}
    assert all(int(r[6]) > 0 for r in rows)  # every parameter set settles some events and sends some to the machine
    assert all(int(r[5]) > int(r[6]) for r in rows)


def test_iid_case_settles_most_events(selftest):
    """2 Mbp i.i.d., 0.5 % substitutions, 0.05 % indels, k = 25, h = 3: the program reports 7,453 of 10,414 events
    settled, a share of 0.7157 (the others: indels, errors within 2k of each other or of a contig's end)"""
    m = re.search(r"^iid: events (\d+) settled (\d+) mismatches 0 share ([0-9.]+)$", selftest, re.M)
    assert m, selftest[-600:]
    assert int(m.group(2)) * 2 >= int(m.group(1))


def test_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own"""
    exe = S.build_settle_host(str(tmp_path), sanitize=True)
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    assert S.tally(r.stdout)[2] == 0
