"""The HIP-free parts of ntedit_amd/csrc/nte_reads_unit.h and the two host helpers of nte_reads_grammar.h on the CPU:
tests/unit/unit_host.cpp holds the checks (the per-context registry, alone and under eight threads; Keep untouched by
`scr = Scratch()`; rp_make_filter against the three inline tests it replaced; rp_counts_add; the carver), built plain,
with -fsanitize=address,undefined and with -fsanitize=thread, as test_feed_cpu.py builds its program.  No GPU, nothing
of the library linked."""
import os
import subprocess

import pytest

import helpers as H

_SRC = os.path.join(H.ROOT, "tests", "unit", "unit_host.cpp")
_FLAGS = {"plain": ["-O2"],
          "asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "tsan": ["-O1", "-g", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(_FLAGS))
def exe(request, tmp_path_factory):
    """g++ build of the host program, once per flavour"""
    out = str(tmp_path_factory.mktemp("unit") / ("unit_host_" + request.param))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + _FLAGS[request.param] + ["-o", out, _SRC], check=True)
    return out


@pytest.mark.parametrize("what", ["registry", "threads", "scratch", "filter", "counts", "carver"])
def test_unit_parts(exe, what):
    """one check of the program; any sanitizer report fails it (a report ends the program with a non-zero status)"""
    r = subprocess.run([exe, what], capture_output=True, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (what, r.returncode, r.stdout[-2000:], err[-4000:])
    assert r.stdout.decode().splitlines() == ["ok"]


def test_the_program_knows_its_checks(exe):
    """a name it does not know is refused, so a check that was renamed away cannot pass by running nothing"""
    assert subprocess.run([exe, "no such check"], capture_output=True, timeout=120).returncode == 2
