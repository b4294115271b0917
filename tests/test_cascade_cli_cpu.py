"""`ntedit --reads -k K1,K2,...` (a cascade of polishing rounds) without a GPU: every refusal of a list of k happens
before the device is opened and before any file is written; the {k} of the saved files' names; the multi-GPU driver
refuses a list; and the ctypes mirrors of the two build structs have the header's sizes."""
import ctypes
import os
import subprocess

import pytest

import helpers as H

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
HOST = os.path.join(H.ROOT, "ntedit_amd", "host")
NO_DEVICE = "no usable HIP device"


@pytest.fixture(scope="module")
def ntedit():
    if not os.path.exists(NTEDIT):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return NTEDIT


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "d.fa").write_text(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    (tmp_path / "r.fq").write_text("@r1\n" + "ACGTACGTAC" * 5 + "\n+\n" + "I" * 50 + "\n")
    (tmp_path / "f.bf").write_text("not a filter\n")
    return tmp_path


def _run(ntedit, args, cwd):
    return subprocess.run([ntedit] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


READS = ["-f", "d.fa", "--reads", "r.fq", "--cutoff", 2, "--bf", 4096]
REFUSALS = {
    "with -r": (["-f", "d.fa", "-r", "f.bf", "-k", "40,30", "-b", "p"], "-k 40,30: a list of k", "only with --reads"),
    "with --genome": (["-f", "d.fa", "--genome", "d.fa", "-k", "40,30", "-b", "p"], "-k 40,30: a list of k",
                      "only with --reads"),
    "without -b": (READS + ["-k", "40,30"], "-k 40,30: a list of k needs -b", None),
    "not a number": (READS + ["-k", "40,x", "-b", "p"], "-k 40,x: k must be between 12 and 200", "`x'"),
    "an empty k": (READS + ["-k", "40,,30", "-b", "p"], "-k 40,,30: k must be between 12 and 200", "`'"),
    "a trailing comma": (READS + ["-k", "40,", "-b", "p"], "-k 40,: k must be between 12 and 200", None),
    "a negative k": (READS + ["-k", "40,-30", "-b", "p"], "k must be between 12 and 200", "`-30'"),
    "k below 12": (READS + ["-k", "40,11", "-b", "p"], "k must be between 12 and 200", "`11'"),
    "k above 200": (READS + ["-k", "201,40", "-b", "p"], "k must be between 12 and 200", "`201'"),
    "a k twice": (READS + ["-k", "40,30,40", "-b", "p"], "k = 40 is given twice", None),
    "nine k": (READS + ["-k", "12,13,14,15,16,17,18,19,20", "-b", "p"], "at most 8 k in a list", "9 given"),
    "with --shard": (["-f", "d.fa", "--reads", "r.fq", "--cutoff", 2, "--bf", 4096, "-k", "40,30", "-b", "p",
                      "--shard", "0/2"], "-k 40,30 and --shard", None),
    "--save_bf without {k}": (READS + ["-k", "40,30", "-b", "p", "--save_bf", "f_k.bf"],
                              "--save_bf f_k.bf: with a list of k the name needs {k}", None),
    "--save_reject_bf without {k}": (READS + ["-k", "40,30", "-b", "p", "--reject_cutoff", 9, "--reject_bf", 4096,
                                              "--save_bf", "f_{k}.bf", "--save_reject_bf", "rej.bf"],
                                     "--save_reject_bf rej.bf: with a list of k the name needs {k}", None),
    "--hist without {k}": (READS + ["-k", "40,30", "-b", "p", "--hist", "h.hist"],
                           "--hist h.hist: with a list of k the name needs {k}", None),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_list_of_k_is_refused_before_the_device_is_opened(ntedit, inputs, name):
    args, message, detail = REFUSALS[name]
    before = sorted(os.listdir(inputs))
    r = _run(ntedit, args, inputs)
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr and (detail is None or detail in r.stderr), r.stderr
    assert NO_DEVICE not in r.stderr
    assert sorted(os.listdir(inputs)) == before


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks where the run fails without a device")
def test_a_good_list_reaches_the_device(ntedit, inputs):
    """what none of the rules refuses goes on to open the device: eight k, {k} in every name"""
    r = _run(ntedit, READS + ["-k", "40,30,25,24,23,22,21,20", "-b", "p", "--save_bf", "f_{k}.bf", "--hist", "{k}.hist"],
             inputs)
    assert r.returncode == 1 and NO_DEVICE in r.stderr, r.stderr
    # ... and so does a single k, whose names are taken as they are
    r = _run(ntedit, READS + ["-k", 25, "--save_bf", "f.bf"], inputs)
    assert r.returncode == 1 and NO_DEVICE in r.stderr, r.stderr


def _compile_and_run(tmp_path, source):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(source)
    subprocess.run(["c++", "-std=c++17", "-I", os.path.join(H.ROOT, "include"), "-I", HOST, "-o", str(exe), str(src)],
                   check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


def test_k_replaces_every_k_in_braces(tmp_path):
    out = _compile_and_run(tmp_path, """#include "k_list.h"
#include <cstdio>
int main() {
    for (const char* n : { "f_{k}.bf", "{k}", "a{k}/b_{k}_{k}.hist", "none.bf", "{K}{k" })
        printf("%s\\n", nte_host::with_k(n, 40).c_str());
    std::vector<std::string> ks;
    printf("[%s]\\n", nte_host::k_list_rules("040,30,25", true, false, true, { { "--save_bf", "x_{k}" } }, &ks).c_str());
    for (const std::string& k : ks) printf("%s\\n", k.c_str());
}
""")
    assert out.splitlines() == ["f_40.bf", "40", "a40/b_40_40.hist", "none.bf", "{K}{k", "[]", "40", "30", "25"]


def test_the_multi_gpu_driver_refuses_a_list_of_k(inputs):
    from ntedit_amd import run
    from ntedit_amd.make_reads import Refused
    with pytest.raises(Refused, match="-k 40,30: a list of k"):
        run.parse(["-f", str(inputs / "d.fa"), "--reads", str(inputs / "r.fq"), "-k", "40,30", "--cutoff", "2",
                   "--bf", "4096", "-b", "p"])
    # (a single k still parses)
    args = run.parse(["-f", str(inputs / "d.fa"), "--reads", str(inputs / "r.fq"), "-k", "25", "--cutoff", "2",
                      "--bf", "4096"])
    assert args.reads_args["k"] == 25


def test_the_build_structs_have_the_headers_sizes(tmp_path):
    from ntedit_amd import _lib
    out = _compile_and_run(tmp_path, """#include "ntedit_hip.h"
#include <cstdio>
#include <cstddef>
int main() { printf("%zu %zu %zu %zu %zu\\n", sizeof(ntedit_hip_reads_build_args), sizeof(ntedit_hip_reads_build_result),
                    offsetof(ntedit_hip_reads_build_args, min_read), offsetof(ntedit_hip_reads_build_args, keep_store),
                    offsetof(ntedit_hip_reads_build_result, from_store)); }
""")
    want = [ctypes.sizeof(_lib.ReadsBuildArgs), ctypes.sizeof(_lib.ReadsBuildResult), _lib.ReadsBuildArgs.min_read.offset,
            _lib.ReadsBuildArgs.keep_store.offset, _lib.ReadsBuildResult.from_store.offset]
    assert [int(x) for x in out.split()] == want
