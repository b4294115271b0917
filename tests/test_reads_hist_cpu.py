"""The k-mer histogram of ntedit-make-reads-bf without a GPU: the host-only summary and --solid cutoff calls (on the
demo's ntCard histogram and on hand-made arrays), the new flags' argument checks, and the library's exports."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
FIXTURE = os.path.join(H.GOLDEN, "ntcard_k25.hist")


@pytest.fixture(scope="module")
def lib():
    from ntedit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)
    return TOOL


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def cutoff(lib, f):
    """(rc, cmin) of ntedit_hip_reads_solid_cutoff on f[0..255]"""
    f = _u64(f)
    assert f.shape == (256,)
    c = ctypes.c_uint32(0)
    rc = lib.ntedit_hip_reads_solid_cutoff(f.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c))
    return rc, c.value


def summary(lib, occ):
    occ = _u64(occ)
    f = np.full(256, 7, dtype=np.uint64)  # every entry written, f[0] included
    F0, F1 = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.ntedit_hip_reads_hist_summary(occ.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(F0), ctypes.byref(F1))
    assert rc == 0
    return f, F0.value, F1.value


def read_hist(path):
    """ntCard's text histogram: ({"F1": n, "F0": n}, f[0..255] with the listed c)"""
    head, f = {}, np.zeros(256, dtype=np.uint64)
    for line in open(path):
        key, val = line.split("\t")
        if key in ("F0", "F1"):
            head[key] = int(val)
        else:
            f[int(key)] = int(val)
    return head, f


# ------------------------------------------------------------------ the --solid cutoff
def test_demo_histogram_cutoff_is_5(lib):
    head, f = read_hist(FIXTURE)
    assert head == {"F1": 105829544, "F0": 11488448}
    assert (f[4], f[5], f[6]) == (191, 63, 256)
    assert cutoff(lib, f) == (0, 5)


def test_monotone_histogram_is_refused(lib):
    f = np.arange(256, 0, -1)
    rc, _ = cutoff(lib, f)
    assert rc != 0
    assert b"valley" in lib.ntedit_hip_reads_last_error(None)
    assert cutoff(lib, np.zeros(256))[0] != 0  # flat: no strict rise anywhere


def test_valley_at_1(lib):
    f = np.zeros(256)
    f[1], f[2] = 10, 11
    assert cutoff(lib, f) == (0, 1)


def test_equal_neighbours_are_not_a_valley(lib):
    f = np.zeros(256)
    f[1:8] = [100, 50, 20, 20, 20, 10, 10]
    f[9] = 30  # f[8] = 0 < f[9]: the first strict rise is at 8
    assert cutoff(lib, f) == (0, 8)


def test_the_last_two_bins_never_give_the_cutoff(lib):
    f = np.zeros(256)
    f[1:254] = np.arange(1000, 1000 - 253, -1)
    f[254], f[255] = 0, 5  # f[255] > f[254]: a rise at 254 is not a valley ("255 or more" is not a count)
    assert cutoff(lib, f)[0] != 0
    f[254] = 1000  # a rise at 253 is
    assert cutoff(lib, f) == (0, 253)


# ------------------------------------------------------------------ F1, F0, f[c]
def test_summary_rounding_f0_f1_and_the_last_bin(lib):
    occ = np.zeros(256, dtype=np.uint64)
    occ[1], occ[2], occ[3], occ[4], occ[5] = 7, 3, 4, 2, 8
    occ[255] = 255 * 3 + 127
    f, F0, F1 = summary(lib, occ)
    want = np.zeros(256, dtype=np.uint64)
    # (occ + c/2) / c: 3/2 -> 2 (half rounds up), 4/3 -> 1, 2/4 -> 1, 8/5 -> 2, (3*255 + 127)/255 -> 3
    want[1], want[2], want[3], want[4], want[5], want[255] = 7, 2, 1, 1, 2, 3
    assert np.array_equal(f, want)
    assert F0 == 16
    assert F1 == int(occ.sum())
    occ[255] += 1  # 3*255 + 128: rounds up
    assert summary(lib, occ)[0][255] == 4


def test_summary_counts_bin_0_in_f1_only(lib):
    occ = np.zeros(256, dtype=np.uint64)
    occ[0], occ[6] = 5, 6
    f, F0, F1 = summary(lib, occ)
    assert f[0] == 0 and f[6] == 1 and F0 == 1 and F1 == 11


def test_summary_matches_the_definition_on_random_arrays(lib):
    rng = np.random.default_rng(1)
    for _ in range(5):
        occ = rng.integers(0, 1 << 40, 256).astype(np.uint64)
        f, F0, F1 = summary(lib, occ)
        c = np.arange(1, 256, dtype=np.uint64)
        want = (occ[1:] + c // np.uint64(2)) // c
        assert f[0] == 0 and np.array_equal(f[1:], want)
        assert F0 == int(want.sum()) and F1 == int(occ.sum())


def test_host_calls_refuse_null_arguments(lib):
    f = _u64(np.zeros(256))
    assert lib.ntedit_hip_reads_solid_cutoff(f.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.ntedit_hip_reads_solid_cutoff(None, ctypes.byref(ctypes.c_uint32())) != 0
    assert lib.ntedit_hip_reads_hist_summary(None, f.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ctypes.c_uint64()),
                                             ctypes.byref(ctypes.c_uint64())) != 0


# ------------------------------------------------------------------ the library
def test_library_exports_the_histogram_calls(lib):
    from ntedit_amd import _lib
    for s in ("ntedit_hip_sketch_histogram", "ntedit_hip_sketch_histogram_download", "ntedit_hip_reads_hist_summary",
              "ntedit_hip_reads_solid_cutoff"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    # a null context is an argument error, not a crash
    occ = _u64(np.zeros(256))
    assert lib.ntedit_hip_sketch_histogram(None, b"ACGT", 4, 0) != 0
    assert lib.ntedit_hip_sketch_histogram_download(None, occ.ctypes.data_as(ctypes.c_void_p)) != 0


# ------------------------------------------------------------------ the CLI
@pytest.fixture()
def reads(tmp_path):
    f = tmp_path / "r.fq"
    f.write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return str(f)


def _run(tool, *args, cwd=None):
    return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


def test_help_lists_solid_and_hist(tool):
    r = _run(tool, "--help")
    assert r.returncode == 0
    assert "--solid" in r.stderr and "--hist" in r.stderr
    # the cutoff rule is the tool's own
    assert "ntCard" in r.stderr and "f[c+1] > f[c]" in r.stderr


@pytest.mark.parametrize("args,message", [
    (["-k", "25", "--solid", "-c", "2", "--bf", "4096"], "--solid and -c"),
    (["-k", "25", "--solid", "-c", "2"], "--solid and -c"),
    (["-k", "25", "--bf", "4096"], "-c: required"),
    (["-k", "25", "--hist", "h.txt"], "-c: required"),
    (["-k", "25", "-c", "2"], "--bf or --num_elements"),
    (["-k", "25", "-c", "2", "--counts"], "--bf or --num_elements"),
    (["-k", "25", "--solid", "--hist"], "Too few arguments"),
])
def test_bad_histogram_arguments_are_refused(tool, reads, tmp_path, args, message):
    out = tmp_path / "o.bf"
    r = _run(tool, "--reads", reads, "-o", str(out), *args, cwd=str(tmp_path))
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fq"]


def test_refusal_without_a_size_names_the_histogram_flags(tool, reads):
    r = _run(tool, "--reads", reads, "-k", "25", "-c", "2")
    assert r.returncode != 0 and "--solid" in r.stderr.splitlines()[0]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
@pytest.mark.parametrize("args", [
    ["--solid"],
    ["--solid", "--counts"],
    ["-c", "2"],
])
def test_sizing_from_the_histogram_passes_the_checks_then_fails_without_a_device(tool, reads, tmp_path, args):
    out = tmp_path / "o.bf"
    r = _run(tool, "--reads", reads, "-k", "25", "-o", str(out), "--hist", str(tmp_path / "h.txt"), *args,
             cwd=str(tmp_path))
    assert r.returncode != 0 and "error" in r.stderr, r.stderr
    assert "Usage" not in r.stderr  # past the argument checks
    assert "BF size (bytes): from the k-mer histogram" in r.stdout
    # the default sketch when sized from the histogram: one counter per input byte, at least 64 MiB
    assert "Sketch size (counters): %d" % (64 << 20) in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["r.fq"]
