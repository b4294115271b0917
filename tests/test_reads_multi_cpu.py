"""The sharded reads filter build without a GPU: the partition (ntedit_amd.make_reads.plan), the byte-range reader behind
ntedit_hip_reads_pass (through the host-only ntedit_hip_reads_range_text), the cut-point check, and the driver's
argument refusals, which match ntedit-make-reads-bf's."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")
WHOLE = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    from ntedit_amd import _lib
    return _lib.load()


def range_reads(lib, path, begin, end):
    """(reads, start, next) of one range"""
    n, count, start, nxt = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    cap = os.path.getsize(path) + 64
    buf = ctypes.create_string_buffer(cap)
    rc = lib.ntedit_hip_reads_range_text(str(path).encode(), begin, end, buf, cap, ctypes.byref(n), ctypes.byref(count),
                                         ctypes.byref(start), ctypes.byref(nxt))
    assert rc == 0, lib.ntedit_hip_reads_last_error(None)
    reads = buf.raw[:n.value].split(b"\n")[:-1]
    assert len(reads) == count.value
    return reads, start.value, nxt.value


SMALL = {
    "fasta": b">r1 one\nACGTACGTAC\nGGTTA\n>r2\n\n>r3\nTTTT\n>r4\nACGTNNACGT\n",
    "fastq": b"@r1\nACGTACGTAC\n+\n@IIIIIIIII\n@r2\nGG\n+r2\n>I\n@r3\n\n+\n\n@r4\nTTTTCAGT\n+\nIIIIIIII\n",
    "crlf": b">r1\r\nACGTAC\r\nGT\r\n>r2\r\nTTTT\r\n@r3\r\nCCCC\r\n+\r\nIIII\r\n",
    "preamble": b"some text first\nmore\n>r1\nACGT\n>r2\nCCGG\n",
    "no_newline": b">r1\nACGT\n>r2\nCCGGTT",
    "fastq_no_newline": b"@r1\nACGT\n+\nIIII\n@r2\nCC\n+\nII",
    "empty": b"",
    "short_reads": b">a\nA\n>b\nC\n>c\n\n>d\nG\n",
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_two_ranges_at_every_cut_read_the_whole_file(lib, tmp_path, name):
    p = tmp_path / (name + ".txt")
    p.write_bytes(SMALL[name])
    size = len(SMALL[name])
    whole, _, _ = range_reads(lib, p, 0, WHOLE)
    for cut in range(size + 1):
        r0, s0, n0 = range_reads(lib, p, 0, cut)
        r1, s1, n1 = range_reads(lib, p, cut, size)
        assert s0 == 0
        assert n0 == s1, (cut, n0, s1)
        assert r0 + r1 == whole, cut


def test_three_ranges_at_every_pair_of_cuts(lib, tmp_path):
    data = SMALL["fastq"] + b"@r5\nACGTTT\n+\nIIIIII\n"
    p = tmp_path / "r.fq"
    p.write_bytes(data)
    whole, _, _ = range_reads(lib, p, 0, WHOLE)
    assert len(whole) == 5
    for a in range(0, len(data) + 1, 3):
        for b in range(a, len(data) + 1, 5):
            parts = [range_reads(lib, p, x, y) for x, y in ((0, a), (a, b), (b, len(data)))]
            assert parts[0][2] == parts[1][1] and parts[1][2] == parts[2][1]
            assert parts[0][0] + parts[1][0] + parts[2][0] == whole


def test_multiline_fastq_can_break_a_cut_and_the_check_sees_it(lib, tmp_path):
    """a quality line that starts with '@' two lines above a '+' looks like a record start"""
    data = b"@r1\nACGT\nACGT\n+\n@II\nII\n+II\n@r2\nCCCC\n+\nIIII\n"
    p = tmp_path / "m.fq"
    p.write_bytes(data)
    whole, _, _ = range_reads(lib, p, 0, WHOLE)
    assert whole == [b"ACGTACGT", b"CCCC"]
    broken = 0
    for cut in range(1, len(data)):
        r0, _, n0 = range_reads(lib, p, 0, cut)
        r1, s1, _ = range_reads(lib, p, cut, len(data))
        if n0 == s1:
            assert r0 + r1 == whole
        else:
            broken += 1
    assert broken > 0


def test_gzip_files_are_not_cut(lib, tmp_path):
    p = tmp_path / "r.fq.gz"
    with gzip.open(p, "wb") as f:
        f.write(SMALL["fastq"])
    assert lib.ntedit_hip_reads_is_gzip(str(p).encode()) == 1
    reads, _, _ = range_reads(lib, p, 0, WHOLE)
    assert len(reads) == 4
    n = ctypes.c_uint64()
    rc = lib.ntedit_hip_reads_range_text(str(p).encode(), 5, 40, None, 0, ctypes.byref(n), ctypes.byref(n),
                                         ctypes.byref(n), ctypes.byref(n))
    assert rc != 0 and b"gzip" in lib.ntedit_hip_reads_last_error(None)


# ------------------------------------------------------------------ planner
def _facts(sizes_gz):
    return [(n, gz) for n, gz in sizes_gz]


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_plan_covers_every_byte_once_and_keeps_gzip_whole(world):
    from ntedit_amd.make_reads import WHOLE as W, plan
    facts = _facts([(1000, False), (333, True), (1, False), (0, False), (98765, False), (4000, True)])
    paths = ["f%d" % i for i in range(len(facts))]
    units, owner = plan(paths, facts, world)
    again = plan(paths, facts, world)
    assert [(u.file, u.begin, u.end) for u in units] == [(u.file, u.begin, u.end) for u in again[0]]
    assert owner == again[1]
    assert all(0 <= o < world for o in owner)
    for i, (n, gz) in enumerate(facts):
        mine = sorted((u.begin, u.end) for u in units if u.file == i)
        if gz or world == 1 or n == 0:
            assert mine == [(0, W)]
            continue
        if mine == [(0, W)]:
            continue
        assert mine[0][0] == 0 and mine[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
        assert all(a < b for a, b in mine)
    loads = [sum(u.weight for u, o in zip(units, owner) if o == r) for r in range(world)]
    assert sum(loads) == sum(n * (4 if gz else 1) for n, gz in facts)
    assert max(loads) - min(loads) <= max(u.weight for u in units)


def test_plan_no_split_keeps_every_file_whole():
    from ntedit_amd.make_reads import WHOLE as W, plan
    units, _ = plan(["a", "b"], [(10000, False), (20000, False)], 4, split=False)
    assert [(u.begin, u.end) for u in units] == [(0, W), (0, W)]


def test_check_cuts():
    from ntedit_amd.make_reads import check_cuts
    ok = [(0, 0, 0, 50), (0, 40, 50, 90), (0, 80, 90, 100), (1, 0, 0, 7)]
    assert check_cuts(ok) is None
    assert check_cuts(list(reversed(ok))) is None
    assert check_cuts([(0, 0, 0, 50), (0, 40, 48, 90)]) == (0, 0, 40, 50, 48)
    assert check_cuts([(0, 0, 0, WHOLE), (0, 40, 48, 90)]) is not None


# ------------------------------------------------------------------ sizing through the library
def test_sizing_calls_match_the_binary_rules(lib, tmp_path):
    from ntedit_amd.make_reads import parse, sizes
    import math
    want = int(math.ceil(1000000 * (-3 / math.log(1 - math.exp(math.log(0.01) / 3)))) / 8)
    assert lib.ntedit_hip_reads_bf_size(1000000, 3, 0.01) == want
    plain, gz = tmp_path / "a.fa", tmp_path / "b.fq.gz"
    plain.write_bytes(b">r\nACGT\n" * 10_000_000)
    with gzip.open(gz, "wb") as f:
        f.write(b"@r\nACGT\n+\nIIII\n" * 1000)
    files = (ctypes.c_char_p * 2)(str(plain).encode(), str(gz).encode())
    assert lib.ntedit_hip_reads_default_sketch(files, 2, 0) == 80_000_000 + 4 * os.path.getsize(gz)
    assert lib.ntedit_hip_reads_default_sketch(files, 2, 1 << 20) == 64 << 20
    assert lib.ntedit_hip_reads_default_sketch(files, 2, 1 << 30) == 16 << 30
    assert lib.ntedit_hip_reads_default_sketch(files, 2, 1 << 40) == 32 << 30
    a = parse(["--reads", str(plain), "-k", "25", "-c", "2", "--num_elements", "1000000"])
    assert sizes(lib, a) == (want, max(want * 16, 64 << 20))


def test_hist_writer(lib, tmp_path):
    f = np.arange(256, dtype=np.uint64)
    p = tmp_path / "h.hist"
    assert lib.ntedit_hip_reads_write_hist(str(p).encode(), f.ctypes.data_as(ctypes.c_void_p), 7, 9) == 0
    lines = p.read_text().splitlines()
    assert lines[:3] == ["F1\t9", "F0\t7", "1\t1"] and lines[-1] == "255\t255" and len(lines) == 257


# ------------------------------------------------------------------ the driver's refusals: the binary's
@pytest.fixture()
def reads(tmp_path):
    f = tmp_path / "r.fq"
    f.write_text("@r1\nACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return str(f)


def _driver(*args):
    return subprocess.run([sys.executable, "-m", "ntedit_amd.make_reads"] + list(args), capture_output=True, text=True,
                          timeout=120, cwd=H.ROOT)


@pytest.mark.parametrize("args", [
    ["-k", "11", "-c", "2", "--bf", "4096"],
    ["-k", "201", "-c", "2", "--bf", "4096"],
    ["-k", "x25", "-c", "2", "--bf", "4096"],
    ["-c", "2", "--bf", "4096"],
    ["-k", "25", "-c", "0", "--bf", "4096"],
    ["-k", "25", "-c", "256", "--bf", "4096"],
    ["-k", "25", "--bf", "4096"],
    ["-k", "25", "-c", "2", "--hashes", "9", "--bf", "4096"],
    ["-k", "25", "-c", "2"],
    ["-k", "25", "-c", "2", "--bf", "0"],
    ["-k", "25", "-c", "2", "--num_elements", "0"],
    ["-k", "25", "-c", "2", "--bf", "4096", "--bogus"],
    ["-k", "25", "--solid", "-c", "3"],
    ["-k", "25", "-c", "2", "--fpr", "1.5", "--bf", "4096"],
    ["-k", "25", "-c", "2", "--bf"],
])
def test_driver_refusals_are_the_binarys(reads, tmp_path, args):
    out = tmp_path / "o.bf"
    full = ["--reads", reads, "-o", str(out)] + args
    r = _driver(*full)
    t = subprocess.run([TOOL] + full, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and t.returncode != 0
    assert r.stderr.splitlines()[0] == t.stderr.splitlines()[0], (r.stderr, t.stderr)
    assert not out.exists()


def test_driver_no_reads_is_refused():
    r = _driver("-k", "25", "-c", "2", "--bf", "4096")
    assert r.returncode != 0 and "--reads: 1 or more" in r.stderr


def test_driver_help_names_its_own_flags():
    r = _driver("--help")
    assert r.returncode == 0 and "--no-split" in r.stderr and "--backend" in r.stderr


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the failure without a device")
def test_driver_without_a_device_fails_and_writes_nothing(reads, tmp_path):
    out = tmp_path / "o.bf"
    r = _driver("--reads", reads, "-k", "25", "-c", "2", "--bf", "4096", "-o", str(out))
    assert r.returncode != 0 and "no HIP device" in r.stderr
    assert not out.exists()
