"""The packed tile of nte_tile.h (two 4-bit codes per byte, 32 starts per thread) on the CPU:
tests/tile/tile_packed_host.cpp plays the 1,024 threads of a partition workgroup through tile_stage_packed,
tile_prime_packed and the eight-start reader, and compares every start's (valid, fh + rh) with the byte walk's, for
k in 1, 7, 8, 9, 25, 31, 32, 33, 255, 256 (every kind of k mod 8 and the halo's limit), both look-up rules, batches of
k - 1 and k bytes, batches that end inside a tile, at a tile's end and with a halo, streams with N runs, IUPAC codes,
lower case and separators at the tile's, the halo's, a stream's and a word's ends, and two poison codes under the
staging.  No GPU."""
import os
import re
import subprocess

import helpers as H

_SRC = os.path.join(H.ROOT, "tests", "tile", "tile_packed_host.cpp")
KS = [1, 7, 8, 9, 25, 31, 32, 33, 255, 256]


def build_host(out_dir, sanitize=False):
    exe = os.path.join(out_dir, "tile_packed_host_san" if sanitize else "tile_packed_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, _SRC], check=True)
    return exe


def check(text):
    rows = re.findall(r"^k (\d+): starts (\d+) valid (\d+) mismatches (\d+)$", text, re.M)
    assert [int(r[0]) for r in rows] == KS
    for k, starts, valid, mismatches in ((int(x) for x in r) for r in rows):
        # 6 batch lengths in 1, 1, 1, 1, 2, 3 tiles (k = 1: the empty batch is one tile too) and four more plantings of a
        # two-tile batch, under two look-up rules
        assert starts == (9 + 4 * 2) * 32768 * 2 - (2 * 32768 if k == 1 else 0) and mismatches == 0
        assert starts // 3 < valid < starts * 2 // 3
    m = re.search(r"^starts (\d+) valid (\d+) mismatches (\d+)\s*$", text.strip().splitlines()[-1])
    assert m and int(m.group(3)) == 0 and int(m.group(1)) == sum(int(r[1]) for r in rows)


def test_packed_walk_equals_the_byte_walk(tmp_path):
    r = subprocess.run([build_host(str(tmp_path)), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    check(r.stdout)


def test_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own: no read or write leaves the LDS array or
    the batch"""
    r = subprocess.run([build_host(str(tmp_path), sanitize=True), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    check(r.stdout)
