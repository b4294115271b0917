"""nte_tile.h (ntedit_amd/csrc) on the CPU: tests/tile/tile_host.cpp plays the 256 threads of a workgroup one after the
other -- every tile staged, then walked by the byte reader and by the four-start reader -- and compares every start's
(valid, fh + rh) with a direct computation, for k in 12, 13, 14, 15, 25, 64, 65, 199, 200, 255, 256 (all four residues
of k % 4 and the halo's limit), both look-up rules, batches of 0, 1, k - 1, k, 16384, 16384 + k - 1, 16384 + k and
2 * 16384 + 5 bytes with N, R, lower case and a newline at the tile's, the halo's and a stream's ends, and two poison
codes under the staging; then the entry cursor against a linear scan, entry_behind, bit_range and byte_sat_inc.  No GPU."""
import os
import re
import subprocess

import pytest

import helpers as H

_SRC = os.path.join(H.ROOT, "tests", "tile", "tile_host.cpp")
KS = [12, 13, 14, 15, 25, 64, 65, 199, 200, 255, 256]


def build_tile_host(out_dir, sanitize=False):
    """g++ build of the host program (as settle_case.build_settle_host); returns its path"""
    exe = os.path.join(out_dir, "tile_host_san" if sanitize else "tile_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, _SRC], check=True)
    return exe


def check(text):
    rows = re.findall(r"^k (\d+): starts (\d+) valid (\d+) mismatches (\d+)$", text, re.M)
    assert [int(r[0]) for r in rows] == KS
    for k, starts, valid, mismatches in ((int(x) for x in r) for r in rows):
        # 8 batch lengths in 1, 1, 1, 1, 1, 2, 2, 3 tiles and three more plantings of the longest, under two look-up rules
        assert starts == (12 + 3 * 3) * 16384 * 2 and mismatches == 0
        # the starts of the long batches are k-mers but for the planted bytes: 11 of the 21 tiles, less k per planted byte
        assert starts // 3 < valid < starts * 11 // 21
    m = re.search(r"^starts (\d+) valid (\d+) mismatches (\d+)\s*$", text.strip().splitlines()[-1])
    assert m and int(m.group(3)) == 0 and int(m.group(1)) == sum(int(r[1]) for r in rows)


def test_walk_and_entries_equal_the_direct_computation(tmp_path):
    r = subprocess.run([build_tile_host(str(tmp_path)), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    check(r.stdout)


def test_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own: no read or write leaves the LDS array,
    the batch or the tables"""
    r = subprocess.run([build_tile_host(str(tmp_path), sanitize=True), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    check(r.stdout)
