"""nte_probe_draw.h (ntedit_amd/csrc) on the CPU: tests/draw/draw_host.cpp enumerates the probe stage's draw coordinates --
for 1, 7, 11 and 256 runs per slice and longest runs of 0, 1, 511, 512, 513 and 17,184 records every (run, step below the
bound) is handed out exactly once, nothing beyond it, and the one draw that closes the slice is the last, also for a slice
without a record -- and plays probe_claim_try's order of events with 1 to 64 simulated workgroups on two XCD ids over lists
of slices that include empty ones, whole and in 2 and 4 parts: every unit once, and every workgroup comes to an end.
No GPU."""
import os
import re
import subprocess

import helpers as H

_SRC = os.path.join(H.ROOT, "tests", "draw", "draw_host.cpp")


def build_draw_host(out_dir, sanitize=False):
    """g++ build of the host program (as test_tile_cpu.build_tile_host); returns its path"""
    exe = os.path.join(out_dir, "draw_host_san" if sanitize else "draw_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, _SRC], check=True)
    return exe


def check(text):
    coords = re.findall(r"^coords n_wg (\d+) longest (\d+): draws (\d+) units (\d+) mismatches (\d+)$", text, re.M)
    assert [(int(r[0]), int(r[1])) for r in coords] == [(w, l) for w in (1, 7, 11, 256) for l in (0, 1, 511, 512, 513, 17184)]
    for n_wg, longest, draws, units, mismatches in ((int(x) for x in r) for r in coords):
        steps = max(1, -(-longest // 512))
        assert units == n_wg * steps and draws == -(-units // 8) and mismatches == 0
    claims = re.findall(r"^claim slices (\d+) parts (\d+) n_wg (\d+) workgroups (\d+): units (\d+) handed (\d+) events (\d+) "
                        r"waits (\d+) mismatches (\d+)$", text, re.M)
    assert len(claims) == 4 * (3 * 4 + 2)
    for slices, parts, n_wg, workgroups, units, handed, events, waits, mismatches in ((int(x) for x in r) for r in claims):
        assert handed == units and mismatches == 0
        assert units >= slices * parts * n_wg  # (a pair without a record hands out one step of every run)
    assert text.strip().splitlines()[-1] == "mismatches 0"


def test_coordinates_and_claims(tmp_path):
    r = subprocess.run([build_draw_host(str(tmp_path)), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    check(r.stdout)


def test_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own: no index leaves the control words"""
    r = subprocess.run([build_draw_host(str(tmp_path), sanitize=True), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-6000:]
    check(r.stdout)
