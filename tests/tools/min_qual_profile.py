"""Measurements of DESIGN.md 9.19 (--min_qual): one synthetic set of 150-base reads with qualities (a 3' tail of low
qualities per read, one base in a hundred anywhere), as plain FASTQ and as BAM, through ntedit-make-reads-bf --gpu_parse in
one session of alternating runs: a parent build's tool when one is given (--parent_tool), this tree's without the flag, this
tree's with --min_qual 20.  Per run the tool's own lines: milliseconds in the parse kernels (FASTQ), in the BAM decode
kernels, the passes, and what was masked.  Writes the record as JSON.

    python tests/tools/min_qual_profile.py --out profiles/min_qual.json [--mbases 150] [--runs 3] [--parent_tool PATH]
"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bam_corpus as BAM  # noqa: E402
from bam_profile import bgzf_fast  # noqa: E402
from ntedit_amd import _lib  # noqa: E402

TOOL = os.path.join(ROOT, "ntedit_amd", "ntedit-make-reads-bf")
Q = 20
PASS = re.compile(r"Pass (\S+) \([^)]*\): (\d+) bases, ([\d.]+) ms, [\d.]+ Gbases/s \(GPU calls ([\d.]+) ms")
PARSE_LINE = re.compile(r"--gpu_parse: (\d+) chunks parsed on the device .*?([\d.]+) ms in the parse kernels")
BAM_LINE = re.compile(r"BAM: (\d+) records .*?([\d.]+) ms in the walk kernels, ([\d.]+) ms in the decode kernels")
MASK_LINE = re.compile(r"--min_qual (\d+): (\d+) of (\d+) bases with a quality masked")


def read_set(rng, count, length=150):
    """-> (the BAM's inflated bytes, the FASTQ's bytes) of `count` reads of `length` bases, built with numpy"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.array([1, 2, 4, 8], dtype=np.uint8)
    name_len = 10
    names = np.frombuffer(b"".join(b"r%09d" % i for i in range(count)), dtype=np.uint8).reshape(count, name_len)
    idx = rng.integers(0, 4, size=(count, length), dtype=np.uint8)
    tail = rng.integers(0, 29, count)
    low = (np.arange(length)[None, :] >= length - tail[:, None]) | (rng.random((count, length)) < 0.01)
    phred = np.where(low, rng.integers(2, Q, (count, length)), rng.integers(Q, 42, (count, length))).astype(np.uint8)
    padded = np.concatenate([code[idx], np.zeros((count, length % 2), dtype=np.uint8)], axis=1)
    packed = (padded[:, 0::2] << 4 | padded[:, 1::2]).astype(np.uint8)
    block = 32 + name_len + 1 + packed.shape[1] + length
    fixed = struct.pack("<iiiBBHHHIiii", block, -1, -1, name_len + 1, 0, 4680, 0, 4, length, -1, -1, 0)
    rec = np.empty((count, 4 + block), dtype=np.uint8)
    rec[:, :36] = np.frombuffer(fixed, dtype=np.uint8)
    rec[:, 36:36 + name_len] = names
    rec[:, 36 + name_len] = 0
    rec[:, 37 + name_len:37 + name_len + packed.shape[1]] = packed
    rec[:, 37 + name_len + packed.shape[1]:] = phred
    q = np.empty((count, 1 + name_len + 1 + length + 3 + length + 1), dtype=np.uint8)
    q[:, 0] = ord("@")
    q[:, 1:1 + name_len] = names
    q[:, 1 + name_len] = 10
    q[:, 2 + name_len:2 + name_len + length] = acgt[idx]
    q[:, 2 + name_len + length:5 + name_len + length] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    q[:, 5 + name_len + length:-1] = phred + 33
    q[:, -1] = 10
    return BAM.header(b"@HD\tVN:1.6\tSO:unknown\n") + rec.tobytes(), q.tobytes(), float(low.mean())


def tool_run(tool, path, extra):
    r = subprocess.run([tool, "--reads", path, "-k", "25", "-c", "2", "--bf", "200000000", "--gpu_parse", "-o", path + ".bf"] + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(passes={n: dict(bases=int(b), wall_ms=float(w), gpu_calls_ms=float(g)) for n, b, w, g in PASS.findall(r.stderr)})
    rec["text_parse_ms"] = [float(m[1]) for m in PARSE_LINE.findall(r.stderr)]
    rec["bam_decode_ms"] = [float(m[2]) for m in BAM_LINE.findall(r.stderr)]
    rec["masked"] = [dict(q=int(q), masked_bases=int(m), qual_bases=int(b)) for q, m, b in MASK_LINE.findall(r.stderr)]
    with open(path + ".bf", "rb") as f:
        rec["filter_crc32"] = zlib.crc32(f.read())
    os.remove(path + ".bf")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mbases", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent_tool", help="ntedit-make-reads-bf of a build of the parent commit (beside its libntedit_hip.so)")
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    raw, fq, low = read_set(rng, a.mbases * 1000000 // 150)
    doc = dict(source="tests/tools/min_qual_profile.py", build_id=_lib.load().ntedit_hip_build_id().decode(), mbases=a.mbases,
               min_qual=Q, low_fraction=round(low, 4), runs=[])
    variants = ([("parent", a.parent_tool, [])] if a.parent_tool else []) + [("tree", TOOL, []), ("tree_min_qual", TOOL, ["--min_qual", str(Q)])]
    with tempfile.TemporaryDirectory() as d:
        files = {"fastq": os.path.join(d, "r.fq"), "bam": os.path.join(d, "r.bam")}
        with open(files["fastq"], "wb") as f:
            f.write(fq)
        with open(files["bam"], "wb") as f:
            f.write(bgzf_fast(raw))
        doc["file_bytes"] = {k: os.path.getsize(p) for k, p in files.items()}
        for i in range(a.runs):  # alternating, in one session
            doc["runs"].append({name: {kind: tool_run(tool, files[kind], extra) for kind in files} for name, tool, extra in variants})
            print("run", i, json.dumps(doc["runs"][-1]), flush=True)
    # the flagless filters are the parent's; the masked ones are one filter, whatever the format
    for names in (("parent", "tree"), ("tree_min_qual",)):
        crcs = {r[n][k]["filter_crc32"] for r in doc["runs"] for n in names if n in r for k in r[n]}
        assert len(crcs) == 1, (names, crcs)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
