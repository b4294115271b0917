"""Measurements of DESIGN.md 9.17 (--gpu_parse on BAM): two synthetic read sets of the same bases -- reads of 150 bases,
reads of 15 to 20 kb -- each as BAM and as bgzip FASTQ, through ntedit-make-reads-bf --gpu_parse in one session (the
tool's own Pass, BGZF and BAM lines), and the walk of one inflated chunk with the default segments against one chain
(the segment set to the chunk's size).  Writes the record as JSON.

    python tests/tools/bam_profile.py --out profiles/bam_parse.json [--mbases 150] [--runs 3]
"""
import argparse
import ctypes
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_corpus as BAM  # noqa: E402
from ntedit_amd import _lib  # noqa: E402

TOOL = os.path.join(ROOT, "ntedit_amd", "ntedit-make-reads-bf")
PASS = re.compile(r"Pass (\S+) \([^)]*\): (\d+) bases, ([\d.]+) ms, [\d.]+ Gbases/s \(GPU calls ([\d.]+) ms")
BAM_LINE = re.compile(r"BAM: (\d+) records .*?(\d+) chunks, (\d+) segments, (\d+) walked again by the stitch, ([\d.]+) ms in the walk "
                      r"kernels, ([\d.]+) ms in the decode kernels")
BGZF_LINE = re.compile(r"BGZF: (\d+) members .*?([\d.]+) ms in the inflate kernels")
PARSE_LINE = re.compile(r"--gpu_parse: (\d+) chunks parsed on the device .*?([\d.]+) ms in the parse kernels")


def bgzf_fast(data, threads=16):
    """data (bytes-like) as BGZF, level 1, the members compressed by a pool of threads (zlib releases the GIL)"""
    view = memoryview(data)
    blocks = [view[i:i + 65280] for i in range(0, len(view), 65280)]

    def one(b):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        s = c.compress(b) + c.flush()
        assert 18 + len(s) + 8 <= 65536
        return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(s) + 8 - 1) + s + struct.pack(
            "<II", zlib.crc32(b), len(b))
    with ThreadPoolExecutor(threads) as ex:
        return b"".join(ex.map(one, blocks)) + BAM.EOF_MEMBER


def read_set(rng, lengths):
    """-> (the BAM's inflated bytes, the twin FASTQ's bytes), built with numpy: records of equal length in one block each"""
    bam, fq = [BAM.header(b"@HD\tVN:1.6\tSO:unknown\n")], []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.array([1, 2, 4, 8], dtype=np.uint8)
    serial = 0
    for length, count in lengths:
        name_len = 10
        names = np.array([list(b"r%09d" % (serial + i)) for i in range(count)], dtype=np.uint8)
        serial += count
        idx = rng.integers(0, 4, size=(count, length), dtype=np.uint8)
        padded = np.concatenate([code[idx], np.zeros((count, length % 2), dtype=np.uint8)], axis=1)
        packed = (padded[:, 0::2] << 4 | padded[:, 1::2]).astype(np.uint8)
        block = 32 + name_len + 1 + packed.shape[1] + length
        fixed = struct.pack("<iiiBBHHHIiii", block, -1, -1, name_len + 1, 0, 4680, 0, 4, length, -1, -1, 0)
        rec = np.empty((count, 4 + block), dtype=np.uint8)
        rec[:, :36] = np.frombuffer(fixed, dtype=np.uint8)
        rec[:, 36:36 + name_len] = names
        rec[:, 36 + name_len] = 0
        rec[:, 37 + name_len:37 + name_len + packed.shape[1]] = packed
        rec[:, 37 + name_len + packed.shape[1]:] = 0xFF
        bam.append(rec.tobytes())
        q = np.empty((count, 1 + name_len + 1 + length + 3 + length + 1), dtype=np.uint8)
        q[:, 0] = ord("@")
        q[:, 1:1 + name_len] = names
        q[:, 1 + name_len] = 10
        q[:, 2 + name_len:2 + name_len + length] = acgt[idx]
        q[:, 2 + name_len + length:5 + name_len + length] = np.frombuffer(b"\n+\n", dtype=np.uint8)
        q[:, 5 + name_len + length:-1] = ord("I")
        q[:, -1] = 10
        fq.append(q.tobytes())
    return b"".join(bam), b"".join(fq)


def tool_run(path, extra):
    r = subprocess.run([TOOL, "--reads", path, "-k", "25", "-c", "2", "--bf", "200000000", "--gpu_parse", "-o", path + ".bf"] + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(passes={n: dict(bases=int(b), wall_ms=float(w), gpu_calls_ms=float(g)) for n, b, w, g in PASS.findall(r.stderr)})
    rec["bgzf_inflate_ms"] = [float(m[1]) for m in BGZF_LINE.findall(r.stderr)]
    rec["bam"] = [dict(records=int(m[0]), chunks=int(m[1]), segments=int(m[2]), rewalked=int(m[3]), walk_ms=float(m[4]),
                       decode_ms=float(m[5])) for m in BAM_LINE.findall(r.stderr)]
    rec["text_parse_ms"] = [float(m[1]) for m in PARSE_LINE.findall(r.stderr)]
    with open(path + ".bf", "rb") as f:
        rec["filter_crc32"] = zlib.crc32(f.read())
    os.remove(path + ".bf")
    return rec


def walk_runs(pol, raw, segment, runs):
    import torch
    lib = pol._lib
    dev = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
    text = torch.empty(len(raw) + 256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.ntedit_hip_reads_bam_set_segment(pol._h, segment) == 0
    out = []
    for _ in range(runs + 1):
        before, after, res = _lib.ReadsBamStats(), _lib.ReadsBamStats(), _lib.ReadsBamResult()
        lib.ntedit_hip_reads_bam_info(pol._h, before)
        rc = lib.ntedit_hip_reads_bam_device(pol._h, dev.data_ptr(), len(raw), 1, 1, 25, text.data_ptr(), len(raw), res)
        assert rc == 0 and res.clean == 1, lib.ntedit_hip_reads_last_error(pol._h)
        lib.ntedit_hip_reads_bam_info(pol._h, after)
        out.append(dict(walk_ms=round(after.ms_walk - before.ms_walk, 3), decode_ms=round(after.ms_decode - before.ms_decode, 3),
                        segments=after.segments - before.segments, rewalked=after.rewalked - before.rewalked,
                        records=res.records, cut=res.cut, text_len=res.text_len))
    return out[1:]  # (the first call allocates the scratch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mbases", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk_mib", type=int, default=128)
    a = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    rng = np.random.default_rng(2026)
    bases = a.mbases * 1000000
    long_lengths = [(int(x), 1) for x in rng.integers(15000, 20001, size=bases // 17500)]
    sets = {"reads_150": [(150, bases // 150)], "reads_15_to_20_kb": long_lengths}
    doc = dict(source="tests/tools/bam_profile.py", build_id=_lib.load().ntedit_hip_build_id().decode(), mbases=a.mbases, sets={})
    raws = {}
    with tempfile.TemporaryDirectory() as d:
        for name, lengths in sets.items():
            t0 = time.time()
            raw, fq = read_set(rng, lengths)
            files = {"bam": os.path.join(d, name + ".bam"), "bgzip_fastq": os.path.join(d, name + ".fq.gz")}
            for kind, data in (("bam", raw), ("bgzip_fastq", fq)):
                with open(files[kind], "wb") as f:
                    f.write(bgzf_fast(data))
            raws[name] = raw
            rec = dict(records=sum(c for _, c in lengths), inflated_bytes=dict(bam=len(raw), bgzip_fastq=len(fq)),
                       file_bytes={k: os.path.getsize(p) for k, p in files.items()}, runs=[])
            print(name, "written in %.1f s" % (time.time() - t0), flush=True)
            for i in range(a.runs):  # alternating, in one session
                rec["runs"].append({kind: tool_run(files[kind], []) for kind in ("bam", "bgzip_fastq")})
                print(name, "run", i, json.dumps(rec["runs"][-1]), flush=True)
            assert len({r[k]["filter_crc32"] for r in rec["runs"] for k in r}) == 1  # the same filter bytes every time
            doc["sets"][name] = rec
    import torch  # noqa: F401
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    try:
        doc["one_chunk"] = {}
        for name, raw in raws.items():
            chunk = raw[:a.chunk_mib << 20]
            doc["one_chunk"][name] = dict(bytes=len(chunk), stitched_default_segment=walk_runs(pol, chunk, 0, a.runs),
                                          one_chain=walk_runs(pol, chunk, 1 << 31, a.runs))
            print(name, json.dumps(doc["one_chunk"][name]), flush=True)
    finally:
        pol._lib.ntedit_hip_reads_bam_set_segment(pol._h, 0)
        pol._lib.ntedit_hip_sketch_free(pol._h)
        pol.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
