"""Measurements of DESIGN.md 9.20 (--min_read_len, --min_mean_qual, --min_rq): the synthetic 150-base read set of
tests/tools/min_qual_profile.py as plain FASTQ and as BAM, and one set of 20 kb reads, in one session of alternating runs.

  tool     ntedit-make-reads-bf --gpu_parse: a parent build's tool when one is given (--parent_tool), this tree's without the
           options, this tree's with --min_mean_qual 20 --min_rq 0.99.  Per run the tool's own lines: milliseconds in the
           parse kernels (FASTQ) and in the BAM decode kernels, the passes, the read filter's line, the filter's CRC-32.
  library  one chunk through ntedit_hip_reads_parse_device / _bam_device with and without the filter, alternating: what
           k_rp_qsum (with the filtering k_rp_records) adds to the parse kernels, and what k_bam_facts adds to the decode
           kernels at each group width (8, 16, 64 lanes per record), for the short and the long reads.
  yardstick  the bytes each new kernel must read (the quality lines for k_rp_qsum; the quality and aux bytes for k_bam_facts)
           over the rate k_rp_copy<false> and k_bam_decode<false> reach on the same chunk, and the ratio of the kernel's own
           time to that.  The per-kernel times come from a kernel trace of a run of its own (--library_only under the
           profiler, its statistics table given back with --kernel_stats).
  bench    bench.py --gpus 1 --steps 20 --warmup 5 of this tree and, with --parent_root, of the parent's, alternating.

    python tests/tools/read_filter_profile.py --out profiles/read_filter.json [--mbases 150] [--runs 3]
           [--parent_tool PATH] [--parent_root DIR]
"""
import argparse
import ctypes
import json
import os
import re
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
from min_qual_profile import BAM_LINE, PARSE_LINE, PASS, read_set  # noqa: E402
from ntedit_amd import _lib  # noqa: E402

TOOL = os.path.join(ROOT, "ntedit_amd", "ntedit-make-reads-bf")
Q, R = 20, 0.99
FILTER_LINE = re.compile(r"read filter: (\d+) of (\d+) records dropped \(length (\d+), rq (\d+), mean quality (\d+)\)")


def with_aux(rng, raw, count, length):
    """the BAM of read_set with aux fields behind every record's qualities, as a PacBio record has them: rq:f drawn around
    R, and a kinetics array ip:B:C of one byte per base -> (the bytes, the aux bytes per record)"""
    head = len(BAM.header(b"@HD\tVN:1.6\tSO:unknown\n"))
    rec = np.frombuffer(raw, dtype=np.uint8)[head:].reshape(count, -1)
    aux = np.empty((count, 7 + 8 + length), dtype=np.uint8)
    aux[:, 0:4] = np.frombuffer(b"ipBC", dtype=np.uint8)  # (in front of rq: the walk skips it by its count)
    aux[:, 4:8] = np.frombuffer(np.array([length], dtype="<u4").tobytes(), dtype=np.uint8)
    aux[:, 8:8 + length] = rng.integers(0, 256, (count, length), dtype=np.uint8)
    aux[:, 8 + length:11 + length] = np.frombuffer(b"rqf", dtype=np.uint8)
    aux[:, 11 + length:] = np.clip(R + rng.uniform(-0.02, 0.01, count), 0, 1).astype("<f4").view(np.uint8).reshape(count, 4)
    out = np.concatenate([rec, aux], axis=1)
    out[:, 0:4] = np.frombuffer(np.array([out.shape[1] - 4], dtype="<u4").tobytes(), dtype=np.uint8)
    return raw[:head] + out.tobytes(), aux.shape[1]


def yardstick(stats_csv, library):
    """kernel name -> (calls, mean ns) from the profiler's statistics table; then per new kernel the bytes it must read,
    the rate of the flagless copy / decode on the same chunk, the time those bytes take at that rate, and the ratio"""
    import csv
    mean = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("k_rp_qsum", "k_rp_copy<false>", "k_rp_copy<0>", "k_bam_decode<false>", "k_bam_decode<0>", "k_bam_facts<8>", "k_bam_facts<16>",
                        "k_bam_facts<64>"):
                if key in name.replace("(bool)0", "false").replace("(int)", ""):
                    mean[key.replace("<0>", "<false>")] = float(row.get("AverageNs") or row.get("Average") or 0) / 1e6
    rec = library["reads_150"]
    out = dict(kernel_ms=mean)
    if "k_rp_copy<false>" in mean and "k_rp_qsum" in mean:
        rate = rec["fastq_bytes"] / mean["k_rp_copy<false>"]  # bytes per ms: the copy reads the whole chunk
        need = rec["quality_line_bytes"] / rate
        out["k_rp_qsum"] = dict(bytes=rec["quality_line_bytes"], copy_gb_s=round(rate / 1e6, 1), yardstick_ms=round(need, 3),
                                ratio=round(mean["k_rp_qsum"] / need, 2))
    if "k_bam_decode<false>" in mean:
        rate = rec["bam_seq_bytes"] / mean["k_bam_decode<false>"]  # the decode reads the packed bases
        need = rec["bam_qual_aux_bytes"] / rate
        for w in (8, 16, 64):
            k = "k_bam_facts<%d>" % w
            if k in mean:
                out[k] = dict(bytes=rec["bam_qual_aux_bytes"], decode_gb_s=round(rate / 1e6, 1), yardstick_ms=round(need, 3),
                              ratio=round(mean[k] / need, 2))
    return out


def tool_run(tool, path, extra):
    r = subprocess.run([tool, "--reads", path, "-k", "25", "-c", "2", "--bf", "200000000", "--gpu_parse", "-o", path + ".bf"] + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(passes={n: dict(bases=int(b), wall_ms=float(w), gpu_calls_ms=float(g)) for n, b, w, g in PASS.findall(r.stderr)})
    rec["text_parse_ms"] = [float(m[1]) for m in PARSE_LINE.findall(r.stderr)]
    rec["bam_decode_ms"] = [float(m[2]) for m in BAM_LINE.findall(r.stderr)]
    rec["read_filter"] = [dict(dropped=int(d), records=int(n), length=int(a), rq=int(b), mean_quality=int(c))
                          for d, n, a, b, c in FILTER_LINE.findall(r.stderr)]
    with open(path + ".bf", "rb") as f:
        rec["filter_crc32"] = zlib.crc32(f.read())
    os.remove(path + ".bf")
    return rec


def library_runs(sets, runs):
    """{set: {fastq: {...}, bam: {...}}}: kernel milliseconds of one chunk, without and with the filter, alternating"""
    import torch
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    lib, h = pol._lib, pol._h
    out = {}
    for name, (raw, fq, length, count, aux_bytes) in sets.items():
        text = torch.empty(max(len(raw), len(fq)) + 64, dtype=torch.uint8, device="cuda")
        cap = (max(len(raw), len(fq)) + 15) // 16 * 16

        def parse_ms(q):
            st0, st1, res = _lib.ReadsParseStats(), _lib.ReadsParseStats(), _lib.ReadsParseResult()
            assert lib.ntedit_hip_reads_set_read_filter(h, 0, q, 0.0) == 0 and lib.ntedit_hip_reads_parse_info(h, st0) == 0
            assert lib.ntedit_hip_reads_parse_device(h, fq, len(fq), 0, 25, text.data_ptr(), cap, res) == 0 and res.clean == 1
            assert lib.ntedit_hip_reads_parse_info(h, st1) == 0
            return st1.ms_kernels - st0.ms_kernels, res.reads

        def bam_ms(q, r, width):
            st0, st1, res = _lib.ReadsBamStats(), _lib.ReadsBamStats(), _lib.ReadsBamResult()
            assert lib.ntedit_hip_reads_set_read_filter(h, 0, q, r) == 0 and lib.ntedit_hip_reads_bam_set_group_width(h, width) == 0
            assert lib.ntedit_hip_reads_bam_info(h, st0) == 0
            assert lib.ntedit_hip_reads_bam_device(h, raw, len(raw), 0, 1, 25, text.data_ptr(), cap, res) == 0 and res.clean == 1
            assert lib.ntedit_hip_reads_bam_info(h, st1) == 0
            return st1.ms_decode - st0.ms_decode, res.kept

        parse_ms(0), bam_ms(0, 0.0, 0)  # (warm: the scratch is allocated)
        rec = dict(read_length=length, reads=count, fastq_bytes=len(fq), bam_bytes=len(raw), quality_line_bytes=count * length,
                   bam_seq_bytes=count * ((length + 1) // 2), bam_qual_aux_bytes=count * (length + aux_bytes), runs=[])
        for _ in range(runs):
            # (a minimum of 1 keeps every read: the copy and the decode behind the new kernels do the work they do without)
            one = dict(parse_off=parse_ms(0), parse_mean_qual=parse_ms(1), decode_off=bam_ms(0, 0.0, 0))
            for width in (8, 16, 64):
                one["decode_facts_%d" % width] = bam_ms(1, 1e-6, width)  # (every rq is above it: the walk runs, no read is dropped)
            rec["runs"].append({k: dict(ms=round(v[0], 3), kept=int(v[1])) for k, v in one.items()})
        med = lambda key: float(np.median([r[key]["ms"] for r in rec["runs"]]))
        rec["added_ms"] = dict(k_rp_qsum=round(med("parse_mean_qual") - med("parse_off"), 3),
                               **{"k_bam_facts_%d" % w: round(med("decode_facts_%d" % w) - med("decode_off"), 3) for w in (8, 16, 64)})
        out[name] = rec
    lib.ntedit_hip_reads_set_read_filter(h, 0, 0, 0.0)
    lib.ntedit_hip_reads_bam_set_group_width(h, 0)
    lib.ntedit_hip_sketch_free(h)
    pol.close()
    return out


def bench_run(root):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root, capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mbases", type=int, default=150)
    ap.add_argument("--long_mbases", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent_tool", help="ntedit-make-reads-bf of a build of the parent commit (beside its libntedit_hip.so)")
    ap.add_argument("--parent_root", help="a built tree of the parent commit, for bench.py")
    ap.add_argument("--no_bench", action="store_true")
    ap.add_argument("--bench_only", action="store_true", help="add the bench.py runs to an existing --out")
    ap.add_argument("--library_only", action="store_true", help="the library runs of the 150-base set alone, once (for a kernel trace)")
    ap.add_argument("--kernel_stats", help="the profiler's kernel statistics (CSV) of a --library_only run: adds the yardstick to --out")
    a = ap.parse_args()
    if a.bench_only:  # (the same session, behind the runs above: the record grows by the benchmark's lines)
        with open(a.out) as f:
            doc = json.load(f)
        for i in range(a.runs):
            doc["bench"].append({name: bench_run(root) for name, root in (("parent", a.parent_root), ("tree", ROOT)) if root})
            print("bench", i, json.dumps(doc["bench"][-1]), flush=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
        return
    if a.kernel_stats:  # (no device: the recorded runs and the statistics table)
        with open(a.out) as f:
            doc = json.load(f)
        doc["yardstick"] = yardstick(a.kernel_stats, doc["library"])
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        return
    import torch  # (torch's HIP runtime first, as the drivers load it: the library runs below go through it)
    torch.cuda.init()
    rng = np.random.default_rng(2026)
    n_short, n_long = a.mbases * 1000000 // 150, a.long_mbases * 1000000 // 20000
    raw, fq, low = read_set(rng, n_short)
    aux_raw, aux_short = with_aux(rng, raw, n_short, 150)
    if a.library_only:
        print(json.dumps(library_runs({"reads_150": (aux_raw, fq, 150, n_short, aux_short)}, 1)))
        return
    long_raw, long_fq, _ = read_set(rng, n_long, 20000)
    long_raw, aux_long = with_aux(rng, long_raw, n_long, 20000)
    doc = dict(source="tests/tools/read_filter_profile.py", build_id=_lib.load().ntedit_hip_build_id().decode(), mbases=a.mbases,
               min_mean_qual=Q, min_rq=R, tool_runs=[], bench=[])
    extra = ["--min_mean_qual", str(Q), "--min_rq", str(R)]
    variants = ([("parent", a.parent_tool, [])] if a.parent_tool else []) + [("tree", TOOL, []), ("tree_read_filter", TOOL, extra)]
    with tempfile.TemporaryDirectory() as d:
        files = {"fastq": os.path.join(d, "r.fq"), "bam": os.path.join(d, "r.bam")}
        with open(files["fastq"], "wb") as f:
            f.write(fq)
        with open(files["bam"], "wb") as f:
            f.write(bgzf_fast(raw))
        doc["file_bytes"] = {k: os.path.getsize(p) for k, p in files.items()}
        for i in range(a.runs):  # alternating, in one session
            doc["tool_runs"].append({name: {kind: tool_run(tool, files[kind], x) for kind in files} for name, tool, x in variants})
            print("tool run", i, json.dumps(doc["tool_runs"][-1]), flush=True)
    # the flagless filters are the parent's; the filtered ones are one filter, whatever the format
    for names in (("parent", "tree"), ("tree_read_filter",)):
        crcs = {r[n][k]["filter_crc32"] for r in doc["tool_runs"] for n in names if n in r for k in r[n]}
        assert len(crcs) == 1, (names, crcs)
    # (the library runs take the BAM with rq and kinetics aux fields: the aux walk has something to walk)
    doc["library"] = library_runs({"reads_150": (aux_raw, fq, 150, n_short, aux_short),
                                   "reads_20kb": (long_raw, long_fq, 20000, n_long, aux_long)}, a.runs)
    print("library", json.dumps(doc["library"]), flush=True)
    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)

    save()
    for i in range(0 if a.no_bench else a.runs):
        doc["bench"].append({name: bench_run(root) for name, root in (("parent", a.parent_root), ("tree", ROOT)) if root})
        print("bench", i, json.dumps(doc["bench"][-1]), flush=True)
        save()


if __name__ == "__main__":
    main()
