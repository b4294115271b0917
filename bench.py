#!/usr/bin/env python
"""bench.py -- polished Mbases/s of the ntEdit hot path on MI355X.

One "step" = one pass of the hot path (screen -> event extraction -> event
machine -> edit records back in host memory) over one batch of synthetic draft
that is already resident in HBM.  Workload at N=1 (BASELINE.json: the config
the metric is quoted on): synthetic 3 Gbp draft (0.1% substitutions, 0.01%
indels), k=25, 4 GiB Bloom filter with h=3 built from the truth genome.
N>1: one process per GPU, STRONG scaling (BASELINE.json configs[3]: ONE 3 Gbp
draft sharded over the GPUs): every rank holds the same draft, the contigs are
partitioned by bases exactly as the multi-GPU driver does it (ntedit_amd.dist:
contigs larger than an eighth of a GPU's share are cut into segments at
event-free boundaries, greedy LPT over the pieces), each rank polishes its
pieces against an identical filter that rank 0 builds and broadcasts once over
RCCL (the path's single collective, untimed set-up).  No communication inside
the timed region; value = the whole draft's bases / the slowest rank's time.

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype,
ms_per_step, the workload's config) with an extra object "roofline"
(screening kernel, HBM-bound; algorithmic bytes = 4.125 B per screened base at
h=3), computed from the timed steps' own timers.

A plain run does only what that line needs: set-up, warm-up, the timed steps,
--dump-outputs.  Whatever takes runs of its own comes with --full:
  "weak"                  N>1: every rank polishes the whole 3 Gbp draft
                          (weak scaling), measured right behind the strong figure
  roofline.random_gather_probes_per_s  a random-gather micro-benchmark
  "kernel_region_host*", "end_to_end*"  N=1: the batch from host memory, and
                          the `ntedit` binary end to end (measured_regions)
  "cpu_baseline"          N=1: the C oracle timed on a bounded sample of the
                          same draft + filter on the host
The --no-* options below leave out single parts of --full.

--dump-outputs DIR writes what the last timed step computed (its edit records; with --screen-only the bitmap) as
DIR/<name>.npy, float32 / float64, at most 64 MB: the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=float, default=3.0e9, help="draft bases per GPU")
    ap.add_argument("--filter-bytes", type=int, default=1 << 32)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: the weak-scaling leg (N>1), the random-gather "
                         "roofline, the host-buffer and end-to-end regions and the CPU baseline (N=1)")
    ap.add_argument("--cpu-sample-bases", type=float, default=30e6)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the multi-threaded CPU baseline (default min(64, cores))")
    ap.add_argument("--cpu-mt-seconds", type=float, default=12.0, help="target duration of the multi-threaded CPU baseline")
    ap.add_argument("--no-gather", action="store_true", help="--full without the random-gather micro-benchmark")
    ap.add_argument("--screen-only", action="store_true", help="time only the screening kernel (profiling aid)")
    ap.add_argument("--start-grid", type=int, default=0, help="event start grid override (tuning)")
    ap.add_argument("--screen-mode", type=int, default=0, help="0 auto, 1 direct gather, 2 L2-partitioned")
    ap.add_argument("--contig-len", type=int, default=0, help="contigs of exactly this many bases (configs[2]: 100000)")
    ap.add_argument("--no-weak", action="store_true", help="--full without the weak-scaling leg at N>1")
    ap.add_argument("--e2e-gzip", action="store_true", help="also run the end-to-end region on the draft as ONE gzip stream (level 6), "
                    "inflated by host/gunzip.cpp and, for comparison, by zlib")
    ap.add_argument("--e2e-bgzf", action="store_true", help="also run the end-to-end region on a BGZF-compressed draft")
    ap.add_argument("--no-e2e", action="store_true", help="--full without the end-to-end region (the `ntedit` binary)")
    ap.add_argument("--no-regions", action="store_true", help="--full without the host-buffer and end-to-end regions (N=1)")
    ap.add_argument("--snv", action="store_true",
                    help="N=1 side line: -s 1 (every position re-assessed, ntedit.cpp:1806,1865; -i/-d 0)")
    ap.add_argument("--counting", action="store_true",
                    help="N=1 side line: a counting filter of --filter-bytes 8-bit counters (synthetic contents), -p 2")
    ap.add_argument("--structure", choices=("iid", "genome"), default="iid",
                    help="truth genome: i.i.d. bases (SURVEY 8d, the headline) or with repeat arrays, repeat families, segmental "
                         "duplications and stretches the filter does not hold (synth.GenomeStructure; a side line)")
    ap.add_argument("--structure-fractions", default="", help="JSON: shares of single classes of --structure genome, e.g. "
                    "'{\"novel\": 0}' (diagnosis)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="ntedit_hip_set_tuning knob (repeatable; none of them changes a result)")
    ap.add_argument("--no-reserve", action="store_true",
                    help="skip ntedit_hip_reserve in the set-up: the first step then pays the context's buffer allocations")
    ap.add_argument("--shared-filter", action="store_true",
                    help="use the multi-GPU filter path (torch-owned filter tensor + broadcast) even with 1 rank")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32/float64, "
                         "at most 64 MB in all; see dump_edits / dump_screen)")
    args = ap.parse_args()
    if (args.e2e_gzip or args.e2e_bgzf) and not args.full:
        ap.error("--e2e-gzip / --e2e-bgzf extend the end-to-end region, which only --full measures")
    return args


def usable_cpus():
    """CPUs this process can really use: affinity mask and cgroup CPU quota (a GPU box's container may
    show 256 CPUs and be allowed 16 of them)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(job, pol, args):
    """The oracle ("port") on the same draft and the same filter (downloaded from HBM): one thread on a
    ~cpu-sample-bases sample, then the reference's contig-level parallelism on up to 64 threads.  Reported,
    not targeted."""
    import numpy as np
    import torch
    import helpers as H

    H.build_oracle()
    # pick whole contigs, shortest first in input order, until the sample is filled
    want = int(args.cpu_sample_bases)
    idx, total = [], 0
    for i in np.argsort(job.lens, kind="stable"):
        if total >= want:
            break
        if total + int(job.lens[i]) > 2 * want and total > 0:
            continue
        idx.append(int(i))
        total += int(job.lens[i])
    idx.sort()
    parts, offs, lens, pos = [], [], [], 0
    for i in idx:
        o, l = int(job.offsets[i]), int(job.lens[i])
        parts.append(job.batch[o:o + l + 1].cpu().numpy().tobytes())
        offs.append(pos)
        lens.append(l)
        pos += l + 1
    blob = b"".join(parts)
    offs = np.array(offs, dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    bits = pol.filter_download(0)
    k, h, nbytes, _ = pol.filter_info(0)
    t0 = time.perf_counter()
    done = H.oracle_polish_flat(blob, offs, lens, bits, h, k)
    dt = time.perf_counter() - t0
    single = {"value": done / dt / 1e6, "cores": 1,
              "sample": "%d contigs / %.1f Mbases of the same draft, same %d-byte filter, 1 thread, %.1f s" %
                        (len(lens), done / 1e6, nbytes, dt)}
    # The reference's own parallelism: contigs handed out to host threads (OpenMP loop, ntedit.cpp:2213-2253).
    # Up to 64 threads (north_star's "64 host cores") over as much of the draft as ~cpu-mt-seconds allow.
    cores = max(1, min(64, usable_cpus(), int(args.cpu_threads) if args.cpu_threads else 64))
    host = job.batch.cpu().numpy()

    def prefix(budget, first=0):
        # contigs in input order (the order the reference hands them to its threads), whole contigs only
        pick, total = [], 0
        for i in range(first, len(job.lens)):
            if total >= budget and pick:
                break
            pick.append(i)
            total += int(job.lens[i])
        return pick

    pick = prefix(single["value"] * 1e6 * cores * float(args.cpu_mt_seconds))
    t0 = time.perf_counter()
    done_mt = H.oracle_polish_flat_mt(host, job.offsets[pick], job.lens[pick], bits, h, k, cores)
    dt_mt = time.perf_counter() - t0
    return {"value": done_mt / dt_mt / 1e6, "unit": "Mbases/s", "cores": cores, "kind": "port",
            "sample": "%d of %d contigs / %.1f Mbases of the same draft (longest %.1f Mbp), same %d-byte filter, contigs "
                      "handed out to %d threads, %.1f s" % (len(pick), len(job.lens), done_mt / 1e6,
                                                              float(job.lens[pick].max()) / 1e6, nbytes, cores, dt_mt),
            "single_thread": single}


def measured_regions(job, pol, args):
    """The other two regions of SURVEY.md 8(d), measured on the same draft + filter and carried in the same JSON line:
    kernel_region_host  the batch starts in (page-locked) HOST memory and the edit records end in host memory:
                        ntedit_hip_polish_batch(on_device=0), H2D pieces overlapped with the screening;
    end_to_end          the `ntedit` binary on a plain FASTA + .bf file on local disk, its
                        "reading/processing input sequence" -> "process complete" region (ntedit.cpp:2589-2598):
                        FASTA parse, H2D, GPU, D2H, serial-order apply + rendering, 3 GB of output written.
    Neither is `value` (that is the HBM-resident rate)."""
    import shutil
    import subprocess
    import tempfile
    import torch
    out = {}
    host = torch.empty(job.n_bytes, dtype=torch.uint8).pin_memory()
    host.copy_(job.batch)
    torch.cuda.synchronize()
    hnp = host.numpy()
    try:
        ms = []
        for i in range(3):
            t0 = time.perf_counter()
            res = pol.polish_batch(hnp, job.offsets, job.lens)
            dt = time.perf_counter() - t0
            st = res.stats()
            res.free()
            if i:
                ms.append((dt * 1e3, st.ms_total, st.ms_screen, st.screen_launches))
        best = min(ms)
        out["kernel_region_host"] = {
            "value": round(job.n_bases / best[0] / 1e3, 2), "unit": "Mbases/s", "ms_per_call": round(best[0], 3),
            "gpu_timeline_ms": round(best[1], 3), "screen_ms_incl_copy_waits": round(best[2], 3),
            "screen_launches": int(best[3]),
            "note": "page-locked host batch -> edit records in host memory, one ntedit_hip_polish_batch call "
                    "(wall clock, best of 2 after a warm-up); H2D in pieces overlapped with screening"}
    except Exception as e:  # pragma: no cover
        out["kernel_region_host"] = {"error": str(e)}
    # the same region with the batch in the PACKED form (include/ntedit_hip.h: 4-bit codes + a case bit per base, 5/8 of the
    # bytes): what crosses PCIe when the FASTA parser -- which touches every byte anyway -- emits that form next to the
    # bytes the renderer keeps.  Packing happens before the clock starts (it is the producer's work, timed separately).
    try:
        ppin = torch.empty(pol.packed_size(job.n_bytes), dtype=torch.uint8).pin_memory()
        t0 = time.perf_counter()
        packed = pol.pack_bases(hnp, out=ppin.numpy())
        t_pack = time.perf_counter() - t0
        if packed is not None:
            ms = []
            for i in range(3):
                t0 = time.perf_counter()
                res = pol.polish_batch(hnp, job.offsets, job.lens, packed=packed)
                dt = time.perf_counter() - t0
                st = res.stats()
                res.free()
                if i:
                    ms.append((dt * 1e3, st.ms_total, st.ms_screen, st.screen_launches))
            best = min(ms)
            out["kernel_region_host_packed"] = {
                "value": round(job.n_bases / best[0] / 1e3, 2), "unit": "Mbases/s", "ms_per_call": round(best[0], 3),
                "gpu_timeline_ms": round(best[1], 3), "screen_ms_incl_copy_waits": round(best[2], 3),
                "packed_bytes": int(pol.packed_size(job.n_bytes)), "pack_s_host_threads": round(t_pack, 3),
                "note": "the batch handed over in the packed form (page-locked), unpacked on the device (k_unpack); "
                        "packing it (ntedit_hip_pack_bases, multi-threaded) is the producer's work and not in the region"}
        del ppin
    except Exception as e:  # pragma: no cover
        out["kernel_region_host_packed"] = {"error": str(e)}
    if args.no_e2e:
        del host
        return out
    cli = os.path.join(ROOT, "ntedit_amd", "ntedit")
    work = tempfile.mkdtemp(prefix="ntedit_bench_e2e_")
    try:
        bf = os.path.join(work, "truth.bf")
        pol.filter_save_file(bf)
        draft = os.path.join(work, "draft.fa")
        with open(draft, "wb") as f:
            for i, (o, l) in enumerate(zip(job.offsets.tolist(), job.lens.tolist())):
                f.write(b">contig%d len=%d\n" % (i, l))
                f.write(hnp[o:o + l + 1].tobytes())  # sequence + '\n'
        runs = []
        os.sync()  # (dirty pages of whatever ran before -- this draft, test outputs -- are written back first)
        # The CLI runs as a child of this process, which keeps its own context on the same GPU: about every other run
        # its host-to-device copies crawl (polish calls 0.9 s instead of 0.37 s; by hand, without this parent, never --
        # tools/gpu_numa.sh).  Hence the best of five.
        for _ in range(5):
            for suf in ("_edited.fa", "_changes.tsv", "_variants.vcf"):  # (every run starts without output files)
                if os.path.exists(os.path.join(work, "out" + suf)):
                    os.unlink(os.path.join(work, "out" + suf))
            t0 = time.perf_counter()
            r = subprocess.run([cli, "-f", draft, "-r", bf, "-b", os.path.join(work, "out"), "--report"],
                               capture_output=True, text=True, timeout=300)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-500:])
            if os.environ.get("NTEDIT_HIP_DEBUG"):
                sys.stderr.write("".join(l + "\n" for l in r.stderr.splitlines() if "[ntedit_hip]" in l))
            rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            if os.environ.get("NTEDIT_HIP_DEBUG"):
                sys.stderr.write("[cli report] %s\n" % json.dumps(rep))
            runs.append((rep["seconds"], wall, rep))
        sec, wall, rep = min(runs, key=lambda x: x[0])
        all_s = sorted(x[0] for x in runs)
        out["end_to_end"] = {
            "value": round(rep["bases"] / sec / 1e6, 2), "unit": "Mbases/s", "region_s": round(sec, 4),
            "region_s_all_runs": [round(x[0], 4) for x in runs],
            "stage_s_all_runs": [{"fasta_parse": x[2]["read_s"], "polish_batch_calls": x[2]["polish_call_s"],
                                  "apply_render_write": x[2]["write_s"], "gpu_ms": x[2]["gpu_ms"]} for x in runs],
            "median_value": round(rep["bases"] / all_s[len(all_s) // 2] / 1e6, 2),
            "process_wall_s": round(wall, 3),
            "stage_s": {"open_outputs": rep.get("open_outputs_s"), "fasta_index": rep.get("index_s"),
                        "fasta_parse": rep["read_s"], "polish_batch_calls": rep["polish_call_s"],
                        "apply_render_write": rep["write_s"]},
            "gpu_ms": rep["gpu_ms"], "events_applied": rep["events_applied"],
            "output_bytes": os.path.getsize(os.path.join(work, "out_edited.fa")),
            "note": "`ntedit -f draft.fa -r truth.bf` on local disk, region = the reference's 'reading/processing "
                    "input sequence' -> 'process complete' stamps; the three stages overlap (pipeline); process wall "
                    "adds reading the 4 GiB filter file into HBM; value = best of 5 runs, median_value = their median "
                    "(as a child of this process, which keeps its own context on the GPU, some runs have slow "
                    "host-to-device copies; by hand, without the parent, none does)"}
        if args.e2e_gzip:
            gz = os.path.join(work, "draft1.fa.gz")
            t0 = time.perf_counter()
            gzip_one_stream(draft, gz, min(64, usable_cpus()))
            t_comp = time.perf_counter() - t0
            res = {}
            for tag, extra in (("gunzip", []), ("zlib", ["--tune", "host_zlib=1"])):
                best = None
                for _ in range(2):
                    if os.path.exists(os.path.join(work, "outg_edited.fa")):
                        os.unlink(os.path.join(work, "outg_edited.fa"))
                    r = subprocess.run([cli, "-f", gz, "-r", bf, "-b", os.path.join(work, "outg"), "--report"] + extra,
                                       capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        raise RuntimeError(r.stderr[-500:])
                    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                    if best is None or rep["seconds"] < best["seconds"]:
                        best = rep
                res[tag] = {"value": round(best["bases"] / best["seconds"] / 1e6, 2), "unit": "Mbases/s",
                            "region_s": round(best["seconds"], 4), "fasta_parse_s": best["read_s"],
                            "polish_batch_calls_s": best["polish_call_s"], "apply_render_write_s": best["write_s"]}
            out["end_to_end_gzip"] = {
                **res["gunzip"], "through_zlib": res["zlib"], "compressed_bytes": os.path.getsize(gz),
                "note": "the same draft as ONE gzip member (deflate level 6, %.1f s to write here): inflate thread -> "
                        "parser -> batches; best of 2 runs each; through_zlib = the same with zlib's gzread doing "
                        "the inflating (`--tune host_zlib=1`)" % t_comp}
        if args.e2e_bgzf:
            gz = os.path.join(work, "draft.fa.gz")
            t0 = time.perf_counter()
            bgzf_compress(draft, gz, min(64, usable_cpus()))
            t_comp = time.perf_counter() - t0
            if os.path.exists(os.path.join(work, "out_edited.fa")):
                os.unlink(os.path.join(work, "out_edited.fa"))
            r = subprocess.run([cli, "-f", gz, "-r", bf, "-b", os.path.join(work, "outz"), "--report"],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-500:])
            rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            out["end_to_end_bgzf"] = {
                "value": round(rep["bases"] / rep["seconds"] / 1e6, 2), "unit": "Mbases/s", "region_s": round(rep["seconds"], 4),
                "compressed_bytes": os.path.getsize(gz), "inflate_and_index_s": rep.get("index_s"), "fasta_parse_s": rep["read_s"],
                "note": "the same draft bgzip-compressed (level 1, %.1f s to write here): members inflated on all host "
                        "threads, then read like the plain file" % t_comp}
    except Exception as e:  # pragma: no cover
        out["end_to_end"] = {"error": str(e)}
    finally:
        if os.environ.get("NTEDIT_BENCH_KEEP_E2E"):  # experiments: keep draft.fa / truth.bf for runs by hand
            sys.stderr.write("[bench] end-to-end inputs kept in %s\n" % work)
        else:
            shutil.rmtree(work, ignore_errors=True)
    del host
    return out


def _deflate_piece(job):
    import zlib
    chunk, last = job
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(chunk) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH), zlib.crc32(chunk), len(chunk)


def _crc32_combine(crc1, crc2, len2):
    """CRC-32 of A+B from CRC-32(A), CRC-32(B) and len(B) (the operator that appends one zero bit to a message,
    as a 32x32 matrix over GF(2), squared up to len2 bytes)"""
    def times(mat, vec):
        s, i = 0, 0
        while vec:
            if vec & 1:
                s ^= mat[i]
            vec >>= 1
            i += 1
        return s

    def square(mat):
        return [times(mat, mat[n]) for n in range(32)]
    if len2 == 0:
        return crc1
    odd = [0xedb88320] + [1 << (n - 1) for n in range(1, 32)]
    even = square(odd)
    odd = square(even)
    while True:
        even = square(odd)
        if len2 & 1:
            crc1 = times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = square(even)
        if len2 & 1:
            crc1 = times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def gzip_one_stream(src, dst, procs):
    """src as ONE gzip member, written the way pigz does: pieces deflated side by side (each closed by an empty
    stored block), one header, one trailer"""
    import multiprocessing as mp
    import struct
    piece = 32 << 20
    size = os.path.getsize(src)

    def jobs():
        with open(src, "rb") as f:
            pos = 0
            while True:
                chunk = f.read(piece)
                pos += len(chunk)
                yield chunk, pos >= size
                if pos >= size:
                    break
    crc, total = 0, 0
    with mp.Pool(procs) as pool, open(dst, "wb") as o:
        o.write(b"\x1f\x8b\x08\0\0\0\0\0\0\x03")
        for data, c, n in pool.imap(_deflate_piece, jobs()):
            o.write(data)
            crc = _crc32_combine(crc, c, n)
            total += n
        o.write(struct.pack("<II", crc, total & 0xffffffff))


def _bgzf_members(chunk):
    import struct
    import zlib
    out = []
    for i in range(0, len(chunk), 65280):
        piece = chunk[i:i + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    return b"".join(out)


def bgzf_compress(src, dst, procs):
    """src -> dst in the BGZF container (what `bgzip` writes: independent gzip members of <= 64 KiB), on `procs` processes"""
    import multiprocessing as mp
    step = 65280 * 256

    def chunks():
        with open(src, "rb") as f:
            while True:
                b = f.read(step)
                if not b:
                    return
                yield b

    with mp.get_context("fork").Pool(procs) as pool, open(dst, "wb") as o:
        for blob in pool.imap(_bgzf_members, chunks(), chunksize=1):
            o.write(blob)
        o.write(_bgzf_members(b"") or b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0")


class _DeviceSeq:
    """a contig of the HBM-resident batch, sliceable to host bytes (what dist.plan_pieces needs to place cuts)"""

    def __init__(self, batch, off, n):
        self.batch, self.off, self.n = batch, off, n

    def __len__(self):
        return self.n

    def __getitem__(self, sl):
        lo, hi, _ = sl.indices(self.n)
        return self.batch[self.off + lo:self.off + hi].cpu().numpy().tobytes()


def shard_batch(job, pol, rank, world, k, torch):
    """This rank's share of the one draft, laid out as its own HBM-resident batch: the pieces dist.plan_pieces
    assigns to it (whole contigs, or segments of contigs larger than an eighth of a share with their look-ahead
    halos).  Returns (batch tensor, offsets, lens, halos, pieces of every rank)."""
    import numpy as np
    from ntedit_amd import dist as ndist
    p = pol.params
    halo = ndist.halo_bases(k, p.max_insertions, p.max_deletions)
    records = [(b"contig%d" % i, _DeviceSeq(job.batch, int(job.offsets[i]), int(job.lens[i])))
               for i in range(len(job.lens))]
    pieces = ndist.plan_pieces(records, world, p.min_contig_len, k, halo, pol.screen)
    mine = [q for q in pieces if q.owner == rank]
    nl = torch.tensor([10], dtype=torch.uint8, device=job.batch.device)
    parts, offs, lens, halos, pos = [], [], [], [], 0
    for q in mine:
        h = 0 if q.seg == q.n_seg - 1 else halo
        o = int(job.offsets[q.contig])
        # (every entry starts 16-byte aligned like a fresh batch would; pad with separators)
        pad = (-pos) % 16
        if pad:
            parts.append(nl.repeat(pad))
            pos += pad
        parts.append(job.batch[o + q.start:o + q.end + h])
        parts.append(nl)
        offs.append(pos)
        lens.append(q.end - q.start + h)
        halos.append(h)
        pos += q.end - q.start + h + 1
    batch = torch.cat(parts) if parts else torch.zeros(16, dtype=torch.uint8, device=job.batch.device)
    return (batch, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), np.array(halos, dtype=np.int64),
            pieces)


DUMP_LIMIT = 64_000_000  # bytes of .npy files --dump-outputs writes at most (all ranks together)
DUMP_SEED = 20251033      # the fixed sample of a larger output
STATS_FIELDS = ("bases", "absent_kmers", "events")  # (the applied-edit counters are filled in by rendering only)
NPY_HEADER = 128          # bytes np.save puts in front of a small array's data
RECORD_BYTES = 3 * 8 + 6 * 4 + 2 * 3 * 4  # one record's share of the edit_* arrays, its bases aside


def _save(out_dir, prefix, arrays):
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, prefix + name + ".npy"), a)


def dump_edits(out_dir, recs, pool, stats, n_contigs, prefix="", limit=DUMP_LIMIT):
    """--dump-outputs of the polish path: what ntedit_hip_polish_batch hands its caller, the batch's edit records
    (_lib.EDIT_DTYPE, the _changes.tsv rows) and the bases of its insertions / deletions.
      stats             float64 [3]: the result counters of STATS_FIELDS
      edits_per_contig  float64 [n_contigs]: records per entry, over ALL records
      edits_per_kind    float64 [5]: records per kind (_lib.EDIT_SUB .. EDIT_SNV_KEPT; 0 unused), over ALL records
      edit_index        float64 [S]: which records follow, in order (all of them, or a fixed seeded sample when they
                        would not fit in `limit`), then one array per record field of those S records:
      edit_contig, edit_draft_pos (float64); edit_len, edit_support, edit_kind, edit_draft_base, edit_new_base,
      edit_n_alt (float32); edit_alt_base, edit_alt_support (float32 [S, 3]);
      edit_bases        float32: the inserted / deleted bases (byte values) of those records that are insertions or
                        deletions, edit_len of them per record, one record after the other"""
    import numpy as np
    from ntedit_amd import _lib
    n = len(recs)
    head = {"stats": np.array([float(getattr(stats, f)) for f in STATS_FIELDS], dtype=np.float64),
            "edits_per_contig": np.bincount(recs["contig"].astype(np.int64), minlength=n_contigs).astype(np.float64),
            "edits_per_kind": np.bincount(recs["kind"], minlength=5).astype(np.float64)}
    carry = (recs["kind"] == _lib.EDIT_INS) | (recs["kind"] == _lib.EDIT_DEL)
    cost = RECORD_BYTES + 4 * np.where(carry, recs["len"], 0).astype(np.int64)
    room = limit - sum(a.nbytes for a in head.values()) - 16 * NPY_HEADER
    if int(cost.sum()) <= room:
        idx = np.arange(n)
    else:  # the longest prefix of a seeded permutation that fits
        order = np.random.default_rng(DUMP_SEED).permutation(n)
        idx = np.sort(order[:int(np.searchsorted(np.cumsum(cost[order]), room, side="right"))])
    s = recs[idx]
    lens = np.where(carry[idx], s["len"], 0).astype(np.int64)
    starts = np.repeat(s["bases_off"].astype(np.int64) - (np.cumsum(lens) - lens), lens)
    at = starts + np.arange(int(lens.sum()))
    body = {"edit_index": idx.astype(np.float64), "edit_contig": s["contig"].astype(np.float64),
            "edit_draft_pos": s["draft_pos"].astype(np.float64)}
    for f in ("len", "support", "kind", "draft_base", "new_base", "n_alt", "alt_base", "alt_support"):
        body["edit_" + f] = s[f].astype(np.float32)
    body["edit_bases"] = np.frombuffer(pool, dtype=np.uint8)[at].astype(np.float32)
    _save(out_dir, prefix, {**head, **body})


def dump_screen(out_dir, words, n, prefix="", limit=DUMP_LIMIT):
    """--dump-outputs of --screen-only: the screening bitmap of the n-byte batch (one bit per position, set where the
    k-mer starting there is absent from the filter: Stats.absent_kmers counts them).
      screen_absent_per_block  float64: set bits per 65536 positions, over the whole batch
      screen_word_index        float64 [S]: 64-bit words of the bitmap (all of them, or a fixed seeded sample)
      screen_word_lo / _hi     float64 [S]: their low / high 32 bits"""
    import numpy as np
    words = np.ascontiguousarray(words[:(n + 63) // 64]).view(np.uint64).copy()
    if n % 64:
        words[-1] &= np.uint64((1 << (n % 64)) - 1)
    pop = np.bitwise_count(words)
    per_block = np.add.reduceat(pop, np.arange(0, len(words), 1024), dtype=np.int64).astype(np.float64) \
        if len(words) else np.zeros(0)
    cap = max(0, (limit - per_block.nbytes - 4 * NPY_HEADER) // 24)
    nw = len(words)
    idx = np.arange(nw) if nw <= cap else np.sort(np.random.default_rng(DUMP_SEED).choice(nw, cap, replace=False))
    w = words[idx]
    _save(out_dir, prefix, {"screen_absent_per_block": per_block, "screen_word_index": idx.astype(np.float64),
                            "screen_word_lo": (w & np.uint64(0xFFFFFFFF)).astype(np.float64),
                            "screen_word_hi": (w >> np.uint64(32)).astype(np.float64)})


LAST_RANK_SECONDS = []  # per rank: its own seconds of the last timed_steps() (the value is the slowest rank's, barrier included)


def timed_steps(step, steps, world, dev, torch, dist, keep_last=False):
    """K steps bracketed by barrier + synchronize on both sides; returns (max-over-ranks seconds, per-step stats).
    keep_last: the last step keeps its result for --dump-outputs (freed after the clock instead of inside it)"""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    out = [step(keep=keep_last and i == steps - 1) for i in range(steps)]
    torch.cuda.synchronize()
    own = time.perf_counter() - t0  # this rank's own time, before it waits for the others
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    LAST_RANK_SECONDS[:] = [own]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        mine = torch.tensor([own], dtype=torch.float64, device=dev)
        every = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(every, mine)
        LAST_RANK_SECONDS[:] = [float(x.item()) for x in every]
    return elapsed, out


def main():
    args = parse()
    import numpy as np
    import torch
    import torch.distributed as dist
    import ntedit_amd
    from ntedit_amd import dist as ndist
    from ntedit_amd.synth import SyntheticJob

    rank, world, local = ndist.env_rank()
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d" % args.gpus)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # (rehearsal hook: NTEDIT_BENCH_BACKEND=gloo lets N ranks share the GPUs that are there -- RCCL refuses two
    # ranks on one device -- so the N>1 code path can be run on a 1-GPU box; the numbers then mean nothing)
    backend = os.environ.get("NTEDIT_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    ndist.init_process_group(backend)
    dev = torch.device("cuda", local)

    pol = ntedit_amd.Polisher(local)
    for kv in args.tune:
        key, _, val = kv.partition("=")
        pol.set_tuning(key, int(val))
    pol._lib.ntedit_hip_bind_near_device(local)  # this rank's host side on the socket its GPU hangs off
    mode_kw = {}
    if args.snv:
        mode_kw = dict(snv=1, max_insertions=0, max_deletions=0)
    if (args.snv or args.counting) and world > 1:
        raise SystemExit("--snv / --counting are single-GPU side lines")
    pol.set_params(ntedit_amd.default_params(start_grid=args.start_grid, screen_mode=args.screen_mode, **mode_kw))
    t_setup = time.perf_counter()
    # the same truth genome and the same draft on every rank; rank 0 builds the filter and broadcasts it (RCCL)
    shared = world > 1 or args.shared_filter
    if shared:
        fbuf = ndist.shared_filter(pol, args.filter_bytes, args.hashes, args.k)
        build = "insert" if rank == 0 else False
    else:
        build = "alloc"
    job = SyntheticJob(pol, args.bases, k=args.k, hash_num=args.hashes,
                       filter_bytes=args.filter_bytes // 8 if args.counting else args.filter_bytes,
                       seed=20251031, draft_seed=20251032, device=dev, build_filter=build,
                       contig_len=args.contig_len, structure=args.structure,
                       structure_fractions=json.loads(args.structure_fractions) if args.structure_fractions else None)
    counters = None
    if args.counting:
        # the plain filter's bit slots become 8-bit counters (1..4 for every truth k-mer); -p 2
        from ntedit_amd.synth import counting_filter_from_plain
        counters = counting_filter_from_plain(pol, args.k, args.hashes, device=dev)
        pol.set_params(ntedit_amd.default_params(start_grid=args.start_grid, screen_mode=args.screen_mode, min_threshold=2))
    if shared:
        ndist.broadcast_filter(fbuf, src=0)
    torch.cuda.synchronize()

    # ---- this rank's share of the draft (the whole batch at N=1)
    if world > 1:
        my_batch, my_offs, my_lens, my_halos, pieces = shard_batch(job, pol, rank, world, args.k, torch)
        my_bases = int(my_lens.astype(np.int64).sum() - my_halos.sum())
        n_cut = len(set(q.contig for q in pieces if q.n_seg > 1))
    else:
        my_batch, my_offs, my_lens, my_halos, pieces = job.batch, job.offsets, job.lens, None, None
        my_bases, n_cut = job.n_bases, 0
    my_bytes = int(my_batch.numel())
    torch.cuda.synchronize()
    weak_leg = args.full and world > 1 and not args.no_weak and not args.screen_only
    # start-up, untimed like the filter load: this rank's buffers + one internal warm-up batch (ntedit_hip_reserve)
    t_reserve = time.perf_counter()
    if not args.no_reserve:
        nres = max(my_bytes, int(job.n_bytes)) if weak_leg else my_bytes
        pol.reserve(nres, len(job.lens) + 64, on_device=1)
    t_reserve = time.perf_counter() - t_reserve
    t_setup = time.perf_counter() - t_setup

    launches = [1]
    cuts_rejected = [0]
    bitmap = None
    if args.screen_only:
        bitmap = torch.zeros((my_bytes + 63) // 64 + 1, dtype=torch.int64, device=dev)

    kept = []  # --dump-outputs: the last timed step's result

    def make_step(batch, offs, lens, nbytes, check_halos=None):
        def step(keep=False):
            if args.screen_only:
                return None, pol.screen_device(batch.data_ptr(), nbytes, bitmap.data_ptr())
            res = pol.polish_batch(None, offs, lens, device_ptr=batch.data_ptr(), n=nbytes)
            st = res.stats()
            if check_halos is not None:
                # (warm-up only) every cut of this rank's segments must verify, as the driver checks it
                ok = res.cuts_ok(lens, [(0, int(h), 0) for h in check_halos])
                # (the driver polishes such a segment again, joined with its successor; with the bench's filter
                # load none is expected -- a draft whose serial run ends early in a contig, as the reference's does
                # at false-positive rates of several percent, makes every later cut of that contig one)
                cuts_rejected[0] = int((~ok).sum())
            if keep:
                kept.append(res)
            else:
                res.free()
            launches[0] = max(1, int(st.screen_launches))
            return st, st.ms_screen
        return step

    step = make_step(my_batch, my_offs, my_lens, my_bytes)
    warm = make_step(my_batch, my_offs, my_lens, my_bytes, my_halos)
    for i in range(args.warmup):
        (warm if i == 0 and not args.screen_only else step)()
    elapsed, stats = timed_steps(step, args.steps, world, dev, torch, dist, keep_last=bool(args.dump_outputs))
    if args.dump_outputs:
        # (each rank its own share; at N>1 as rank<r>_<name>.npy, entries in the draft's contig numbering)
        prefix = "rank%d_" % rank if world > 1 else ""
        limit = DUMP_LIMIT // world
        if args.screen_only:
            dump_screen(args.dump_outputs, bitmap.cpu().numpy(), my_bytes, prefix, limit)
        else:
            res = kept.pop()
            host = my_batch.cpu().numpy()
            segments, n_entries = None, len(job.lens)
            if world > 1:
                mine = [q for q in pieces if q.owner == rank]
                segments = [(q.start, int(h), 0) for q, h in zip(mine, my_halos)]
            recs, pool = res.edits(host, my_offs, my_lens, segments)
            if world > 1:
                recs["contig"] = np.array([q.contig for q in mine], dtype=np.uint32)[recs["contig"]]
            dump_edits(args.dump_outputs, recs, pool, res.stats(), n_entries, prefix, limit)
            res.free()
            del host
    rank_ms_per_step = [round(x / args.steps * 1e3, 3) for x in LAST_RANK_SECONDS]
    screen_ms = [ms for _, ms in stats]
    machine_ms = [st.ms_machine for st, _ in stats if st is not None]
    last = stats[-1][0] if stats else None
    binned = bool(last is not None and last.screen_binned)
    probe_ms = [st.ms_probe for st, _ in stats if st is not None]
    part_ms = [st.ms_partition for st, _ in stats if st is not None]

    shard_bases = [my_bases]
    rejected_total = 0
    if world > 1:
        nb = torch.tensor([my_bases], dtype=torch.int64, device=dev)
        allnb = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(allnb, nb)
        shard_bases = [int(x.item()) for x in allnb]
        rj = torch.tensor([cuts_rejected[0]], dtype=torch.int64, device=dev)
        dist.all_reduce(rj, op=dist.ReduceOp.SUM)
        rejected_total = int(rj.item())
    total_bases = sum(shard_bases)

    # ---- weak-scaling leg (--full): every rank polishes the whole draft
    weak = None
    if weak_leg:
        wstep = make_step(job.batch, job.offsets, job.lens, job.n_bytes)
        wstep()
        w_elapsed, _ = timed_steps(wstep, args.steps, world, dev, torch, dist)
        weak = {"value": round(job.n_bases * world * args.steps / w_elapsed / 1e6, 2), "unit": "Mbases/s",
                "ms_per_step": round(w_elapsed / args.steps * 1e3, 3),
                "bases_per_gpu": job.n_bases, "note": "every rank polishes the whole draft (weak scaling)"}

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = total_bases * args.steps / elapsed / 1e6
        # Screening = the dominant part of a step.  Direct path: ONE kernel (k_screen), algorithmic bytes per k-mer
        # start = h filter bytes + 1 draft byte + 1/8 bitmap byte.  Binned path: the partition kernel and the
        # probe kernel, once per record chunk (ONE chunk at 3 Gbp); the dominant one is k_bin_probe, whose share of
        # those bytes is the h filter bytes + the bitmap byte/8 (the draft byte is read by the partition kernel);
        # the per-launch figures are what rocprofv3's
        # kernel stats average over.  `pipeline` prices the whole screening at the full 4.125 B per k-mer start.
        step_screen = sum(screen_ms) / len(screen_ms)
        if binned:
            step_probe = sum(probe_ms) / len(probe_ms)
            avg_screen = step_probe / launches[0]
            algo_bytes = (args.hashes + 0.125) * my_bytes / launches[0]
            dom_kernel = "k_bin_probe"
        else:
            avg_screen = step_screen / launches[0]
            algo_bytes = (args.hashes + 1 + 0.125) * my_bytes / launches[0]  # h filter B + 1 draft B + 1/8 bitmap B
            dom_kernel = "k_screen"
        achieved = algo_bytes / (avg_screen * 1e-3) / 1e9
        out = {
            "metric": "polished Mbases/s",
            "value": round(value, 2),
            "unit": "Mbases/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {
                "workload": "synthetic %.2f Gbp draft (%d contigs%s, 0.1%% sub + 0.01%% indel, 1 kbp N-run / 10 Mbp), "
                            "k=%d, %d-byte Bloom filter h=%d, %s" %
                            (job.n_bases / 1e9, len(job.lens),
                             " of %d bp" % args.contig_len if args.contig_len else " 50 kbp-50 Mbp",
                             args.k, args.filter_bytes, args.hashes,
                             "screen kernel only" if args.screen_only else
                             "screen + event extraction + event machine + edit records to host") +
                            (", GENOME-LIKE truth (" + ", ".join("%s %.1f%%" % (kk, 100.0 * vv / job.n_bases) for kk, vv in
                                                                job.structure.bases.items()) + " of the bases)"
                             if job.structure is not None else "") +
                            (", SNV mode (-s 1, -i 0 -d 0)" if args.snv else "") +
                            (", COUNTING filter (8-bit counters, synthetic contents 1..4, -p 2)" if args.counting else ""),
                "total_bases": total_bases,
                "workload_bytes": int(my_bytes),  # (batch bytes of this rank: what the counter records under profiles/ are keyed by)
                "k": args.k, "hashes": args.hashes, "filter_bytes": args.filter_bytes,
                "snv": bool(args.snv), "counting": bool(args.counting), "structure": args.structure,
                "parallelism": "ONE draft sharded over %d rank(s) by bases (LPT over pieces; %d contig(s) cut into "
                               "segments), filter broadcast once over RCCL (untimed)" % (world, n_cut),
                "shard_bases": shard_bases,
                "ms_per_step_by_rank": rank_ms_per_step,  # (each rank's own time; ms_per_step is the slowest one's, barriers included)
                "segment_cuts_rejected": rejected_total,
            },
            "roofline": {
                "bound": "hbm",
                "kernel": dom_kernel,
                "achieved": round(achieved, 2),
                "peak": 8000.0,
                "unit": "GB/s",
                "frac": round(achieved / 8000.0, 5),
                "traffic": None,
                "algorithmic_bytes_per_launch": int(algo_bytes),
                "avg_launch_ms": round(avg_screen, 3),
                "launches_per_step": launches[0],
                "probes_per_s": round(args.hashes * my_bytes / (step_screen * 1e-3), 0),
                "pipeline": {
                    "kernels": ["k_wc_scatter_b", "k_bin_probe", "k_ovf_probe"] if binned else ["k_screen"],
                    "ms_per_step": round(step_screen, 3),
                    "algorithmic_bytes_per_step": int((args.hashes + 1 + 0.125) * my_bytes),
                    "achieved": round((args.hashes + 1 + 0.125) * my_bytes / (step_screen * 1e-3) / 1e9, 2),
                    "frac": round((args.hashes + 1 + 0.125) * my_bytes / (step_screen * 1e-3) / 1e9 / 8000.0, 5),
                    "partition_ms": round(sum(part_ms) / len(part_ms), 3) if binned else None,
                    "probe_ms": round(sum(probe_ms) / len(probe_ms), 3) if binned else None,
                },
            },
            "setup_s": round(t_setup, 1),
            "reserve_s": round(t_reserve, 3),
        }
        if weak is not None:
            out["weak"] = weak
        # what the library's kernels were built from: counter records kept under profiles/ are quoted for this build only
        try:
            from ntedit_amd import _lib as _L
            build_id = _L.load().ntedit_hip_build_id().decode()
        except Exception:
            build_id = None
        out["build_id"] = build_id
        # HBM traffic of the dominant kernel's launches from the committed PMC run (bench.py cannot collect counters
        # itself); only quoted when it was taken on this exact workload AND this exact build of the kernels
        try:
            tr = json.load(open(os.path.join(ROOT, "profiles", "roofline_traffic.json")))
            kk = [k for k in tr["kernels"] if k.split("<")[0] == dom_kernel]
            if int(tr["workload_bytes"]) == int(my_bytes) and args.hashes == 3 and kk and \
                    int(tr["kernels"][kk[0]]["launches"]) % launches[0] == 0:
                if build_id is not None and tr.get("build_id") == build_id:
                    e = tr["kernels"][kk[0]]
                    out["roofline"]["traffic"] = int(e["fetch_bytes_per_launch"] + e["write_bytes_per_launch"])
                    out["roofline"]["traffic_source"] = tr["source"]
                    out["roofline"]["l2_hit_rate"] = round(e["tcc_hit_rate"], 4) if e.get("tcc_hit_rate") is not None else None
                else:
                    out["roofline"]["traffic_source"] = ("none: profiles/roofline_traffic.json was taken on build %s, this is %s"
                                                         % (tr.get("build_id"), build_id))
        except Exception:
            pass
        if last is not None:
            out["phases_ms"] = {"screen_launches_sum": round(step_screen, 3),
                                "machine_launches_sum": round(sum(machine_ms) / len(machine_ms), 3),
                                "other": round(ms_per_step - step_screen - sum(machine_ms) / len(machine_ms), 3)}
            out["events"] = {"absent_kmers": int(last.absent_kmers), "event_starts": int(last.events),
                             "skipped_as_overtaken": int(last.events_skipped),
                             "deferred_to_sweep_pass": int(last.events_deferred)}
        pps = None
        if args.full and not args.no_gather:
            try:
                pps, gms = pol.gather_bench(args.filter_bytes if args.filter_bytes & (args.filter_bytes - 1) == 0
                                            else 1 << 32, 4_000_000_000)
                out["roofline"]["random_gather_probes_per_s"] = round(pps, 0)
                out["roofline"]["frac_of_random_gather"] = round(out["roofline"]["probes_per_s"] / pps, 4)
            except Exception as e:  # pragma: no cover
                out["roofline"]["random_gather_error"] = str(e)
        # the edit search ("report probes/s only"): filter bytes gathered by the event-machine launches of one
        # step, counted lane by lane by the profile build (`make profile`, tools/gpu_machine_probes.sh) on this workload
        # and this build of the kernels, over the machine time of THIS run
        if last is not None and not args.screen_only:
            m_ms = sum(machine_ms) / len(machine_ms)
            mach = {"ms": round(m_ms, 3), "probes": None, "probes_per_s": None, "frac_of_random_gather": None}
            try:
                mp = json.load(open(os.path.join(ROOT, "profiles", "machine_probes.json")))
                want = {"workload_bytes": int(my_bytes), "k": args.k, "hashes": args.hashes, "filter_bytes": args.filter_bytes,
                        "snv": bool(args.snv), "counting": bool(args.counting)}
                rec = [r for r in mp["records"] if all(r.get(k2) == v for k2, v in want.items())]
                if rec and build_id is not None and rec[-1].get("build_id") == build_id:
                    r = rec[-1]
                    mach["probes"] = int(r["gathers_thread_launches"] + r["gathers_wave_launches"])
                    mach["probes_thread_launches"] = int(r["gathers_thread_launches"])
                    mach["probes_wave_launches"] = int(r["gathers_wave_launches"])
                    mach["probes_per_s"] = round(mach["probes"] / (m_ms * 1e-3), 0)
                    if pps:
                        mach["frac_of_random_gather"] = round(mach["probes_per_s"] / pps, 4)
                    mach["source"] = mp.get("source")
                elif rec:
                    mach["source"] = "none: profiles/machine_probes.json was taken on build %s, this is %s" % (rec[-1].get("build_id"), build_id)
            except Exception:
                pass
            out["roofline"]["machine"] = mach
        if args.full and world == 1 and not args.no_regions and not args.screen_only:
            out.update(measured_regions(job, pol, args))
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(job, pol, args)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    pol.close()


if __name__ == "__main__":
    main()
