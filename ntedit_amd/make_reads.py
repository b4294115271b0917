"""The reads k-mer filter of ntedit-make-reads-bf, built by N processes, each on its own GPU and its own share of the reads.

    python -m torch.distributed.run --nproc-per-node N -m ntedit_amd.make_reads --reads FILE... -k K (-c CMIN | --solid) ...
    python -m ntedit_amd.make_reads ...                                                          (one GPU)

The flags are ntedit-make-reads-bf's, with its refusals, plus --no-split (every input file is read whole by one process)
and --backend (torch.distributed backend; `gloo` lets N ranks share the GPUs there are, as in ntedit_amd.run).

Every rank plans the same partition from the file sizes: gzip files are whole units (weighted 4 x their size), plain
files are cut into byte ranges, and the units go to ranks longest first.  Each rank counts its units into a sketch of the
binary's size; the sketches merge by a saturating byte-wise sum (reduce-scatter: all_to_all of chunks, k_merge into the
chunk a rank owns, then all_gather).  min(255, sum_r min(255, c_r)) = min(255, sum_r c_r), so every rank then holds the
one-process sketch.  The histogram pass sums 256 integer bins; pass 2 writes per-rank filters that merge by OR (plain)
or max (--counts) into the one-process filter.  The output is byte-identical to the binary's for every world size and
partition, or the run is refused: after pass 1 every range's stop must be the next range's start (see
ntedit_hip_reads_pass), which multi-line FASTQ can break -- then nothing is written and --no-split is the way out.
With --reject_cutoff the same pass 2 fills a second plain filter per rank (the reject filter for ntedit -e), merged by OR
like the first and written by rank 0 to --reject_out.
Only rank 0 writes files.  The per-rank build is build_rank, which `python -m ntedit_amd.run --reads` shares: there it
keeps the reads resident in HBM after pass 1 and builds into the context that then polishes.
"""
import ctypes
import os
import sys
import time

import numpy as np

from . import _lib
from . import dist as ndist

WHOLE = (1 << 64) - 1  # `end` of a unit that is a whole file
ROUND_BYTES = 256 << 20  # exchange rounds: at most this many bytes per peer and round, whatever the array size
BATCH_DEFAULT = _lib.READS_BATCH_DEFAULT
RESIDENT_CAP_DEFAULT = _lib.READS_RESIDENT_CAP_DEFAULT  # the resident store's cap of `ntedit --reads`

USAGE = ("Usage: python -m ntedit_amd.make_reads [--help] --reads VAR... -k VAR (-c VAR | --solid) [--hist VAR] "
         "[--counts] [--hashes VAR] [--fpr VAR] [--bf VAR] [--num_elements VAR] [--sketch_bytes VAR] [--gpu_parse] [-o VAR] "
         "[-t VAR] [--reject_cutoff VAR] [--reject_bf VAR] [--reject_num_elements VAR] [--reject_out VAR] [--min_qual VAR] "
         "[--min_read_len VAR] [--min_mean_qual VAR] [--min_rq VAR] [--no-split] "
         "[--backend VAR]\n\n"
         "ntedit-make-reads-bf on N processes (python -m torch.distributed.run --nproc-per-node N -m "
         "ntedit_amd.make_reads ...): the same flags, the same output bytes.\n"
         "  --no-split      read every input file whole (by one process); gzip files always are\n"
         "  --reject_cutoff also write the reject filter for ntedit -e (the k-mers seen at least this many times), from\n"
         "                  the same pass 2; --reject_bf / --reject_num_elements size it, --reject_out names it\n"
         "                  [default: reads_k<K>_reject.bf]\n"
         "  --gpu_parse     parse plain and bgzip-compressed (BGZF) read files on the GPU: the host ships the file's bytes,\n"
         "                  BGZF still compressed; same output (single-stream gzip stays with the host parser).  BAM files,\n"
         "                  unaligned or aligned, need it; a BAM is read whole by one process, as gzip files are\n"
         "  --min_qual      minimum base quality, 1 to 93 (Phred+33; Phred+64 is not built): a base below it counts as N in\n"
         "                  every rank alike, so the output bytes are the same for every world size\n"
         "  --min_read_len  minimum read length, 1 to 2147483647 (the shortest read kept is the larger of it and k)\n"
         "  --min_mean_qual minimum mean read quality, 1 to 60: the Phred value of the read's mean error probability\n"
         "  --min_rq        minimum read accuracy, above 0 and at most 1: a BAM read whose rq tag is below it is dropped;\n"
         "                  reads without the tag pass.  The three drop the same reads on every rank\n"
         "  --backend       torch.distributed backend (default nccl = RCCL; gloo: N ranks may share a GPU)\n"
         "ntedit-make-reads-bf --help describes the other flags.\n")


class Refused(Exception):
    pass


def _is_option(a):
    return len(a) > 1 and a[0] == "-" and not a[1].isdigit()


def check_options(dialect, given, final, reads=(), solid=False, hist="", gpu_parse=False, counts=False, reject_out=False):
    """The library's reads-option rules (ntedit_hip_reads_options_check) over the option texts given so far (name ->
    text).  final: every rule, and the argument dict of build_rank; else only what is refused at the option itself.
    Refused with the library's message; the tool's "would be empty" is kept in the dict for sizes() to refuse."""
    lib = _lib.load()
    files = (ctypes.c_char_p * max(1, len(reads)))(*[os.fsencode(f) for f in reads])
    own = {name: text for name, text in given.items() if name not in _lib.READS_FILTER_OPTION_TEXTS}
    o = _lib.ReadsOptions(solid=solid, hist=bool(hist), files=files, n_files=len(reads), gpu_parse=bool(gpu_parse),
                          counts=bool(counts), reject_out=bool(reject_out),
                          **{name: os.fsencode(text) for name, text in own.items()})
    r = _lib.ReadsRules()
    rc = lib.ntedit_hip_reads_options_check(o, dialect, int(final), r)
    why = os.fsdecode(lib.ntedit_hip_reads_last_error(None)) if rc else None
    if rc not in (0, _lib.READS_EMPTY):
        raise Refused(why)
    # the read filter's options, behind them (a struct and a call of their own)
    fo = _lib.ReadsFilterOptions(**{name: os.fsencode(given[name]) for name in _lib.READS_FILTER_OPTION_TEXTS if name in given})
    fr = _lib.ReadsFilterRules()
    if lib.ntedit_hip_reads_filter_options_check(fo, dialect, int(final), fr) != 0:
        raise Refused(os.fsdecode(lib.ntedit_hip_reads_last_error(None)))
    return dict(reads=list(reads), k=r.k, cmin=r.cmin if "cutoff" in given else None, solid=solid, hist=hist,
                hashes=r.hash_num, fpr=r.fpr, bf=r.bf_bytes if "bf" in given else None,
                num_elements=r.num_elements if "num_elements" in given else None, sketch_bytes=r.sketch_bytes,
                batch_bytes=r.batch_bytes, store_cap=r.store_cap, threads=r.threads, gather_hist=bool(r.gather_hist),
                size_from_hist=bool(r.size_from_hist), bf_bytes=r.bf_bytes, sketch=r.sketch_counters, empty=why,
                gpu_parse=bool(r.gpu_parse), reject_cmin=r.reject_cmin, reject_bf_bytes=r.reject_bf_bytes,
                reject_num_elements=r.reject_num_elements, reject_size_from_hist=bool(r.reject_size_from_hist),
                min_qual=r.min_qual, min_read_len=fr.min_read_len, min_mean_qual=fr.min_mean_qual, min_rq=fr.min_rq)


def read_filter_on(a):
    """--min_read_len, --min_mean_qual or --min_rq was given"""
    return bool(a.get("min_read_len") or a.get("min_mean_qual") or a.get("min_rq"))


def parse(argv):
    """ntedit-make-reads-bf's arguments, walked as it walks them (host/make_reads_bf.cpp); the rules are the library's"""
    texts = {"-k": "k", "-c": "cutoff", "--hashes": "hashes", "--fpr": "fpr", "--bf": "bf",
             "--num_elements": "num_elements", "--sketch_bytes": "sketch_bytes", "-t": "threads",
             "--batch_bytes": "batch_bytes", "--reject_cutoff": "reject_cutoff", "--reject_bf": "reject_bf",
             "--reject_num_elements": "reject_num_elements", "--min_qual": "min_qual",
             "--min_read_len": "min_read_len", "--min_mean_qual": "min_mean_qual", "--min_rq": "min_rq"}  # (--batch_bytes is not in the usage text: tests force small batches with it)
    own = dict(counts=False, out="", reject_out="", no_split=False, backend=None, help=False)
    given, reads, solid, hist, gpu_parse = {}, [], False, "", False
    i = 0
    while i < len(argv):
        x = argv[i]

        def value(name):
            nonlocal i
            if i + 1 >= len(argv):
                raise Refused("Too few arguments for '%s'." % name)
            i += 1
            return argv[i]

        if x in ("-h", "--help"):
            return dict(own, help=True)
        elif x == "--reads":
            while i + 1 < len(argv) and not _is_option(argv[i + 1]):
                i += 1
                reads.append(argv[i])
        elif x in texts:
            given[texts[x]] = value(x)
            check_options(_lib.READS_DIALECT_TOOL, given, False)
        elif x == "--solid":
            solid = True
        elif x == "--hist":
            hist = value("--hist")
        elif x == "--gpu_parse":
            gpu_parse = True
        elif x == "--counts":
            own["counts"] = True
        elif x == "-o":
            own["out"] = value("-o")
        elif x == "--reject_out":
            own["reject_out"] = value("--reject_out")
        elif x == "--no-split":
            own["no_split"] = True
        elif x == "--backend":
            own["backend"] = value("--backend")
        else:
            raise Refused("Unknown argument: " + x)
        i += 1
    if not reads:
        raise Refused("--reads: 1 or more argument(s) expected. 0 provided.")
    a = dict(check_options(_lib.READS_DIALECT_TOOL, given, True, reads, solid, hist, gpu_parse, own["counts"],
                           bool(own["reject_out"])), **own)
    if not a["out"]:
        a["out"] = "reads_k%d.bf" % a["k"]
    if not a["reject_out"]:
        a["reject_out"] = "reads_k%d_reject.bf" % a["k"]
    return a


def sizes(lib, a):
    """(output bytes or 0 when the histogram sizes it, sketch counters): the binary's sizing, as the rules gave it"""
    if a["empty"]:
        raise Refused(a["empty"])
    return a["bf_bytes"], a["sketch"]


# ---------------------------------------------------------------------------------- partition
class Unit:
    __slots__ = ("file", "path", "begin", "end", "weight")

    def __init__(self, file, path, begin, end, weight):
        self.file, self.path, self.begin, self.end, self.weight = file, path, begin, end, weight

    def key(self):
        return (self.file, self.begin)

    def __repr__(self):
        return "Unit(%d, %d, %s, w=%d)" % (self.file, self.begin, "end" if self.end == WHOLE else self.end, self.weight)


def file_facts(lib, paths):
    """[(bytes, gzip)] of every input; a file that is not a regular file counts 0 bytes and stays whole"""
    out = []
    for p in paths:
        try:
            st = os.stat(p)
            regular = (st.st_mode & 0o170000) == 0o100000
        except OSError:
            regular = False
        if not regular:
            out.append((0, True))
            continue
        out.append((st.st_size, bool(lib.ntedit_hip_reads_is_gzip(p.encode()))))
    return out


def plan(paths, facts, world, split=True):
    """The same units on every rank, from the file facts alone: gzip files whole, plain files cut into ranges of about a
    quarter of a rank's share; then owner[u] for every unit, longest first (dist.lpt_assign).  -> (units, owner)"""
    weights = [n * (_lib.READS_GZIP_WEIGHT if gz else 1) for n, gz in facts]
    target = max(1, -(-sum(weights) // (4 * world)))
    units = []
    for i, (p, (n, gz)) in enumerate(zip(paths, facts)):
        pieces = 1 if (gz or not split or world == 1 or n == 0) else max(1, -(-n // target))
        if pieces == 1:
            units.append(Unit(i, p, 0, WHOLE, weights[i]))
            continue
        cuts = [n * j // pieces for j in range(pieces + 1)]
        for j in range(pieces):
            units.append(Unit(i, p, cuts[j], cuts[j + 1], cuts[j + 1] - cuts[j]))
    return units, ndist.lpt_assign([u.weight for u in units], world)


def check_cuts(records):
    """records: (file, begin, start, next) of every unit of every rank.  The ranges of a file read it as one reader would
    exactly when each range's stop is the next range's start; -> a message naming the first break, or None"""
    by_file = {}
    for f, begin, start, nxt in records:
        by_file.setdefault(f, []).append((begin, start, nxt))
    for f in sorted(by_file):
        rs = sorted(by_file[f])
        for (b0, _, nxt), (b1, start, _) in zip(rs, rs[1:]):
            if nxt != start:
                return (f, b0, b1, nxt, start)
    return None


# ---------------------------------------------------------------------------------- the run
def log_info(msg):
    sys.stderr.write("[%s] [INFO] %s\n" % (time.strftime("%Y-%m-%d %H:%M:%S"), msg))
    sys.stderr.flush()


class Builder:
    """one rank's state: the context it builds in (a Polisher's, owned by the caller), the process group, and what its
    exchanges measured"""

    def __init__(self, a, rank, world, pol, group, name="make_reads"):
        self.a, self.rank, self.world, self.group, self.name = a, rank, world, group, name
        self.lib, self.h = pol._lib, pol._h
        self.xbytes, self.xsec = 0, 0.0
        self.exchanges = []

    def fail(self, what):
        raise RuntimeError("%s: %s: %s" % (self.name, what, self.lib.ntedit_hip_reads_last_error(self.h).decode()))

    # ------------------------------------------------------------------ collectives (gloo: through host memory)
    def _gloo(self):
        import torch.distributed as dist
        return dist.get_backend() == "gloo"

    def all_gather_object(self, obj):
        import torch.distributed as dist
        if self.group is None:
            return [obj]
        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def merge(self, t, op):
        """t: this rank's array (world x S bytes, S a multiple of 16) -> on return every rank holds the fold of all ranks'
        arrays: a reduce-scatter (all_to_all of chunks, k_merge into the chunk this rank owns), then an all_gather; in
        rounds of at most ROUND_BYTES per peer"""
        import torch
        import torch.distributed as dist
        if self.group is None:
            return
        t0 = time.perf_counter()
        w, r = self.world, self.rank
        s = t.numel() // w
        view = t.view(w, s)
        gloo = self._gloo()
        torch.cuda.synchronize()
        for o in range(0, s, ROUND_BYTES):
            p = min(ROUND_BYTES, s - o)
            send = view[:, o:o + p].contiguous()
            if gloo:
                recv_h = torch.empty(send.shape, dtype=torch.uint8)
                dist.all_to_all_single(recv_h, send.cpu())
                recv = recv_h.to(t.device)
            else:
                recv = torch.empty_like(send)
                dist.all_to_all_single(recv, send)
            torch.cuda.synchronize()
            dst = view[r, o:o + p]
            if self.lib.ntedit_hip_merge_bytes(self.h, dst.data_ptr(), recv.data_ptr(), w, p, op) != 0:
                self.fail("merge")
            del send, recv
        for o in range(0, s, ROUND_BYTES):
            p = min(ROUND_BYTES, s - o)
            mine = view[r, o:o + p]
            if gloo:
                outs = [torch.empty(p, dtype=torch.uint8) for _ in range(w)]
                dist.all_gather(outs, mine.cpu())
                flat = torch.stack(outs).to(t.device)
            else:
                flat = torch.empty(w * p, dtype=torch.uint8, device=t.device)
                dist.all_gather_into_tensor(flat, mine)
            view[:, o:o + p].copy_(flat.view(w, p))
            del flat
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        moved = 2 * (w - 1) * s  # bytes this rank sent: its w - 1 foreign chunks, then its own chunk to w - 1 peers
        self.xbytes += moved
        self.xsec += sec
        what = {0: "sat-add", 1: "or", 2: "max"}[op]
        self.exchanges.append(dict(op=what, bytes=t.numel(), sent=moved, ms=round(sec * 1e3, 3)))
        log_info("rank %d/%d: exchange %s of %d bytes: %d bytes sent, %.1f ms (%s)"
                 % (r, w, what, t.numel(), moved, sec * 1e3, "gloo via host" if gloo else "rccl"))

    def all_reduce_hist(self, occ):
        import torch
        import torch.distributed as dist
        if self.group is None:
            return occ
        t0 = time.perf_counter()
        t = torch.from_numpy(occ.astype(np.int64))
        if not self._gloo():
            t = t.cuda()
        dist.all_reduce(t)
        out = t.cpu().numpy().astype(np.uint64)
        self.exchanges.append(dict(op="sum", bytes=occ.nbytes, sent=occ.nbytes,
                                   ms=round((time.perf_counter() - t0) * 1e3, 3)))
        return out

    def padded(self, nbytes):
        q = 16 * self.world
        return -(-nbytes // q) * q


@_lib.READS_LOG_FN
def _log_line(user, to_stdout, line):
    """the stages' console lines (a sharded build keeps its standard output for its results)"""
    log_info(line.decode())


def build_rank(pol, a, rank, world, group, slot=0, use_store=False, store_cap=RESIDENT_CAP_DEFAULT, name="make_reads"):
    """One rank's share of the reads filter build, the same for every driver: the stages of ntedit_hip_reads_build with
    the merges in between.  The plan, the count stage over this rank's units into an adopted sketch, the cut-point
    check, the sketch merge, with --solid / --hist the histogram stage and the sum of the ranks' bins, the decide stage
    (rank 0 writes --hist), the insert stage into an adopted filter in `slot` of pol's context, the filter merge.  On
    return every rank holds the whole filter there and the sketch is freed.  With use_store the reads of pass 1 stay
    resident in HBM (up to store_cap bytes) and the later passes read the store; a rank whose store was released
    reads its ranges again, with the same result.  The stages fill the PRIMARY slot, so that is the only slot a build
    can fill.  With a reject cutoff (a["reject_cmin"]) the same pass 2 fills a second adopted tensor in the SECONDARY
    slot, merged with OR as the primary is; pol keeps it alive (dist._keep).
    -> (the filter tensor, which the caller keeps alive while the slot is in use, a report dict)"""
    import torch
    if slot != 0:
        raise ValueError("build_rank: pass 2 from the files fills the PRIMARY slot (0) only")
    lib = pol._lib
    bf, sketch = sizes(lib, a)
    reject = a.get("reject_cmin") or 0
    facts = file_facts(lib, a["reads"])
    units, owner = plan(a["reads"], facts, world, split=not a["no_split"])
    mine = [u for u, o in zip(units, owner) if o == rank]
    mine.sort(key=Unit.key)
    if rank == 0:
        log_info("%d ranks, %d units (%d input files), sketch %d counters, %s" %
                 (world, len(units), len(a["reads"]), sketch,
                  "output from the k-mer histogram" if a["size_from_hist"] else "output %d bytes" % bf) +
                 ("" if not reject else ", reject filter at %d, %s" % (
                     reject, "from the k-mer histogram" if a["reject_size_from_hist"] else "%d bytes" % a["reject_bf_bytes"])))
    b = Builder(a, rank, world, pol, group, name)
    n = len(mine)
    u64s = ctypes.c_uint64 * max(n, 1)
    starts, nexts = u64s(), u64s()
    args = _lib.ReadsBuildArgs(
        files=(ctypes.c_char_p * max(n, 1))(*[u.path.encode() for u in mine]), n_files=n,
        begins=u64s(*[u.begin for u in mine]), ends=u64s(*[u.end for u in mine]), rank=rank, world=world, k=a["k"],
        hash_num=a["hashes"], cmin=a["cmin"] or 0, solid=a["solid"], counts=a["counts"], bf_bytes=bf, fpr=a["fpr"],
        batch_bytes=a["batch_bytes"], hist_path=a["hist"].encode() or None, use_store=use_store, store_cap=store_cap,
        log=_log_line, device_parse=bool(a.get("gpu_parse")), reject_cmin=reject,
        reject_bf_bytes=a.get("reject_bf_bytes") or 0, reject_num_elements=a.get("reject_num_elements") or 0,
        min_qual=a.get("min_qual") or 0)
    # the read filter is the context's setting (no field of the build's arguments): every pass of this build follows it
    if lib.ntedit_hip_reads_set_read_filter(b.h, a.get("min_read_len") or 0, a.get("min_mean_qual") or 0, a.get("min_rq") or 0.0):
        raise RuntimeError("reads_set_read_filter: " + os.fsdecode(lib.ntedit_hip_reads_last_error(b.h)))
    res = _lib.ReadsBuildResult()
    parsed = {}

    def note_parse(key):
        # --min_qual: what the pass that just ran masked (ntedit_hip_reads_min_qual_info: the last pass)
        with_qual, masked = ctypes.c_uint64(), ctypes.c_uint64()
        if a.get("min_qual") and lib.ntedit_hip_reads_min_qual_info(b.h, with_qual, masked) == 0:
            parsed.setdefault(key, {})["min_qual"] = dict(q=a["min_qual"], qual_bases=with_qual.value,
                                                          masked_bases=masked.value)
        # the read filter: what the records of the pass that just ran came to (ntedit_hip_reads_read_filter_info)
        fs = _lib.ReadsReadFilterStats()
        if read_filter_on(a) and lib.ntedit_hip_reads_read_filter_info(b.h, fs) == 0:
            parsed.setdefault(key, {})["read_filter"] = dict(
                min_read_len=a.get("min_read_len") or 0, min_mean_qual=a.get("min_mean_qual") or 0,
                min_rq=a.get("min_rq") or 0.0, **fs.as_dict())
        # --gpu_parse: what the pass that just ran parsed where (ntedit_hip_reads_parse_info: the last pass)
        st = _lib.ReadsParseStats()
        if a.get("gpu_parse") and lib.ntedit_hip_reads_parse_info(b.h, st) == 0:
            parsed.setdefault(key, {}).update(device_chunks=st.device_chunks, fallback_chunks=st.fallback_chunks,
                                              raw_bytes=st.raw_bytes, text_bytes=st.text_bytes,
                                              kernel_ms=round(st.ms_kernels, 3), broken=st.broken, host_files=st.host_files)
            zs = _lib.ReadsInflateStats()  # ... and, of BGZF inputs, what it inflated on the device
            if lib.ntedit_hip_reads_inflate_info(b.h, zs) == 0 and zs.files:
                parsed[key]["bgzf"] = dict(files=zs.files, members=zs.members, compressed_bytes=zs.comp_bytes,
                                           inflated_bytes=zs.raw_bytes, kernel_ms=round(zs.ms_kernels, 3),
                                           handed_back=zs.handed_back)
            bs = _lib.ReadsBamStats()  # ... and, of BAM inputs, what it walked and decoded there
            if lib.ntedit_hip_reads_bam_info(b.h, bs) == 0 and bs.files:
                parsed[key]["bam"] = dict(files=bs.files, chunks=bs.chunks, records=bs.records, kept=bs.kept,
                                          skipped_flag=bs.skipped_flag, skipped_short=bs.skipped_short,
                                          segments=bs.segments, rewalked=bs.rewalked, walk_ms=round(bs.ms_walk, 3),
                                          decode_ms=round(bs.ms_decode, 3))
    try:
        k, hashes = a["k"], a["hashes"]
        counters = (sketch + 7) // 8 * 8
        sk = torch.zeros(b.padded(counters), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if lib.ntedit_hip_sketch_set_device(b.h, sk.data_ptr(), counters, hashes, k) != 0:
            b.fail("sketch")
        if lib.ntedit_hip_reads_stage_count(b.h, args, res, starts, nexts) != 0:
            b.fail("pass 1 (count)")
        note_parse("1")
        cut = [(u.file, u.begin, starts[i], nexts[i]) for i, u in enumerate(mine)]
        brk = check_cuts([c for part in b.all_gather_object(cut) for c in part])
        if brk is not None:
            f, b0, b1, nxt, start = brk
            raise Refused("%s: the ranges at bytes %d and %d do not meet (the first stops before byte %s, the second "
                          "starts at byte %d): this file cannot be cut into ranges (multi-line FASTQ?); run with "
                          "--no-split, which reads every file whole.  No output was written."
                          % (a["reads"][f], b0, b1, "(a failed record)" if nxt == WHOLE else nxt, start))
        b.merge(sk, _lib.MERGE_SAT_ADD)
        occ = None
        if a["gather_hist"]:
            occ = np.zeros(256, dtype=np.uint64)
            if lib.ntedit_hip_reads_stage_histogram(b.h, args, res, occ.ctypes.data) != 0:
                b.fail("pass H (histogram)")
            if res.store_state != _lib.RESIDENT_ON:
                note_parse("H")
            occ = b.all_reduce_hist(occ)
        rc = lib.ntedit_hip_reads_stage_decide(args, None if occ is None else occ.ctypes.data, res)
        if rc != 0:
            why = lib.ntedit_hip_reads_last_error(None).decode()
            raise Refused(why) if rc == _lib.E_ARG else RuntimeError(why)
        nbytes = (res.bf_bytes + 7) // 8 * 8
        out = torch.zeros(b.padded(nbytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pol.set_filter_device(out.data_ptr(), nbytes, hashes, k, slot=slot, counting=a["counts"])
        out2, nbytes2 = None, 0
        if reject:
            nbytes2 = (res.reject_bf_bytes + 7) // 8 * 8
            out2 = torch.zeros(b.padded(nbytes2), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            pol.set_filter_device(out2.data_ptr(), nbytes2, hashes, k, slot=1, counting=False)
            ndist._keep(pol, 1, out2)
        if lib.ntedit_hip_reads_stage_insert(b.h, args, res) != 0:  # (it frees the sketch, and the store with it)
            b.fail("pass 2 (solid k-mers)")
        if res.store_state != _lib.RESIDENT_ON:
            note_parse("2")
        del sk
        b.merge(out, _lib.MERGE_MAX if a["counts"] else _lib.MERGE_OR)
        if reject:
            b.merge(out2, _lib.MERGE_OR)
    finally:
        lib.ntedit_hip_sketch_free(b.h)
    on = res.store_state == _lib.RESIDENT_ON
    passes = {key: dict(bases=p.bases, ms=round(p.ms_wall, 3), gpu_ms=round(p.ms_gpu, 3))
              for key, p in zip("1H2", res.passes) if key != "H" or a["gather_hist"]}
    rep = dict(units=n, store=dict(used=on, state=("off", "on", "over cap", "no memory")[res.store_state] if use_store
                                   else "not asked", batches=res.store_batches, bytes=res.store_bytes,
                                   fallback=use_store and not on),
               cmin=res.cmin, filter_bytes=nbytes, passes=passes, exchanges=b.exchanges, exchange_bytes=b.xbytes,
               exchange_ms=round(b.xsec * 1e3, 3))
    if a.get("gpu_parse") or a.get("min_qual") or read_filter_on(a):
        rep["parse"] = parsed
    if reject:
        rep["reject"] = dict(cutoff=reject, filter_bytes=nbytes2, merge_ms=b.exchanges[-1]["ms"] if group is not None else 0.0)
    return out, rep


def build(a, lib, rank, world, local, group):
    from .polisher import Polisher
    pol = Polisher(local)
    try:
        out, rep = build_rank(pol, a, rank, world, group)
        if rank == 0:
            occupied, slots = pol.filter_occupancy(0)
            print("Bloom filter FPR: %g" % ((occupied / slots) ** a["hashes"]), flush=True)
            if lib.ntedit_hip_filter_save_file(pol._h, 0, a["out"].encode()) != 0:
                raise RuntimeError("cannot write " + a["out"])
            log_info("rank 0: filter (%d bytes) written to %s; exchanges %d bytes sent in %.1f ms"
                     % (rep["filter_bytes"], a["out"], rep["exchange_bytes"], rep["exchange_ms"]))
            if a.get("reject_cmin"):
                occupied, slots = pol.filter_occupancy(1)
                print("Reject Bloom filter FPR: %g" % ((occupied / slots) ** a["hashes"]), flush=True)
                if lib.ntedit_hip_filter_save_file(pol._h, 1, a["reject_out"].encode()) != 0:
                    raise RuntimeError("cannot write " + a["reject_out"])
                log_info("rank 0: reject filter (%d bytes, k-mers seen at least %d times) written to %s"
                         % (rep["reject"]["filter_bytes"], a["reject_cmin"], a["reject_out"]))
        if group is not None:
            import torch.distributed as dist
            dist.barrier()
        del out
    finally:
        pol.close()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    # torch's HIP runtime first, as in ntedit_amd.run: the library then binds to the runtime torch brought in
    # (loaded the other way round, the library's context cannot see the device in a torch.distributed.run child)
    import torch
    import torch.distributed as dist
    try:
        a = parse(argv)
        if a["help"]:
            sys.stderr.write(USAGE)
            return 0
        lib = _lib.load()
        sizes(lib, a)  # (the empty-output refusal comes before any device)
    except Refused as e:
        sys.stderr.write("%s\n%s" % (e, USAGE))
        return 1
    if not torch.cuda.is_available():
        sys.stderr.write("make_reads: error: no HIP device (this build has no CPU path)\n")
        return 1
    rank, world, local = ndist.env_rank()
    if (a["backend"] or "nccl") != "nccl":
        local = local % torch.cuda.device_count()  # (gloo rehearsal: ranks share the GPUs there are)
    torch.cuda.set_device(local)
    group = None
    if world > 1 or "RANK" in os.environ or a["backend"]:
        ndist.init_process_group(a["backend"] or "nccl", port=29517, single=True)
        group = dist.group.WORLD
    try:
        return build(a, lib, rank, world, local, group)
    except Refused as e:
        sys.stderr.write("make_reads: error: %s\n" % e)
        return 1
    finally:
        if group is not None:
            dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
