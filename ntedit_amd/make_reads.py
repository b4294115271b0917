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
GZIP_WEIGHT = 4  # a gzip byte weighs as much as 4 plain ones (the binary's default sketch counts it so)
ROUND_BYTES = 256 << 20  # exchange rounds: at most this many bytes per peer and round, whatever the array size
BATCH_DEFAULT = 256 << 20
RESIDENT_CAP_DEFAULT = 48 << 30  # the resident store's cap of `ntedit --reads` (128 Gbases at 3 bits per base)
PASS_NAMES = {_lib.READS_PASS_COUNT: "1 (count)", _lib.READS_PASS_HIST: "H (histogram)",
              _lib.READS_PASS_SOLID: "2 (solid k-mers)"}

USAGE = ("Usage: python -m ntedit_amd.make_reads [--help] --reads VAR... -k VAR (-c VAR | --solid) [--hist VAR] "
         "[--counts] [--hashes VAR] [--fpr VAR] [--bf VAR] [--num_elements VAR] [--sketch_bytes VAR] [-o VAR] [-t VAR] "
         "[--no-split] [--backend VAR]\n\n"
         "ntedit-make-reads-bf on N processes (python -m torch.distributed.run --nproc-per-node N -m "
         "ntedit_amd.make_reads ...): the same flags, the same output bytes.\n"
         "  --no-split      read every input file whole (by one process); gzip files always are\n"
         "  --backend       torch.distributed backend (default nccl = RCCL; gloo: N ranks may share a GPU)\n"
         "ntedit-make-reads-bf --help describes the other flags.\n")


class Refused(Exception):
    pass


def _is_option(a):
    return len(a) > 1 and a[0] == "-" and not a[1].isdigit()


def _u64(name, v):
    if not v or not v.isdigit():
        raise Refused("%s: not a number: '%s'" % (name, v))
    return int(v)


def parse(argv):
    """ntedit-make-reads-bf's argument rules and messages (host/make_reads_bf.cpp), checked in the same order"""
    a = dict(reads=[], k=None, cmin=None, solid=False, hist="", counts=False, hashes=3, fpr=0.01, bf=None,
             num_elements=None, sketch_bytes=0, out="", threads=12, batch_bytes=BATCH_DEFAULT, no_split=False,
             backend=None, help=False)
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
            a["help"] = True
            return a
        elif x == "--reads":
            while i + 1 < len(argv) and not _is_option(argv[i + 1]):
                i += 1
                a["reads"].append(argv[i])
        elif x == "-k":
            a["k"] = _u64("-k", value("-k"))
        elif x == "-c":
            a["cmin"] = _u64("-c", value("-c"))
        elif x == "--solid":
            a["solid"] = True
        elif x == "--hist":
            a["hist"] = value("--hist")
        elif x == "--counts":
            a["counts"] = True
        elif x == "--hashes":
            a["hashes"] = _u64("--hashes", value("--hashes"))
        elif x == "--fpr":
            v = value("--fpr")
            try:
                a["fpr"] = float(v)
            except ValueError:
                a["fpr"] = float("nan")
            if not (0.0 < a["fpr"] < 1.0):
                raise Refused("--fpr: needs a number between 0 and 1: '%s'" % v)
        elif x == "--bf":
            a["bf"] = _u64("--bf", value("--bf"))
        elif x == "--num_elements":
            a["num_elements"] = _u64("--num_elements", value("--num_elements"))
        elif x == "--sketch_bytes":
            a["sketch_bytes"] = _u64("--sketch_bytes", value("--sketch_bytes"))
        elif x == "--batch_bytes":  # (not in the usage text: tests force many small batches with it)
            a["batch_bytes"] = _u64("--batch_bytes", value("--batch_bytes"))
        elif x == "-o":
            a["out"] = value("-o")
        elif x == "-t":
            a["threads"] = _u64("-t", value("-t"))
        elif x == "--no-split":
            a["no_split"] = True
        elif x == "--backend":
            a["backend"] = value("--backend")
        else:
            raise Refused("Unknown argument: " + x)
        i += 1
    if not a["reads"]:
        raise Refused("--reads: 1 or more argument(s) expected. 0 provided.")
    if a["k"] is None:
        raise Refused("-k: required.")
    if not 12 <= a["k"] <= 200:
        raise Refused("-k %d: k must be between 12 and 200." % a["k"])
    if a["solid"] and a["cmin"] is not None:
        raise Refused("--solid and -c: give one of them (--solid takes the minimum count from the k-mer histogram).")
    if a["cmin"] is None and not a["solid"]:
        raise Refused("-c: required (or --solid).")
    if a["cmin"] is not None and not 1 <= a["cmin"] <= 255:
        raise Refused("-c %d: the minimum count must be between 1 and 255." % a["cmin"])
    if not 1 <= a["hashes"] <= 8:
        raise Refused("--hashes %d: the number of hash functions must be between 1 and 8." % a["hashes"])
    a["gather_hist"] = a["solid"] or bool(a["hist"])
    a["size_from_hist"] = a["bf"] is None and a["num_elements"] is None
    if a["size_from_hist"] and not a["gather_hist"]:
        raise Refused("--bf or --num_elements: one of them is required (or --solid / --hist, which size the filter "
                      "from the k-mer histogram).")
    if a["batch_bytes"] < 4096:
        raise Refused("--batch_bytes: at least 4096.")
    if not a["out"]:
        a["out"] = "reads_k%d.bf" % a["k"]
    return a


def sizes(lib, a):
    """(output bytes or 0 when the histogram sizes it, sketch counters): the binary's sizing, through its own calls"""
    bf = 0
    if a["bf"] is not None:
        bf = a["bf"]
    elif a["num_elements"] is not None:
        bf = lib.ntedit_hip_reads_bf_size(a["num_elements"], a["hashes"], a["fpr"])
    if not a["size_from_hist"] and bf == 0:
        raise Refused("The output filter would be empty (--bf 0 or --num_elements too small).")
    sketch = a["sketch_bytes"]
    if sketch == 0:
        files = (ctypes.c_char_p * len(a["reads"]))(*[f.encode() for f in a["reads"]])
        sketch = lib.ntedit_hip_reads_default_sketch(files, len(a["reads"]), 0 if a["size_from_hist"] else bf)
    return bf, sketch


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
    weights = [n * (GZIP_WEIGHT if gz else 1) for n, gz in facts]
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
    """one rank's state: the context it builds in (a Polisher's, owned by the caller), the process group, and what the
    build measured (passes, exchanges)"""

    def __init__(self, a, rank, world, pol, group, name="make_reads"):
        self.a, self.rank, self.world, self.group, self.name = a, rank, world, group, name
        self.lib, self.h = pol._lib, pol._h
        self.xbytes, self.xsec = 0, 0.0
        self.passes, self.exchanges = {}, []

    def fail(self, what):
        raise RuntimeError("%s: %s: %s" % (self.name, what, self.lib.ntedit_hip_reads_last_error(self.h).decode()))

    def run_pass(self, which, units, cmin=0):
        n = len(units)
        files = (ctypes.c_char_p * max(n, 1))(*[u.path.encode() for u in units])
        begins = (ctypes.c_uint64 * max(n, 1))(*[u.begin for u in units])
        ends = (ctypes.c_uint64 * max(n, 1))(*[u.end for u in units])
        starts = (ctypes.c_uint64 * max(n, 1))()
        nexts = (ctypes.c_uint64 * max(n, 1))()
        st = _lib.ReadsPassStats()
        if self.lib.ntedit_hip_reads_pass(self.h, which, files, begins, ends, n, self.a["batch_bytes"], cmin,
                                          ctypes.byref(st), starts, nexts) != 0:
            self.fail("pass " + PASS_NAMES[which])
        self._log_pass(which, st.bases, st.ms_wall, st.ms_gpu, "%d ranges" % n)
        return [(u.file, u.begin, starts[i], nexts[i]) for i, u in enumerate(units)]

    def store_pass(self, which, bases, batches, slot=0, cmin=0):
        """the histogram pass or pass 2 over the resident store (bases: pass 1's, which the store holds)"""
        t0 = time.perf_counter()
        rc = (self.lib.ntedit_hip_resident_histogram(self.h) if which == _lib.READS_PASS_HIST
              else self.lib.ntedit_hip_resident_insert_solid(self.h, slot, cmin))
        if rc != 0:
            self.fail("pass " + PASS_NAMES[which])
        ms = (time.perf_counter() - t0) * 1e3
        self._log_pass(which, bases, ms, ms, "%d batches of the resident store" % batches)

    def _log_pass(self, which, bases, ms, g, what):
        self.passes[PASS_NAMES[which][0]] = dict(bases=bases, ms=round(ms, 3), gpu_ms=round(g, 3))
        log_info("rank %d/%d: Pass %s: %d bases, %.1f ms, %.3f Gbases/s (GPU calls %.1f ms, %.3f Gbases/s), %s"
                 % (self.rank, self.world, PASS_NAMES[which], bases, ms, bases / ms / 1e6 if ms > 0 else 0.0, g,
                    bases / g / 1e6 if g > 0 else 0.0, what))

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


STORE_STATES = {_lib.RESIDENT_OFF: "off", _lib.RESIDENT_ON: "on", _lib.RESIDENT_OVER_CAP: "over cap",
                _lib.RESIDENT_NO_MEMORY: "no memory"}


def build_rank(pol, a, rank, world, group, slot=0, use_store=False, store_cap=RESIDENT_CAP_DEFAULT, name="make_reads"):
    """One rank's share of the reads filter build, the same for every driver: the plan, pass 1 over this rank's units
    into an adopted sketch, the cut-point check, the sketch merge, with --solid / --hist the histogram pass (rank 0
    writes --hist), pass 2 into an adopted filter in `slot` of pol's context, the filter merge.  On return every rank
    holds the whole filter there and the sketch is freed.  With use_store the reads of pass 1 stay resident in HBM
    (ntedit_hip_resident_begin, up to store_cap bytes) and the later passes read the store; a rank whose store was
    released reads its ranges again, with the same result.  ntedit_hip_reads_pass fills the PRIMARY slot, so that is
    the only slot a build can fill.
    -> (the filter tensor, which the caller keeps alive while the slot is in use, a report dict)"""
    import torch
    if slot != 0:
        raise ValueError("build_rank: pass 2 from the files fills the PRIMARY slot (0) only")
    lib = pol._lib
    bf, sketch = sizes(lib, a)
    facts = file_facts(lib, a["reads"])
    units, owner = plan(a["reads"], facts, world, split=not a["no_split"])
    mine = [u for u, o in zip(units, owner) if o == rank]
    mine.sort(key=Unit.key)
    if rank == 0:
        log_info("%d ranks, %d units (%d input files), sketch %d counters, %s" %
                 (world, len(units), len(a["reads"]), sketch,
                  "output from the k-mer histogram" if a["size_from_hist"] else "output %d bytes" % bf))
    b = Builder(a, rank, world, pol, group, name)
    rep = dict(units=len(mine), store=dict(used=False, state="not asked", batches=0, bytes=0, fallback=False))
    try:
        k, hashes = a["k"], a["hashes"]
        counters = (sketch + 7) // 8 * 8
        sk = torch.zeros(b.padded(counters), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if lib.ntedit_hip_sketch_set_device(b.h, sk.data_ptr(), counters, hashes, k) != 0:
            b.fail("sketch")
        if use_store and lib.ntedit_hip_resident_begin(b.h, store_cap) != 0:
            b.fail("resident store")
        cut = b.run_pass(_lib.READS_PASS_COUNT, mine)
        from_store, batches = False, 0
        if use_store:
            st = _lib.ResidentStats()
            if lib.ntedit_hip_resident_info(b.h, ctypes.byref(st)) != 0:
                b.fail("resident store")
            from_store, batches = st.state == _lib.RESIDENT_ON, st.batches
            rep["store"] = dict(used=from_store, state=STORE_STATES.get(st.state, str(st.state)), batches=st.batches,
                                bytes=st.bytes, fallback=not from_store)
            later = "the histogram pass and pass 2" if a["gather_hist"] else "pass 2"
            if from_store:
                log_info("rank %d/%d: Resident store: %d batches, %d bytes of HBM (3 bits per base); %s read it"
                         % (rank, world, st.batches, st.bytes, later))
            else:
                log_info("rank %d/%d: Resident store: released (%s); %s read this rank's ranges again"
                         % (rank, world, "the reads would pass its cap of %d bytes" % st.cap
                            if st.state == _lib.RESIDENT_OVER_CAP else "a device allocation failed", later))
        bases = b.passes["1"]["bases"]
        brk = check_cuts([c for part in b.all_gather_object(cut) for c in part])
        if brk is not None:
            f, b0, b1, nxt, start = brk
            raise Refused("%s: the ranges at bytes %d and %d do not meet (the first stops before byte %s, the second "
                          "starts at byte %d): this file cannot be cut into ranges (multi-line FASTQ?); run with "
                          "--no-split, which reads every file whole.  No output was written."
                          % (a["reads"][f], b0, b1, "(a failed record)" if nxt == WHOLE else nxt, start))
        b.merge(sk, _lib.MERGE_SAT_ADD)
        cmin = a["cmin"] or 0
        if a["gather_hist"]:
            if from_store:
                b.store_pass(_lib.READS_PASS_HIST, bases, batches)
            else:
                b.run_pass(_lib.READS_PASS_HIST, mine)
            occ = np.zeros(256, dtype=np.uint64)
            if lib.ntedit_hip_sketch_histogram_download(b.h, occ.ctypes.data_as(ctypes.c_void_p)) != 0:
                b.fail("histogram")
            occ = b.all_reduce_hist(occ)
            f = np.zeros(256, dtype=np.uint64)
            F0, F1 = ctypes.c_uint64(), ctypes.c_uint64()
            lib.ntedit_hip_reads_hist_summary(occ.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.byref(F0), ctypes.byref(F1))
            if rank == 0:
                log_info("k-mer histogram: F1 = %d (k-mers), F0 = %d (distinct k-mers)" % (F1.value, F0.value))
                if a["hist"]:
                    if lib.ntedit_hip_reads_write_hist(a["hist"].encode(), f.ctypes.data_as(ctypes.c_void_p), F0.value,
                                                       F1.value) != 0:
                        raise RuntimeError("cannot write " + a["hist"])
                    log_info("Histogram written to " + a["hist"])
            if a["solid"]:
                c = ctypes.c_uint32()
                if lib.ntedit_hip_reads_solid_cutoff(f.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c)) != 0:
                    raise Refused("--solid: the k-mer histogram has no valley after the error peak (no c with f[c+1] "
                                  "> f[c]); pass -c")
                cmin = c.value
                if rank == 0:
                    log_info("--solid: minimum k-mer count %d" % cmin)
            if a["size_from_hist"]:
                ne = int(f[cmin:].sum())
                bf = lib.ntedit_hip_reads_bf_size(ne, hashes, a["fpr"])
                if rank == 0:
                    log_info("Sized from the k-mer histogram: --num_elements %d (k-mers at %d or above), %d bytes"
                             % (ne, cmin, bf))
                if bf == 0:
                    raise Refused("The output filter would be empty (no k-mer at the minimum count or above).")
        nbytes = (bf + 7) // 8 * 8
        out = torch.zeros(b.padded(nbytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pol.set_filter_device(out.data_ptr(), nbytes, hashes, k, slot=slot, counting=a["counts"])
        if from_store:
            b.store_pass(_lib.READS_PASS_SOLID, bases, batches, slot, cmin)
        else:
            b.run_pass(_lib.READS_PASS_SOLID, mine, cmin)
        lib.ntedit_hip_sketch_free(b.h)  # (the store with it)
        del sk
        b.merge(out, _lib.MERGE_MAX if a["counts"] else _lib.MERGE_OR)
    finally:
        lib.ntedit_hip_sketch_free(b.h)
    rep.update(cmin=cmin, filter_bytes=nbytes, passes=b.passes, exchanges=b.exchanges, exchange_bytes=b.xbytes,
               exchange_ms=round(b.xsec * 1e3, 3))
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
        if group is not None:
            import torch.distributed as dist
            dist.barrier()
        del out
    finally:
        pol.close()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        a = parse(argv)
        if a["help"]:
            sys.stderr.write(USAGE)
            return 0
        # torch's HIP runtime first, as in ntedit_amd.run: the library then binds to the runtime torch brought in
        # (loaded the other way round, the library's context cannot see the device in a torch.distributed.run child)
        import torch  # noqa: F401  (no device is touched here)
        lib = _lib.load()
        sizes(lib, a)  # (the empty-output refusal comes before any device)
    except Refused as e:
        sys.stderr.write("%s\n%s" % (e, USAGE))
        return 1
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        sys.stderr.write("make_reads: error: no HIP device (this build has no CPU path)\n")
        return 1
    rank, world, local = ndist.env_rank()
    if (a["backend"] or "nccl") != "nccl":
        local = local % torch.cuda.device_count()  # (gloo rehearsal: ranks share the GPUs there are)
    torch.cuda.set_device(local)
    group = None
    if world > 1 or "RANK" in os.environ or a["backend"]:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group(backend=a["backend"] or "nccl", rank=rank, world_size=world)
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
