"""python -m ntedit_amd.run -f draft.fa[.gz] -r solid.bf [-e repeat.bf] [-b prefix] [ntedit flags]
python -m ntedit_amd.run -f draft.fa[.gz] --reads FILE... -k K (--cutoff C | --solid) [reads flags] [ntedit flags]

The multi-GPU driver of the hot path: one process per GPU, launched with

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        -m ntedit_amd.run -f draft.fa -r solid.bf -b out

(or plainly, without a launcher, on one GPU).  Rank 0 reads the Bloom filter file(s) once and ships the bit
arrays to every GPU with ONE RCCL broadcast each (dist.load_and_broadcast_filter); every rank maps the draft and
reads its INDEX (headers, lengths: Draft / ntedit_hip_fasta_open), computes the same partition of the contigs by bases --
contigs larger than a GPU's share are cut at event-free boundaries (dist.plan_pieces) --, reads the bases of ITS pieces
straight into its page-locked batch, polishes them through the C ABI (ntedit_amd.Polisher = libntedit_hip.so), writes
<prefix>.shard<r>_*, and -- after the per-piece byte counts have been all-gathered, a few KB -- copies its pieces to
their offsets in <prefix>_edited.fa / _changes.tsv / _variants.vcf itself (dist.gather_parallel): no rank holds the
draft, no rank reads another rank's output.  Byte-identical to the single-GPU `ntedit` binary's output (and to the
reference at -t 1).

With --reads instead of -r (the reads options of `ntedit --reads`, with their meaning and refusals, and --no-split of
ntedit_amd.make_reads) every rank builds its share of the reads filter in HBM, the reads it parsed in pass 1 kept
resident there for the later passes, into the context that then polishes (make_reads.build_rank); the merges leave the
whole filter on every rank: no filter file, no broadcast.  With --reject_cutoff the -e filter is built by the same pass 2
and merged the same way into every rank's SECONDARY slot.  The outputs are those of `ntedit --reads` with the same flags.

What the reference does instead: readAndCorrect's OpenMP loop (ntedit.cpp:2213-2252), contigs handed to threads one
at a time, output in completion order."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

from . import _lib, dist as ndist, make_reads
from .make_reads import Refused, log_info
from .polisher import Polisher, default_params, pack_batch


def read_fasta_fast(path, min_len=0, threads=0):
    """[(header, sequence bytes)] of the records with >= min_len bases, read by the SAME code the `ntedit` binary
    ingests with (ntedit_hip_fasta_load: kseq's record semantics, lib/kseq.h:176-215 as used at
    ntedit.cpp:2223-2230 -- gzip / BGZF told apart by their magic bytes, FASTQ, CR line ends, NUL bytes, text in
    front of the first header).  Raises on an unreadable, corrupt or truncated file instead of returning a shorter
    draft."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    rc = lib.ntedit_hip_fasta_load(os.fsencode(path), int(min_len), int(threads), ctypes.byref(h), err, len(err))
    if rc != 0:
        raise _lib.NtEditHipError("%s (%d)" % (err.value.decode(errors="replace") or "cannot read the draft", rc))
    try:
        nbytes = ctypes.c_uint64()
        base = lib.ntedit_hip_fasta_blob(h, ctypes.byref(nbytes))
        recs = []
        hp, hl, off, ln = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        for i in range(lib.ntedit_hip_fasta_count(h)):
            lib.ntedit_hip_fasta_record(h, i, ctypes.byref(hp), ctypes.byref(hl), ctypes.byref(off), ctypes.byref(ln))
            recs.append((ctypes.string_at(hp.value, hl.value) if hl.value else b"",
                         ctypes.string_at(base + off.value, ln.value) if ln.value else b""))
        return recs
    finally:
        lib.ntedit_hip_fasta_free(h)


class LazySlice:
    """bases [start, end) of a record of a Draft: read when somebody needs them (straight into a page-locked batch
    buffer with read_into(), or as bytes)"""
    __slots__ = ("draft", "rec", "start", "end")

    def __init__(self, draft, rec, start, end):
        self.draft, self.rec, self.start, self.end = draft, rec, int(start), int(end)

    def __len__(self):
        return self.end - self.start

    def read_into(self, address):
        self.draft.read_into(self.rec, self.start, self.end, address)

    def __bytes__(self):
        return self.draft.read(self.rec, self.start, self.end)


class LazySeq:
    """one record's sequence, sliceable: seq[a:b] reads those bases (the 64 KB windows cuts are looked for in),
    seq.lazy(a, b) only describes them"""
    __slots__ = ("draft", "rec", "n")

    def __init__(self, draft, rec, n):
        self.draft, self.rec, self.n = draft, rec, int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("LazySeq takes slices")
        a, b, step = key.indices(self.n)
        if step != 1:
            raise ValueError("LazySeq slices are contiguous")
        return self.draft.read(self.rec, a, max(a, b))

    def lazy(self, a, b):
        return LazySlice(self.draft, self.rec, a, b)


class Draft:
    """The draft as a multi-GPU rank needs it: the INDEX of the file -- headers and lengths, found by
    the library's mapped multi-threaded reader, ntedit_hip_fasta_open -- and its bases on demand.  Every rank plans the same
    partition from the lengths and then reads ITS OWN pieces (and the windows of its cuts) out of the mapped file;
    nobody holds the draft.  records() is the [(header, sequence)] list dist.run_sharded takes, with LazySeq
    sequences.  Inputs the mapped reader does not take (single-stream gzip, FASTQ, ...) are loaded whole by the
    library; nothing changes for the caller."""

    def __init__(self, path, min_len=0, threads=0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = self._lib.ntedit_hip_fasta_open(os.fsencode(path), int(min_len), int(threads), ctypes.byref(self._h), err, len(err))
        if rc != 0:
            raise _lib.NtEditHipError("%s (%d)" % (err.value.decode(errors="replace") or "cannot read the draft", rc))
        self.headers, self.lens = [], []
        hp, hl, off, ln = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        for i in range(self._lib.ntedit_hip_fasta_count(self._h)):
            self._lib.ntedit_hip_fasta_record(self._h, i, ctypes.byref(hp), ctypes.byref(hl), ctypes.byref(off), ctypes.byref(ln))
            self.headers.append(ctypes.string_at(hp.value, hl.value) if hl.value else b"")
            self.lens.append(int(ln.value))
        self.bytes_read = 0

    def records(self):
        return [(h, LazySeq(self, i, n)) for i, (h, n) in enumerate(zip(self.headers, self.lens))]

    def read_into(self, rec, start, end, address):
        if self._lib.ntedit_hip_fasta_read(self._h, rec, int(start), int(end - start), ctypes.c_void_p(address)) != 0:
            raise ValueError("draft record %d: bases [%d, %d) are out of range" % (rec, start, end))
        self.bytes_read += end - start

    def read(self, rec, start, end):
        buf = ctypes.create_string_buffer(max(1, end - start))
        self.read_into(rec, start, end, ctypes.addressof(buf))
        return buf.raw[:end - start]

    def close(self):
        if self._h:
            self._lib.ntedit_hip_fasta_free(self._h)
            self._h = ctypes.c_void_p()


class HipBackend:
    """dist.run_sharded's compute backend on the real thing: the HIP library through the C ABI"""

    def __init__(self, polisher, annot=None):
        self.pol = polisher
        self.annot = annot
        self.ms_gpu = 0.0
        self.bases = 0
        self.n_rerun = 0

    def screen(self, blob):
        return self.pol.screen(blob)

    def _pinned_batch(self, entries):
        """the batch layout of pack_batch, written straight into page-locked memory (ntedit_hip_host_alloc): the batch then
        crosses PCIe asynchronously, in pieces, under the screening -- from ordinary memory the runtime stages it through
        its own buffers first (a rank's 375 Mbp: ~35 ms against ~10)"""
        import numpy as np
        total = sum(len(e[1]) + 1 for e in entries)
        lib = self.pol._lib
        if total > getattr(self, "_pin_cap", 0):
            if getattr(self, "_pin_ptr", None):
                lib.ntedit_hip_host_free(ctypes.c_void_p(self._pin_ptr))
            self._pin_ptr = lib.ntedit_hip_host_alloc(total + total // 8 + 4096)
            self._pin_cap = total + total // 8 + 4096 if self._pin_ptr else 0
        if not getattr(self, "_pin_ptr", None):
            return None
        buf = np.ctypeslib.as_array((ctypes.c_uint8 * total).from_address(self._pin_ptr))
        offs, lens, pos = [], [], 0
        for _, seq, _ in entries:
            n = len(seq)
            if hasattr(seq, "read_into"):
                seq.read_into(self._pin_ptr + pos)  # (a piece of a Draft: mapped file -> page-locked batch, one copy)
            else:
                ctypes.memmove(self._pin_ptr + pos, seq, n)
            buf[pos + n] = 10
            offs.append(pos)
            lens.append(n)
            pos += n + 1
        return buf, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32)

    def close(self):
        if getattr(self, "_pin_ptr", None):
            self.pol._lib.ntedit_hip_host_free(ctypes.c_void_p(self._pin_ptr))
            self._pin_ptr, self._pin_cap = None, 0

    def polish(self, entries, fa, tsv, vcf, append):
        names = [e[0] for e in entries]
        pinned = self._pinned_batch(entries)
        if pinned is not None:
            blob, offs, lens = pinned
        else:
            blob, offs, lens, _ = pack_batch([(e[0], bytes(e[1])) for e in entries], 0)
        res = self.pol.polish_batch(blob, offs, lens)
        # the renderer's own predicate, asked before anything is written (a refused entry would leave the shard
        # files half-written): a cut that is not event-free is polished again joined with its successor
        ok = res.cuts_ok(lens, [e[2] for e in entries])
        segs, bad = [], []
        for i, (_, _, (off, halo, flags)) in enumerate(entries):
            if not ok[i]:
                bad.append(i)
                flags |= ndist.SEG_SKIP
            segs.append((off, halo, flags))
        sizes = res.write(blob, offs, lens, names, fa, tsv, append=append, vcf_path=vcf, annot=self.annot,
                          segments=segs, want_sizes=True)
        st = res.stats()
        self.ms_gpu += st.ms_total
        self.bases += int(lens.sum())
        self.n_rerun += len(bad)
        res.free()
        return bad, sizes


# the reads options of `ntedit --reads` (+ make_reads' --no-split): (flag, dest), in the order a refusal names them
READS_OPTIONS = [("--cutoff", "cutoff"), ("--solid", "solid"), ("--counts", "counts"), ("--hashes", "hashes"),
                 ("--fpr", "fpr"), ("--bf", "bf_bytes"), ("--num_elements", "num_elements"),
                 ("--sketch_bytes", "sketch_bytes"), ("--hist", "hist"), ("--save_bf", "save_bf"),
                 ("--batch_bytes", "batch_bytes"), ("--resident_cap", "resident_cap"), ("--no-split", "no_split"),
                 ("--gpu_parse", "gpu_parse"), ("--reject_cutoff", "reject_cutoff"), ("--reject_bf", "reject_bf"),
                 ("--reject_num_elements", "reject_num_elements"), ("--save_reject_bf", "save_reject_bf"),
                 ("--min_qual", "min_qual"), ("--min_read_len", "min_read_len"), ("--min_mean_qual", "min_mean_qual"),
                 ("--min_rq", "min_rq")]


def parse(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    reads_mode = "--reads" in argv
    ap = argparse.ArgumentParser(prog="python -m ntedit_amd.run", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-f", dest="draft", required=True)
    ap.add_argument("-r", dest="bf", required=not reads_mode)
    ap.add_argument("-e", dest="bfrep")
    ap.add_argument("-b", dest="prefix")
    ap.add_argument("-l", dest="annot")
    ap.add_argument("-z", dest="min_contig_len", type=int, default=100)
    ap.add_argument("-i", dest="max_insertions", type=int, default=5)
    ap.add_argument("-d", dest="max_deletions", type=int, default=5)
    ap.add_argument("-x", dest="missing_threshold", type=float, default=5.0)
    ap.add_argument("-y", dest="edit_threshold", type=float, default=9.0)
    ap.add_argument("-X", dest="missing_ratio", type=float)
    ap.add_argument("-Y", dest="edit_ratio", type=float)
    ap.add_argument("-j", dest="jump", type=int, default=3)
    ap.add_argument("-m", dest="mode", type=int, default=0)
    ap.add_argument("-s", dest="snv", type=int, default=0)
    ap.add_argument("-a", dest="mask", type=int, default=0)
    ap.add_argument("-p", dest="min_threshold", type=int, default=1)
    ap.add_argument("-q", dest="max_threshold", type=int, default=255)
    ap.add_argument("-t", dest="threads", type=int, default=0, help="host threads rendering the output")
    ap.add_argument("-k", dest="k_ignored", type=str if reads_mode else int,
                    help="ignored: k comes from the filter (with --reads: the k-mer size, 12 to 200, required)")
    ap.add_argument("--seg-bases", type=int, default=None,
                    help="cut contigs longer than 1.5x this (default: an eighth of a GPU's share, 1-32 Mbp)")
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--qv", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    ap.add_argument("--completeness", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    ap.add_argument("--bgzip", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    ap.add_argument("--bed", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    ap.add_argument("--spectrum", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    ap.add_argument("--cn", action="store_true", help=argparse.SUPPRESS)  # (refused: see parse())
    g = ap.add_argument_group("polishing straight from reads (--reads replaces -r; the options of `ntedit --reads`, "
                              "the same filter; every rank builds its share and holds the whole filter)")
    g.add_argument("--reads", nargs="*", metavar="FILE", help="input reads, FASTA or FASTQ, plain or gzip")
    g.add_argument("--cutoff", metavar="C", help="minimum k-mer count of the filter, 1 to 255")
    g.add_argument("--solid", action="store_true", help="take the minimum count from the k-mer histogram instead")
    g.add_argument("--counts", action="store_true", help="build a counting filter (enables -p / -q)")
    g.add_argument("--hashes", metavar="H", help="number of hash functions, 1 to 8 [3]")
    g.add_argument("--fpr", metavar="F", help="false positive rate of the filter (with --num_elements) [0.01]")
    g.add_argument("--bf", dest="bf_bytes", metavar="BYTES", help="filter size in bytes")
    g.add_argument("--num_elements", metavar="N", help="approximate number of solid k-mers")
    g.add_argument("--sketch_bytes", metavar="S", help="counters of the count-min sketch")
    g.add_argument("--hist", metavar="FILE", help="write the k-mer histogram (rank 0)")
    g.add_argument("--save_bf", metavar="FILE", help="write the filter that was built (rank 0); the _r part of the "
                                                     "default prefix [reads_k<K>.bf, not written]")
    g.add_argument("--reject_cutoff", metavar="R", help="also build the -e filter (k-mers to reject) from the same pass over "
                                                        "the reads: the k-mers seen at least R times, 2 to 255 and above "
                                                        "the cutoff (replaces -e; not with --counts)")
    g.add_argument("--reject_bf", metavar="BYTES", help="reject filter size in bytes")
    g.add_argument("--reject_num_elements", metavar="N", help="approximate number of k-mers in the reject filter")
    g.add_argument("--save_reject_bf", metavar="FILE", help="write the reject filter that was built (rank 0) "
                                                            "[reads_k<K>_reject.bf, not written]")
    g.add_argument("--no-split", dest="no_split", action="store_true",
                   help="read every input file whole (by one rank); gzip files always are")
    g.add_argument("--gpu_parse", action="store_true",
                   help="parse plain and bgzip-compressed (BGZF) read files on the GPU: the host ships the file's bytes, BGZF still "
                        "compressed; same outputs (single-stream gzip stays with the host parser).  BAM reads, unaligned or "
                        "aligned, need it; a BAM is read whole by one rank, as gzip files are")
    g.add_argument("--min_qual", metavar="Q",
                   help="minimum base quality, 1 to 93 (Phred+33; Phred+64 is not built): a base whose quality is below Q "
                        "enters the filter build as N, on every rank alike (FASTQ: a quality character below 33 + Q; BAM: a "
                        "quality byte below Q; records without qualities pass as they are)")
    g.add_argument("--min_read_len", metavar="L",
                   help="minimum read length, 1 to 2147483647: the shortest read kept is the larger of L and k")
    g.add_argument("--min_mean_qual", metavar="Q",
                   help="minimum mean read quality, 1 to 60: the Phred value of the read's mean error probability (not the mean "
                        "of the Phred values), over the qualities as stored; reads without qualities pass")
    g.add_argument("--min_rq", metavar="R",
                   help="minimum read accuracy, above 0 and at most 1: a BAM read whose rq tag (type f) is below R is dropped; "
                        "reads without the tag pass, so every FASTA and FASTQ read does")
    g.add_argument("--batch_bytes", help=argparse.SUPPRESS)  # (tests: many small read batches)
    g.add_argument("--resident_cap", help=argparse.SUPPRESS)  # (tests: the resident store's cap; 0: off)
    args = ap.parse_args(argv)
    if args.completeness:
        raise Refused("--completeness: the marks of several GPUs would need a merge of their own, which is out of scope; "
                      "run `ntedit --qv --completeness` on one GPU")
    if args.qv:
        raise Refused("--qv: this driver cuts large contigs into segments, and per-contig rows over cut contigs are out of "
                      "scope; run `ntedit --qv` on one GPU")
    if reads_mode and args.k_ignored is not None and "," in args.k_ignored:
        raise Refused("-k %s: a list of k (a cascade of polishing rounds) is `ntedit --reads` on one GPU; this driver "
                      "polishes at one k" % args.k_ignored)
    args.reads_args = reads_args(args) if reads_mode else None
    if not reads_mode:
        for flag, dest in READS_OPTIONS:
            if getattr(args, dest) not in (None, False):
                raise Refused(flag + ": only with --reads")
    if args.bgzip:  # (behind every older refusal)
        raise Refused("--bgzip: the gather that merges the ranks' pieces by their byte index knows plain text only; run "
                      "`ntedit --bgzip` on one GPU")
    if args.bed:
        raise Refused("--bed: the tracks of cut contigs on several GPUs would need a merge of their own, which is out of "
                      "scope; run `ntedit --qv --bed` on one GPU")
    if args.spectrum:
        raise Refused("--spectrum: the spectra and depth rows of cut contigs on several GPUs would need a merge of their own, "
                      "which is out of scope; run `ntedit --spectrum` on one GPU")
    if args.cn:
        raise Refused("--cn: copy numbers belong to the whole draft, and the rows of cut contigs on several GPUs would need a "
                      "merge of their own, which is out of scope; run `ntedit --spectrum --cn` on one GPU")
    return args


def reads_args(args):
    """the refusals of `ntedit --reads` (host/main.cpp), in its order, before any device or file is touched: what only a
    front end has here, the rules of the options in the library; -> the argument dict of make_reads.build_rank"""
    if args.bf is not None:
        raise Refused("--reads and -r: give one of them (--reads builds the filter that -r would load)")
    if not args.reads:
        raise Refused("--reads: 1 or more files expected")
    if args.reject_cutoff is not None and args.bfrep is not None:
        raise Refused("--reject_cutoff and -e: give one of them (--reject_cutoff builds the filter that -e would load)")
    given = {name: getattr(args, dest) for name, dest in
             (("k", "k_ignored"), ("cutoff", "cutoff"), ("hashes", "hashes"), ("fpr", "fpr"), ("bf", "bf_bytes"),
              ("num_elements", "num_elements"), ("sketch_bytes", "sketch_bytes"), ("batch_bytes", "batch_bytes"),
              ("store_cap", "resident_cap"), ("reject_cutoff", "reject_cutoff"), ("reject_bf", "reject_bf"),
              ("reject_num_elements", "reject_num_elements"), ("min_qual", "min_qual"), ("min_read_len", "min_read_len"),
              ("min_mean_qual", "min_mean_qual"), ("min_rq", "min_rq")) if getattr(args, dest) is not None}
    a = make_reads.check_options(_lib.READS_DIALECT_POLISHER, given, True, args.reads, args.solid, args.hist or "",
                                 args.gpu_parse, args.counts, args.save_reject_bf is not None)
    a.update(counts=args.counts, no_split=args.no_split)
    for path in [args.draft] + a["reads"]:
        try:
            open(path, "rb").close()
        except OSError as e:
            raise Refused("`%s': %s" % (path, e.strerror)) from None
    return a


def build_from_reads(pol, args, rank, world):
    """--reads: this rank's share of the reads filter, built into the PRIMARY slot of pol's context with the reads kept
    resident in HBM (make_reads.build_rank); every rank then holds the whole filter: no file, no broadcast.  Rank 0
    writes --save_bf.  With --reject_cutoff the merged reject filter is left in every rank's SECONDARY slot the same way
    (rank 0 writes --save_reject_bf).  The sketch and the store are freed, and torch's cache of them released, before the polish
    reserves its buffers.  -> the report of the build, or None after a refusal (on every rank alike)"""
    import torch
    import torch.distributed as dist
    a = args.reads_args
    group = dist.group.WORLD if dist.is_initialized() else None
    try:
        buf, rep = make_reads.build_rank(pol, a, rank, world, group, slot=0, use_store=True, store_cap=a["store_cap"],
                                         name="run")
    except Refused as e:
        sys.stderr.write("python -m ntedit_amd.run: error: %s\n" % e)
        return None
    ndist._keep(pol, 0, buf)
    torch.cuda.empty_cache()
    if rank == 0:
        log_info("rank 0: filter (%d bytes) built from the reads in HBM, minimum count %d; exchanges %d bytes sent in "
                 "%.1f ms" % (rep["filter_bytes"], rep["cmin"], rep["exchange_bytes"], rep["exchange_ms"]))
        if args.save_bf:
            pol.filter_save_file(args.save_bf, 0)
            log_info("Bloom filter saved to " + args.save_bf)
        if "reject" in rep:
            log_info("rank 0: reject filter (%d bytes) built from the same pass, reject count %d"
                     % (rep["reject"]["filter_bytes"], rep["reject"]["cutoff"]))
            if args.save_reject_bf:
                pol.filter_save_file(args.save_reject_bf, 1)
                log_info("Reject Bloom filter saved to " + args.save_reject_bf)
    return rep


def main(argv=None):
    import ctypes
    import torch
    import torch.distributed as dist
    try:
        args = parse(argv)
    except Refused as e:
        sys.stderr.write("python -m ntedit_amd.run: error: %s\n" % e)
        return 1
    rank, world, local = ndist.env_rank()
    if not torch.cuda.is_available():
        sys.stderr.write("ntEdit v2.1.1: error: no HIP device (this build has no CPU path)\n")
        return 1
    if (args.backend or "nccl") != "nccl":
        # (rehearsal: `--backend gloo` lets N ranks share the GPUs that are there -- RCCL refuses two ranks on one device --
        # so the N > 1 path of this driver can be run on a one-GPU box; its timings then say nothing about N GPUs)
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1 or args.backend:
        # (a one-rank group still exercises the collective path: the round-end GPU test does this)
        ndist.init_process_group(args.backend or "nccl", port=29511 if world > 1 else 29513, single=True)
    pol = Polisher(local)
    pol._lib.ntedit_hip_bind_near_device(local)  # host threads and buffers on the socket this rank's GPU hangs off
    t0 = time.perf_counter()
    reads = None
    if args.reads_args is not None:
        reads = build_from_reads(pol, args, rank, world)
        if reads is None:
            pol.close()
            if dist.is_initialized():
                dist.destroy_process_group()
            return 1
    else:
        ndist.load_and_broadcast_filter(pol, args.bf, 0, 0)
    if args.bfrep:
        ndist.load_and_broadcast_filter(pol, args.bfrep, 0, 1)
    t_filter = time.perf_counter() - t0
    k, h, nbytes, counting = pol.filter_info(0)
    p = default_params(min_contig_len=args.min_contig_len, max_insertions=args.max_insertions,
                       max_deletions=args.max_deletions, missing_threshold=args.missing_threshold,
                       edit_threshold=args.edit_threshold, jump=args.jump, mode=args.mode, snv=args.snv,
                       mask=args.mask, min_threshold=args.min_threshold if counting else 1,
                       max_threshold=args.max_threshold)
    if args.missing_ratio is not None or args.edit_ratio is not None:
        p.use_ratio = 1
        if args.missing_ratio is not None:
            p.missing_ratio = args.missing_ratio
        if args.edit_ratio is not None:
            p.edit_ratio = args.edit_ratio
    warn = ctypes.create_string_buffer(1024)
    pol._lib.ntedit_hip_params_clamp(ctypes.byref(p), warn, 1024)  # ntedit.cpp:2478-2493
    if warn.value and rank == 0:
        sys.stderr.write(warn.value.decode())
    pol.set_params(p)
    if args.threads:
        pol._lib.ntedit_hip_set_host_threads(args.threads)
    prefix = args.prefix
    if not prefix:  # ntedit.cpp:2496-2502
        # (with --reads the _r part is what `ntedit --reads` puts there: the --save_bf name or reads_k<K>.bf)
        bf_name = args.bf if reads is None else (args.save_bf or "reads_k%d.bf" % k)
        prefix = "%s_k%d_z%d_r%s_i%d_d%d_m%d" % (os.path.basename(args.draft), k, p.min_contig_len,
                                                  os.path.basename(bf_name), p.max_insertions, p.max_deletions, p.mode)
    annot = ctypes.c_void_p()
    if args.annot:
        if pol._lib.ntedit_hip_annot_load(args.annot.encode(), ctypes.byref(annot)):
            sys.stderr.write("Unable to open file\n")
            annot = ctypes.c_void_p()

    # the draft's index (headers, lengths); a rank reads the bases of its own pieces only (Draft)
    t0 = time.perf_counter()
    draft = Draft(args.draft)
    records = draft.records()
    t_read = time.perf_counter() - t0

    # start-up, like the filter load: this rank's buffers for its share of the draft + one internal warm-up batch, so that
    # the one and only polish call of a rank costs what a warm one does (ntedit_hip_reserve)
    t0 = time.perf_counter()
    total = sum(len(r[1]) for r in records)
    pol.reserve(int(total / max(1, world) * 1.15) + (1 << 20), 2 * len(records) + 64)
    t_reserve = time.perf_counter() - t0

    def write_headers(pre):
        open(pre + "_edited.fa", "wb").close()
        pol.write_tsv_header(pre + "_changes.tsv")
        pol._lib.ntedit_hip_write_vcf_header((pre + "_variants.vcf").encode(), args.draft.encode())

    backend = HipBackend(pol, annot if annot.value else None)
    halo = ndist.halo_bases(k, 0 if p.snv else p.max_insertions, 0 if p.snv else p.max_deletions)
    barrier = dist.barrier if (dist.is_initialized() and world > 1) else None

    def all_gather(obj):
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out
    t0 = time.perf_counter()
    mine = ndist.run_sharded(records, backend, prefix, p.min_contig_len, rank, world, k, halo, write_headers,
                             barrier=barrier, seg_bases=args.seg_bases,
                             all_gather=all_gather if barrier else None)
    if barrier:
        barrier()
    t_run = time.perf_counter() - t0
    if args.report:
        n_seg = sum(1 for q in mine if q.n_seg > 1)
        sys.stdout.write('{"rank": %d, "world": %d, "pieces": %d, "segments": %d, "bases": %d, "reruns": %d, '
                         '"gpu_ms": %.3f, "filter_s": %.3f, "index_s": %.3f, "draft_bases_total": %d, "draft_bytes_read": %d, '
                         '"reserve_s": %.3f, "run_s": %.3f, "phases_s": %s%s}\n' %
                         (rank, world, len(mine), n_seg, backend.bases, backend.n_rerun, backend.ms_gpu, t_filter,
                          t_read, total, draft.bytes_read, t_reserve, t_run, json.dumps(ndist.LAST_PHASES),
                          "" if reads is None else ', "reads": ' + json.dumps(reads)))
        sys.stdout.flush()
    if annot.value:
        pol._lib.ntedit_hip_annot_free(annot)
    backend.close()
    draft.close()
    pol.close()
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
