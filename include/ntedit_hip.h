/*
 * ntedit_hip.h -- C ABI of the MI355X-native ntEdit hot path.
 *
 * The reference has no plugin/FFI seam; its hot path is one C++ call,
 *     kmerizeAndCorrect(hdr, seq, len, bloom, bloomrep, dfout, rfout, vfout, clinvar)
 * (ntedit.cpp:1747-1757) made per contig from readAndCorrect's OpenMP loop
 * (ntedit.cpp:2242-2245), with its parameters in the opt:: globals
 * (ntedit.cpp:99-133).  This header is the boundary a maintainer would bind
 * in its place: plain C, plain pointers and sizes, no C++/torch types.
 * INTEGRATION.md shows the reference-side stub.
 *
 * All functions return 0 on success or a negative NTEDIT_E_* code;
 * ntedit_hip_last_error() gives a message.  The host maps a failure to the
 * reference's convention (`ntEdit: error: ...` on stderr, exit(EXIT_FAILURE),
 * ntedit.cpp:476-483,2442-2445).  Nothing here falls back to the CPU: without
 * a HIP device every compute entry point fails with NTEDIT_E_DEVICE.
 */
#ifndef NTEDIT_HIP_H
#define NTEDIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTEDIT_OK 0
#define NTEDIT_E_ARG (-1)      /* bad argument / unsupported option        */
#define NTEDIT_E_DEVICE (-2)   /* HIP runtime error or no device           */
#define NTEDIT_E_NOFILTER (-3) /* primary Bloom filter not set             */
#define NTEDIT_E_OVERFLOW (-4) /* internal capacity exceeded after retries */
#define NTEDIT_E_IO (-5)       /* file could not be read / written         */
#define NTEDIT_E_UNSUPPORTED (-6) /* operation not available (e.g. GPU build of a counting filter) */
#define NTEDIT_E_SEGMENT (-7)  /* a contig segment's cut is not event-free (see ntedit_hip_segment)      */
#define NTEDIT_E_INTERNAL (-8) /* an invariant of the library does not hold (the renderer: an event reached across the margin a
                                  contig's parts are cut with); the output files are incomplete -- a bug to report, not an I/O error */

#define NTEDIT_FILTER_PRIMARY 0   /* -r  (ntedit.cpp:2438) */
#define NTEDIT_FILTER_SECONDARY 1 /* -e  (ntedit.cpp:2570) */

typedef struct ntedit_hip_ctx ntedit_hip_ctx;
typedef struct ntedit_hip_result ntedit_hip_result;
typedef struct ntedit_hip_annot ntedit_hip_annot; /* -l annotation map, see ntedit_hip_annot_load() */

/* The opt:: parameter block (ntedit.cpp:99-133).  k and h are taken from the
 * primary filter (ntedit.cpp:2439,2448), not from -k. */
typedef struct ntedit_hip_params
{
	uint32_t min_contig_len;   /* -z (host-side drop, ntedit.cpp:2242) */
	uint32_t max_insertions;   /* -i */
	uint32_t max_deletions;    /* -d */
	float edit_threshold;      /* -y */
	float missing_threshold;   /* -x */
	float edit_ratio;          /* -Y */
	float missing_ratio;       /* -X */
	int32_t use_ratio;         /* set when -X or -Y was given */
	uint32_t jump;             /* -j */
	int32_t mode;              /* -m */
	int32_t snv;               /* -s */
	int32_t mask;              /* -a */
	uint32_t min_threshold;    /* -p (counting filters only; forced to 1 for plain filters) */
	uint32_t max_threshold;    /* -q (counting filters only) */
	/* tuning, not part of the reference surface (0 = default) */
	uint32_t start_grid;       /* extra event start every N positions in an absent run (power of 2) */
	uint32_t node_window;      /* rope nodes kept live per event thread */
	uint32_t screen_mode;      /* 0 auto, 1 direct gather kernel, 2 L2-partitioned (binned) pipeline */
	uint32_t event_budget;     /* positions a speculative event may walk before it is parked and, if it
	                              turns out to be applied, re-run to completion (0 = default 2048) */
} ntedit_hip_params;

/* defaults of ntedit.cpp:99-133 */
void ntedit_hip_params_default(ntedit_hip_params* p);
/* main()'s clamping after the filter is known (ntedit.cpp:2411-2413,2478-2493).
 * warn (may be NULL, cap bytes) receives the reference's warning texts. */
void ntedit_hip_params_clamp(ntedit_hip_params* p, char* warn, size_t cap);

int ntedit_hip_create(int device, ntedit_hip_ctx** out);
void ntedit_hip_destroy(ntedit_hip_ctx* ctx);
const char* ntedit_hip_last_error(const ntedit_hip_ctx* ctx);

/* ---- Bloom filters (replaces BFWrapper, ntedit.cpp:350-401) -------------
 * bits: the btllib bit array (LSB-first within a byte), nbytes a multiple of 8.
 * set_filter copies host memory to HBM; set_filter_device adopts a device
 * pointer owned by the caller (e.g. a buffer that was just RCCL-broadcast). */
int ntedit_hip_set_filter(
    ntedit_hip_ctx* ctx,
    int slot,
    const uint8_t* bits,
    uint64_t nbytes,
    uint32_t hash_num,
    uint32_t k,
    int counting);
int ntedit_hip_set_filter_device(
    ntedit_hip_ctx* ctx,
    int slot,
    void* device_bits,
    uint64_t nbytes,
    uint32_t hash_num,
    uint32_t k,
    int counting);
/* reads a btllib-format .bf file (header + raw array) straight into HBM */
int ntedit_hip_load_filter_file(ntedit_hip_ctx* ctx, int slot, const char* path);
/* filter geometry as loaded: k, hash_num, bytes, counting */
int ntedit_hip_filter_info(
    const ntedit_hip_ctx* ctx,
    int slot,
    uint32_t* k,
    uint32_t* hash_num,
    uint64_t* nbytes,
    int* counting);
void* ntedit_hip_filter_device_ptr(const ntedit_hip_ctx* ctx, int slot);

/* Build side (fixtures / benchmarks; mirrors src/ntedit_make_genome_bf.cpp:143-157):
 * allocate a zeroed filter in HBM, insert every all-ACGT k-mer of a sequence,
 * download / save it. */
int ntedit_hip_filter_alloc(ntedit_hip_ctx* ctx, int slot, uint64_t nbytes, uint32_t hash_num, uint32_t k);
int ntedit_hip_filter_insert(ntedit_hip_ctx* ctx, int slot, const char* bases, uint64_t n, int on_device);
/* occupied = set bits (plain) / non-zero counters (counting), slots = bits / counters:
 * btllib's get_fpr() is (occupied / slots)^hash_num (printed at ntedit_make_genome_bf.cpp:159) */
int ntedit_hip_filter_occupancy(ntedit_hip_ctx* ctx, int slot, uint64_t* occupied, uint64_t* slots);
int ntedit_hip_filter_download(const ntedit_hip_ctx* ctx, int slot, uint8_t* bits);
int ntedit_hip_filter_save_file(const ntedit_hip_ctx* ctx, int slot, const char* path);

int ntedit_hip_set_params(ntedit_hip_ctx* ctx, const ntedit_hip_params* p);

/* Reads k-mer filter build (ntedit-make-reads-bf; the reference runs ntHits / ntStat on the CPU for this step, and this is
 * neither of them).  k-mers, hashes and slots are those of ntedit_hip_filter_insert: runs of k bytes of ACGTacgt, no
 * k-mer across a byte of anything else, canonical ntHash, h hashes.
 *   pass 1  ntedit_hip_sketch_count: a count-min sketch of `counters` 8-bit counters (btllib's counting-filter layout,
 *           counter hv_i % counters): every k-mer occurrence adds 1 to ALL h of its counters, saturating at 255.
 *           (Plain count-min, not btllib's conservative update: each counter ends at min(255, occurrences that hit
 *           it), whatever the order of the atomics.)
 *   pass 2  ntedit_hip_filter_insert_solid: est(x) = min of x's h sketch counters; every k-mer with est(x) >= cmin
 *           (1..255) sets its h bits in a plain filter slot (ntedit_hip_filter_alloc), or raises its h counters of a
 *           counting slot (ntedit_hip_filter_alloc_counting) to est(x) (max).  The slot's k and hash_num must be the
 *           sketch's.  Results are bit-for-bit independent of batching and order.
 * Batches follow ntedit_hip_filter_insert (host or device bytes, reads separated by e.g. '\n'; device batches
 * 16-byte aligned).  The sketch is held per context beside the two filter slots, on the device that is current on the
 * calling thread at ntedit_hip_sketch_alloc -- every call on a context makes its device current, so after
 * ntedit_hip_create on the same thread that is the context's.  Free it with ntedit_hip_sketch_free before
 * ntedit_hip_destroy.  Messages of these calls: ntedit_hip_reads_last_error() (ntedit_hip_last_error() belongs to
 * the context's own calls). */
int ntedit_hip_sketch_alloc(ntedit_hip_ctx* ctx, uint64_t counters, uint32_t hash_num, uint32_t k); /* counters: rounded up to a multiple of 8 */
int ntedit_hip_sketch_count(ntedit_hip_ctx* ctx, const char* bases, uint64_t n, int on_device);
int ntedit_hip_sketch_occupancy(ntedit_hip_ctx* ctx, uint64_t* nonzero, uint64_t* counters);
int ntedit_hip_sketch_download(ntedit_hip_ctx* ctx, uint8_t* counters);
int ntedit_hip_sketch_save_file(ntedit_hip_ctx* ctx, const char* path); /* as a counting filter file */
void ntedit_hip_sketch_free(ntedit_hip_ctx* ctx);
/* a zeroed counting filter (one 8-bit counter per byte, nbytes rounded up to a multiple of 8) in a filter slot */
int ntedit_hip_filter_alloc_counting(ntedit_hip_ctx* ctx, int slot, uint64_t nbytes, uint32_t hash_num, uint32_t k);
int ntedit_hip_filter_insert_solid(ntedit_hip_ctx* ctx, int slot, const char* bases, uint64_t n, int on_device, uint32_t cmin);
/* Pass 2 with a reject cutoff (the -e filter, "secondary BF with k-mers to reject", built from the same walk over the
 * reads): one kernel, one est(x) per k-mer; a k-mer with est(x) >= cmin sets its bits in the PRIMARY filter, one with
 * est(x) >= rmin also in the SECONDARY filter.  Both slots are checked as ntedit_hip_filter_insert_solid checks its
 * one (set, k and hash_num of the sketch, on its device), both must be plain filters, and cmin < rmin <= 255.  Each
 * filter ends with the bytes ntedit_hip_filter_insert_solid(slot, .., its threshold) over the same batches gives it.
 *   ntedit_hip_reads_set_reject_cutoff: the context's setting that the SOLID pass of ntedit_hip_reads_pass follows: with
 *           rmin > 0 it runs this call with (cmin, rmin) instead of ntedit_hip_filter_insert_solid.  0 turns it off.
 *           The setting lives with the sketch (NTEDIT_E_ARG without one) and goes with it. */
int ntedit_hip_filter_insert_solid2(ntedit_hip_ctx* ctx, const char* bases, uint64_t n, int on_device, uint32_t cmin, uint32_t rmin);
int ntedit_hip_reads_set_reject_cutoff(ntedit_hip_ctx* ctx, uint32_t rmin);
const char* ntedit_hip_reads_last_error(const ntedit_hip_ctx* ctx);
/* k-mer histogram of the read set, from the sketch (after pass 1 over the same inputs; --solid / --hist of the tool):
 *   ntedit_hip_sketch_histogram takes batches exactly as ntedit_hip_sketch_count and adds 1 to bin est(x) of the
 *           context's histogram for every k-mer occurrence x: occ[e] = occurrences whose estimate is e (e in 0..255;
 *           after pass 1 over the same inputs occ[0] = 0).  ntedit_hip_sketch_alloc zeroes it.  Integer sums: the
 *           result is bit-for-bit independent of batching, input form and order.
 * Two host-only calls (no device needed; failures are reported by ntedit_hip_reads_last_error(NULL)):
 *   ntedit_hip_reads_hist_summary: F1 = sum of occ[e] over e = 0..255 (the number of k-mer occurrences);
 *           f[c] = (occ[c] + c/2) / c in integer arithmetic for c = 1..255, f[0] = 0 (bin 255 means "255 or more",
 *           so f[255] is an upper bound on the distinct k-mers in it); F0 = sum of f[c].
 *   ntedit_hip_reads_solid_cutoff: the smallest c in [1, 253] with f[c+1] > f[c] (strictly), the first valley after
 *           the error peak; NTEDIT_E_ARG when there is none.  This is the project's own rule, not ntStat's model fit,
 *           and the counts are count-min estimates, not ntCard's. */
int ntedit_hip_sketch_histogram(ntedit_hip_ctx* ctx, const char* bases, uint64_t n, int on_device);
int ntedit_hip_sketch_histogram_download(ntedit_hip_ctx* ctx, uint64_t occ[256]);
int ntedit_hip_reads_hist_summary(const uint64_t occ[256], uint64_t f[256], uint64_t* F0, uint64_t* F1);
int ntedit_hip_reads_solid_cutoff(const uint64_t f[256], uint32_t* cmin);
/* Sharded builds (ntedit_amd/make_reads.py: each process counts its share of the reads, then the results merge):
 *   ntedit_hip_sketch_set_device adopts `counters` bytes of device memory, owned by the caller, as the context's
 *           sketch (counters a multiple of 8, the pointer 16-byte aligned; the caller zeroes it).  It replaces a sketch
 *           the context held; ntedit_hip_sketch_free then releases the state but never adopted memory.
 *   ntedit_hip_sketch_info: the sketch's counters, hash_num and k.
 *   ntedit_hip_merge_bytes folds n_src chunks of n device bytes, srcs[i * n .. (i + 1) * n), into dst[0 .. n): OP_SAT_ADD
 *           = min(255, sum) per byte (sketches), OP_OR (plain filters), OP_MAX (counting filters).  dst may be the first
 *           chunk.  On the device of dst; returns once the merge is done.  The identities
 *           min(255, sum_r min(255, c_r)) = min(255, sum_r c_r), OR of bits and max of estimates make the merge of
 *           per-process results over any split of the reads the one-process result.
 *   ntedit_hip_reads_pass: one pass of the tool (COUNT: pass 1, HIST: the histogram pass, SOLID: pass 2 into the
 *           primary slot, as ntedit_hip_filter_insert_solid) over n byte ranges [begins[i], ends[i]) of files[i],
 *           parsed as FASTA / FASTQ, plain or gzip, and fed to the GPU in batches of about batch_bytes.  A range owns
 *           the records whose first byte lies in it; ends[i] = ~0 and begins[i] = 0 read a whole file (the only form
 *           a gzip file takes).  starts[i] (may be NULL) receives where range i's first record starts (0 for
 *           begins[i] = 0; a range past byte 0 moves forward to a line that starts with '>' in FASTA, or with '@'
 *           and whose line + 2 starts with '+' in FASTQ), nexts[i] (may be NULL) where its reader stopped: the
 *           first record start at or past ends[i], the end of the file, or ~0 after a record that failed to parse.
 *           Consecutive ranges of a file read it as one reader would exactly when nexts[i] = starts[i + 1].
 * Host-only calls of the tool (no device; failures through ntedit_hip_reads_last_error(NULL)):
 *   ntedit_hip_reads_range_text: the reads of one range, each followed by '\n', into out[0 .. cap) (*len: the bytes
 *           they take; NTEDIT_E_OVERFLOW when that is more than cap), *reads: their number, *start / *next as above.
 *   ntedit_hip_reads_bf_size: ntedit-make-genome-bf's output bytes for num_elements at fpr.
 *   ntedit_hip_reads_default_sketch: the tool's default sketch counters, 16 per output byte, or with bf_bytes = 0
 *           (sized from the histogram) one per input byte with gzip files at 4 x their size; within [64 MiB, 32 GiB].
 *   ntedit_hip_reads_is_gzip: 1 if the file starts with the gzip magic.
 *   ntedit_hip_reads_write_hist: the --hist file (ntCard's text format) of f, F0, F1. */
#define NTEDIT_MERGE_SAT_ADD 0
#define NTEDIT_MERGE_OR 1
#define NTEDIT_MERGE_MAX 2
#define NTEDIT_READS_PASS_COUNT 0
#define NTEDIT_READS_PASS_HIST 1
#define NTEDIT_READS_PASS_SOLID 2
typedef struct ntedit_hip_reads_pass_stats
{
	uint64_t bases;  /* bases of the reads of k bases or more */
	double ms_wall;  /* the pass, parsing included */
	double ms_gpu;   /* the library's GPU calls */
} ntedit_hip_reads_pass_stats;
int ntedit_hip_sketch_set_device(ntedit_hip_ctx* ctx, void* device_counters, uint64_t counters, uint32_t hash_num, uint32_t k);
int ntedit_hip_sketch_info(ntedit_hip_ctx* ctx, uint64_t* counters, uint32_t* hash_num, uint32_t* k);
int ntedit_hip_merge_bytes(ntedit_hip_ctx* ctx, void* dst, const void* srcs, uint32_t n_src, uint64_t n, int op);
int ntedit_hip_reads_pass(ntedit_hip_ctx* ctx, int pass, const char* const* files, const uint64_t* begins, const uint64_t* ends,
                          uint32_t n, uint64_t batch_bytes, uint32_t cmin, ntedit_hip_reads_pass_stats* stats,
                          uint64_t* starts, uint64_t* nexts);
int ntedit_hip_reads_range_text(const char* path, uint64_t begin, uint64_t end, char* out, uint64_t cap, uint64_t* len,
                                uint64_t* reads, uint64_t* start, uint64_t* next);
uint64_t ntedit_hip_reads_bf_size(uint64_t num_elements, uint32_t hash_num, double fpr);
uint64_t ntedit_hip_reads_default_sketch(const char* const* files, uint32_t n, uint64_t bf_bytes);
int ntedit_hip_reads_is_gzip(const char* path);
int ntedit_hip_reads_write_hist(const char* path, const uint64_t f[256], uint64_t F0, uint64_t F1);
/* The resident store: the reads kept in HBM, packed, so that the passes after pass 1 do not parse the inputs again.
 *   ntedit_hip_resident_begin (after ntedit_hip_sketch_alloc or ntedit_hip_sketch_set_device; the store is the
 *           library's own device memory either way, and a new sketch or ntedit_hip_sketch_free releases it): from now
 *           on every ntedit_hip_sketch_count batch is
 *           also packed into the context's store, 3 bits per base: per 16 bytes of the batch one u32 of 2-bit codes
 *           (ACGT, case folded) and one u16 of validity bits (1 for ACGTacgt, 0 for any other byte, the separators
 *           between reads included), batch boundaries kept.  While the stored bytes stay within cap_bytes; a batch that
 *           would pass the cap, or a device allocation that fails, releases the whole store (state OVER_CAP /
 *           NO_MEMORY), and the later passes have to read the inputs again.  Restarts an existing store.
 *   ntedit_hip_resident_info: its state (NTEDIT_RESIDENT_*), batches, bytes of those batches (their `n`,
 *           separators included), device bytes it holds, and the cap.
 *   ntedit_hip_resident_histogram / _insert_solid: the histogram pass and pass 2 (as ntedit_hip_sketch_histogram
 *           and ntedit_hip_filter_insert_solid over the same batches) over every stored batch, each launched with its
 *           own n.  The kernels stage the same codes either way, so histogram and filter bytes are identical to those
 *           of the byte batches.  NTEDIT_E_ARG unless the state is ON.
 *   ntedit_hip_resident_free: releases it (ntedit_hip_sketch_free does too). */
#define NTEDIT_RESIDENT_OFF 0
#define NTEDIT_RESIDENT_ON 1
#define NTEDIT_RESIDENT_OVER_CAP 2
#define NTEDIT_RESIDENT_NO_MEMORY 3
typedef struct ntedit_hip_resident_stats
{
	int state;
	uint64_t batches;
	uint64_t bases;  /* bytes of the stored batches (reads and separators) */
	uint64_t bytes;  /* device bytes held */
	uint64_t cap;
} ntedit_hip_resident_stats;
int ntedit_hip_resident_begin(ntedit_hip_ctx* ctx, uint64_t cap_bytes);
int ntedit_hip_resident_info(ntedit_hip_ctx* ctx, ntedit_hip_resident_stats* st);
int ntedit_hip_resident_histogram(ntedit_hip_ctx* ctx);
int ntedit_hip_resident_insert_solid(ntedit_hip_ctx* ctx, int slot, uint32_t cmin);
int ntedit_hip_resident_insert_solid2(ntedit_hip_ctx* ctx, uint32_t cmin, uint32_t rmin); /* as ntedit_hip_filter_insert_solid2, over the store */
void ntedit_hip_resident_free(ntedit_hip_ctx* ctx);
/* A store that outlives its sketch: the stored codes and validity bits do not depend on k, so one pass over the read
 * files can serve sketches at several k (ntedit --reads -k K1,K2,...: a cascade of polishing rounds).
 *   ntedit_hip_sketch_reset: a fresh, zeroed sketch of `counters` counters, hash_num and k in place of the context's,
 *           the library's own memory, the histogram zeroed, WITHOUT releasing the store: its batches, bytes, cap and
 *           state stay as they are, and so does the ntedit_hip_reads_set_min_read setting (the reject cutoff goes with
 *           the old sketch).  Without a sketch or a store to keep it is ntedit_hip_sketch_alloc.  With counters = 0 it
 *           only releases the counters, the batch staging and the device parser's scratch: the context then holds no
 *           sketch (every sketch call is NTEDIT_E_ARG, ntedit_hip_resident_info and _free still answer) until the next
 *           reset.  If the new sketch cannot be allocated the store is released with the old one.
 *           ntedit_hip_sketch_alloc, _set_device and _free release the store, as always.
 *   ntedit_hip_resident_count: pass 1 (as ntedit_hip_sketch_count over the same batches) over every stored batch, each
 *           launched with its own n, into the context's current sketch: k_count staged from the store.  It stores
 *           nothing again.  The sketch equals, byte for byte, the one ntedit_hip_sketch_count fills from the batches'
 *           bytes at that k.  NTEDIT_E_ARG unless the state is ON.
 *   ntedit_hip_reads_set_min_read: the shortest record ntedit_hip_reads_pass keeps, host parser and --gpu_parse (plain
 *           and BGZF) alike; 0, or a length above the sketch's k, means k, as without the call.  A read shorter than k
 *           holds no k-mer, so a smaller length changes no sketch, histogram or filter; it makes the store hold the
 *           reads a later sketch at a smaller k has to count.  The `bases` of the pass statistics then count the reads
 *           of `len` bases or more.  The setting lives with the context's reads state (NTEDIT_E_ARG without a sketch). */
int ntedit_hip_sketch_reset(ntedit_hip_ctx* ctx, uint64_t counters, uint32_t hash_num, uint32_t k);
int ntedit_hip_resident_count(ntedit_hip_ctx* ctx);
int ntedit_hip_reads_set_min_read(ntedit_hip_ctx* ctx, uint32_t len);
/* --min_qual Q: a base whose Phred quality is below Q enters the batch text as 'N' (Phred+33: a FASTQ quality byte below
 * 33 + Q, a BAM quality byte below Q; Phred+64 is not built).  Only byte values change: the text has the same length, the
 * same reads and the same order as without it (records are kept by their length, masked bases included), and since every
 * kernel behind the parse breaks its k-mer walk at a non-ACGT byte, the sketch, the histogram, the filters and the
 * resident store all follow.  Records without qualities -- FASTA records, BAM records whose first quality byte is 0xFF --
 * pass unmasked.  The host parser masks by kseq's rules (multi-line FASTQ: the i-th quality character after
 * concatenation belongs to the i-th base); the device parser by nte_reads_grammar.h's rp_mask_base, the same function.
 *   ntedit_hip_reads_set_min_qual: the context's setting, 0 (off) to 93, that ntedit_hip_reads_pass,
 *           ntedit_hip_reads_parse_device and ntedit_hip_reads_bam_device follow; above 93: NTEDIT_E_ARG.  It needs no
 *           sketch and outlives ntedit_hip_sketch_reset and ntedit_hip_sketch_free: a cascade masks alike in every round.
 *   ntedit_hip_reads_min_qual_info: the context's last ntedit_hip_reads_pass (the pass zeroes them; the two device calls
 *           add to them): the bases that had a quality, and those of them below the minimum.  0, 0 with the setting off.
 *   ntedit_hip_reads_parse_model_q, _bam_model_q, _range_text_q: the host-only calls with min_qual as one more argument;
 *           the old names are these with 0. */
int ntedit_hip_reads_set_min_qual(ntedit_hip_ctx* ctx, uint32_t min_qual);
int ntedit_hip_reads_min_qual_info(ntedit_hip_ctx* ctx, uint64_t* qual_bases, uint64_t* masked_bases);
int ntedit_hip_reads_range_text_q(const char* path, uint64_t begin, uint64_t end, uint32_t min_qual, char* out, uint64_t cap,
                                  uint64_t* len, uint64_t* reads, uint64_t* start, uint64_t* next);
/* --min_read_len L, --min_mean_qual Q, --min_rq R: which reads go into the batch text.  A record goes in when it passes
 * every rule below; otherwise it is absent, as a record shorter than k is without them.  They hold for every pass over
 * the files, so the resident store only ever holds reads that passed.  (nte_reads_grammar.h, nte_bam_grammar.h: the one
 * place each rule is written; the host parser, the two models and the record kernels call them.)
 *   length        L is 1 to 2^31 - 1; the shortest record kept is max(L, what it is without: k, or what
 *                 ntedit_hip_reads_set_min_read set).
 *   rq            R is above 0 and at most 1.  A BAM record whose rq aux field of type f holds v is kept iff v >= R, as two
 *                 IEEE floats compare: a NaN is dropped.  A record without an rq:f field passes: every FASTA and FASTQ
 *                 record does.  The aux walk follows the SAM specification's types (A c C 1 byte, s S 2, i I f 4, Z H to a
 *                 NUL, B subtype + count * size), runs over [qual_off + l_seq, record end) and reads no byte outside it;
 *                 a field that does not fit, or of an unknown type, ends it: the record counts as having no tag, and as
 *                 aux_malformed.
 *   mean quality  Q is 1 to 60.  A read's mean quality is the Phred value of its mean error probability (as NanoFilt,
 *                 chopper and fastplong take it), not the mean of the Phred values, computed in integers: a base of Phred
 *                 quality q adds E[min(q, 93)], E[q] = round(2^31 * 10^(-q/10)) (a table of literals; a FASTQ byte below
 *                 33 counts as q = 0), S is the sum over the read as 64 bits, and the read is kept iff S <= len * E[Q].
 *                 Records without qualities pass: FASTA records, and BAM records whose first quality byte is 0xFF.  With
 *                 --min_qual the mean is taken over the qualities as stored, not over the masked text, and --min_qual's
 *                 counts cover the bases of the reads that were copied.
 * A dropped record is counted under the first rule that drops it, in the order flag (BAM, as before and in no count here),
 * length, rq, mean quality.
 *   ntedit_hip_reads_set_read_filter: the context's setting, with the lifetime of ntedit_hip_reads_set_min_qual; 0 turns a
 *           rule off (a min_rq that is not above 0 is off, -0.0 included), and with all three off every launch and every
 *           output is what it was before.  Out of range: NTEDIT_E_ARG.
 *           ntedit_hip_reads_build and its stages leave it as it is (it is no field of their arguments): their passes follow
 *           it, and report `read filter: D of N records dropped (length a, rq b, mean quality c)' per pass over the files.
 *   ntedit_hip_reads_get_read_filter: the setting back.
 *   ntedit_hip_reads_read_filter_info: the context's last ntedit_hip_reads_pass (the pass zeroes the counts; the device
 *           calls add to them).  All 0 with the setting off.
 *   ntedit_hip_reads_parse_model_f, _bam_model_f, _range_text_f: the host-only calls with the filter as further arguments
 *           (the text calls take no rq: no text record has the tag) and their counts (st may be NULL); the _q names are
 *           these with the filter off.  _range_text_f's min_len is the shortest record it returns. */
typedef struct ntedit_hip_reads_read_filter_stats
{
	uint64_t records;           /* the records the rules saw (BAM: those the flag rule let through) */
	uint64_t dropped_length;
	uint64_t dropped_rq;
	uint64_t dropped_mean_qual;
	uint64_t rq_tagged;         /* with --min_rq: records that reached the rq rule (neither flag nor length dropped them) and had an rq:f field */
	uint64_t aux_malformed;     /* ... and those whose aux walk ended at a field that does not fit or has an unknown type */
} ntedit_hip_reads_read_filter_stats;
int ntedit_hip_reads_set_read_filter(ntedit_hip_ctx* ctx, uint32_t min_len, uint32_t min_mean_qual, float min_rq);
int ntedit_hip_reads_get_read_filter(ntedit_hip_ctx* ctx, uint32_t* min_len, uint32_t* min_mean_qual, float* min_rq);
int ntedit_hip_reads_read_filter_info(ntedit_hip_ctx* ctx, ntedit_hip_reads_read_filter_stats* st);
int ntedit_hip_reads_range_text_f(const char* path, uint64_t begin, uint64_t end, uint32_t min_qual, uint32_t min_len,
                                  uint32_t min_mean_qual, char* out, uint64_t cap, uint64_t* len, uint64_t* reads, uint64_t* start,
                                  uint64_t* next, ntedit_hip_reads_read_filter_stats* st);
/* The whole filter build of ntedit-make-reads-bf, shared by it and `ntedit --reads`: the sketch (sketch_counters, as
 * sized by the caller), pass 1, with solid or hist_path the histogram pass (the --hist file, the --solid cutoff, and
 * with bf_bytes = 0 the output size from the histogram), the output filter allocated in the PRIMARY slot (counting
 * with `counts`), pass 2, the sketch freed.  With use_store the reads are kept resident from pass 1 (cap: store_cap
 * bytes) and the later passes read the store; past the cap they read the files, as without it.  Console lines go to
 * log(user, to_stdout, line): to_stdout = 0 for a timestamped information line, 1 for a line of standard output.  On
 * failure the message is ntedit_hip_reads_last_error(ctx); the sketch and the store are freed either way.
 *
 * ntedit_hip_reads_build is four stages in a row, exported for the sharded build (ntedit_amd/make_reads.py), which
 * walks the same four with its merges in between.  There `begins` / `ends` are set: files[i] is read in the byte range
 * [begins[i], ends[i]) (as ntedit_hip_reads_pass), the sketch and the PRIMARY filter are the device memory the caller
 * adopted (ntedit_hip_sketch_set_device, ntedit_hip_set_filter_device) instead of the library's own, and the pass and
 * store lines carry "rank <rank>/<world>: " and what was read.  The stages hand their state on in the result:
 *   ntedit_hip_reads_stage_count: the sketch, the store's begin, pass 1 (starts / nexts as ntedit_hip_reads_pass
 *           reports them, may be NULL), the store's state and its lines.  Zeroes *res first.
 *   ntedit_hip_reads_stage_histogram: the histogram pass, from the store or over the same ranges; occ[256] as
 *           ntedit_hip_sketch_histogram_download.
 *   ntedit_hip_reads_stage_decide: host only, no context.  From occ (the caller's own or the sum over the ranks; NULL
 *           when no histogram was gathered) to res->cmin and res->bf_bytes: the histogram's lines, the --hist file
 *           (written before a refused --solid: it is left to look at), the --solid cutoff, the size from the
 *           histogram, and the refusals (NTEDIT_E_ARG; the message is ntedit_hip_reads_last_error(NULL)).  Only
 *           rank 0 writes --hist and logs; every rank reaches the same refusal.
 *   ntedit_hip_reads_stage_insert: the filter of res->bf_bytes, pass 2 with res->cmin from the store or over the
 *           ranges, the sketch and the store freed.
 * With reject_cmin > 0 the build also makes the reject filter (ntedit -e) in the SECONDARY slot: a plain filter of the
 * k-mers with est(x) >= reject_cmin, from the same pass 2 (ntedit_hip_filter_insert_solid2).  The sketch is sized from
 * the primary output alone, so the primary filter's bytes are those of the build without it, and the reject filter's
 * bytes are those of a build with cmin = reject_cmin, bf_bytes = its size and the same sketch.  stage_decide resolves
 * its size (reject_bf_bytes as given, or from the histogram the k-mers at reject_cmin or above) into
 * res->reject_bf_bytes and refuses reject_cmin <= res->cmin; stage_insert allocates it (a sharded build: the SECONDARY
 * filter the caller adopted).  Not with `counts`.
 *
 * A build may start from the store an earlier build left (keep_store, not for a sharded build): when the context's store
 * is ON at ntedit_hip_reads_stage_count, the sketch is made with ntedit_hip_sketch_reset, pass 1 is
 * ntedit_hip_resident_count and no file is opened by any pass; files / min_read are then unused, and the pass lines
 * give the store's bytes (reads and separators) as their bases.  With keep_store a build that succeeds ends with
 * ntedit_hip_sketch_reset(ctx, 0, 0, 0) instead of ntedit_hip_sketch_free when its store is ON; a build that fails, or
 * whose store was released, frees everything as without it. */
typedef struct ntedit_hip_reads_build_args
{
	const char* const* files;
	uint32_t n_files;
	uint32_t k, hash_num;
	uint32_t cmin;            /* unless solid */
	int solid;                /* cmin from the histogram (ntedit_hip_reads_solid_cutoff) */
	int counts;               /* a counting output filter */
	uint64_t bf_bytes;        /* 0: --num_elements from the histogram (needs solid or hist_path) */
	double fpr;
	uint64_t sketch_counters;
	uint64_t batch_bytes;
	const char* hist_path;    /* NULL: none */
	const char* sketch_path;  /* NULL: none (the sketch after pass 1, as a counting filter file) */
	int use_store;
	uint64_t store_cap;
	void (*log)(void* user, int to_stdout, const char* line);
	void* user;
	const uint64_t* begins;   /* NULL: the files whole, one process; else a rank's share of a sharded build */
	const uint64_t* ends;
	uint32_t rank, world;
	int device_parse;         /* --gpu_parse: plain files are parsed on the device (ntedit_hip_reads_parse_device) */
	uint32_t reject_cmin;     /* --reject_cutoff; 0: no reject filter */
	uint64_t reject_bf_bytes; /* --reject_bf, or from --reject_num_elements; 0: from the histogram (needs solid or hist_path) */
	uint64_t reject_num_elements; /* as given (the parameter echo) */
	uint32_t min_read;        /* ntedit_hip_reads_set_min_read for this build's passes over the files; 0: k */
	int keep_store;           /* the build ends with the sketch released and the store, if it is ON, kept for the next build */
	uint32_t min_qual;        /* --min_qual: ntedit_hip_reads_set_min_qual for this build's passes over the files; 0: off */
} ntedit_hip_reads_build_args;
typedef struct ntedit_hip_reads_build_result
{
	uint32_t cmin;                        /* the one pass 2 used */
	uint64_t bf_bytes;                    /* the output filter's size */
	ntedit_hip_reads_pass_stats pass[3];  /* by NTEDIT_READS_PASS_* (HIST zero when it did not run) */
	int store_state;                      /* after pass 1 (OFF without use_store) */
	uint64_t store_bytes;                 /* device bytes the store held after pass 1 */
	double ms_total;
	uint64_t store_batches;               /* batches it held after pass 1 */
	uint64_t reject_bf_bytes;             /* the reject filter's size (0: none) */
	int from_store;                       /* 1: the build began with a store that was ON, and pass 1 read it too */
} ntedit_hip_reads_build_result;
int ntedit_hip_reads_build(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* args, ntedit_hip_reads_build_result* res);
int ntedit_hip_reads_stage_count(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* args, ntedit_hip_reads_build_result* res,
                                 uint64_t* starts, uint64_t* nexts);
int ntedit_hip_reads_stage_histogram(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* args,
                                     ntedit_hip_reads_build_result* res, uint64_t occ[256]);
int ntedit_hip_reads_stage_decide(const ntedit_hip_reads_build_args* args, const uint64_t occ[256], ntedit_hip_reads_build_result* res);
int ntedit_hip_reads_stage_insert(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* args, ntedit_hip_reads_build_result* res);
/* The reads options of the four front ends (ntedit-make-reads-bf and python -m ntedit_amd.make_reads: the TOOL dialect,
 * "-c", sentences; ntedit --reads and python -m ntedit_amd.run --reads: the POLISHER dialect, "--cutoff"), checked in one
 * place.  Host only, no device.  The options come as their text (NULL: not given).  With final = 0 only the options
 * given so far are checked for what is refused at the option itself (a malformed number, --fpr), so that a front end
 * can ask while it walks its arguments; with final = 1 every rule, in that dialect's order: -k required and 12..200,
 * the cutoff xor --solid and 1..255, hashes 1..8, a size unless the histogram gives it, the filter would be empty,
 * batch_bytes >= 4096, then the reject filter's: --reject_cutoff 2..255 and above the cutoff given, not with --counts, a
 * size (--reject_bf or --reject_num_elements) unless the histogram gives it, no size without it, not empty, then
 * --min_qual 1..93 (a malformed one is refused at the option, like every number).  (Under
 * --solid "above the cutoff" waits for ntedit_hip_reads_stage_decide.)  Returns 0 and the normalised arguments, or the first refusal: NTEDIT_READS_REFUSED,
 * NTEDIT_READS_NOT_A_NUMBER (a malformed number), NTEDIT_READS_EMPTY (TOOL dialect: the filter would be empty; the
 * tool prints its parameters before it says so, and *out is filled), its message in ntedit_hip_reads_last_error(NULL). */
#define NTEDIT_READS_DIALECT_TOOL 0
#define NTEDIT_READS_DIALECT_POLISHER 1
#define NTEDIT_READS_REFUSED 1
#define NTEDIT_READS_NOT_A_NUMBER 2
#define NTEDIT_READS_EMPTY 3
#define NTEDIT_READS_BATCH_DEFAULT (256ull << 20)
#define NTEDIT_READS_RESIDENT_CAP_DEFAULT (48ull << 30) /* 128 Gbases at 3 bits per base */
#define NTEDIT_READS_GZIP_WEIGHT 4 /* a gzip byte counts as 4 plain ones (default sketch, the sharded partition) */
typedef struct ntedit_hip_reads_options
{
	const char *k, *cutoff, *hashes, *fpr, *bf, *num_elements, *sketch_bytes, *batch_bytes, *store_cap, *threads;
	int solid, hist;
	const char* const* files; /* for the default sketch */
	uint32_t n_files;
	int gpu_parse;
	const char *reject_cutoff, *reject_bf, *reject_num_elements;
	int counts;     /* --counts (refused with --reject_cutoff) */
	int reject_out; /* an output option of the reject filter was given (--reject_out / --save_reject_bf) */
	const char* min_qual; /* --min_qual (1 to 93) */
} ntedit_hip_reads_options;
typedef struct ntedit_hip_reads_rules
{
	uint32_t k, cmin, hash_num; /* cmin 0: --solid */
	double fpr;
	uint64_t bf_bytes;          /* --bf, or from --num_elements; 0: sized from the histogram */
	uint64_t num_elements;
	uint64_t sketch_bytes;      /* as given (0: default) */
	uint64_t sketch_counters;   /* the sketch to allocate */
	uint64_t batch_bytes, store_cap, threads;
	int gather_hist, size_from_hist;
	int gpu_parse;
	uint32_t reject_cmin;          /* 0: no reject filter */
	uint64_t reject_bf_bytes;      /* --reject_bf, or from --reject_num_elements; 0: sized from the histogram */
	uint64_t reject_num_elements;
	int reject_size_from_hist;
	uint32_t min_qual;             /* 0: off */
} ntedit_hip_reads_rules;
int ntedit_hip_reads_options_check(const ntedit_hip_reads_options* opts, int dialect, int final, ntedit_hip_reads_rules* out);
/* The rules of --min_read_len, --min_mean_qual and --min_rq, in the same two dialects and with the same meaning of
 * `final`; a front end asks them behind ntedit_hip_reads_options_check.  They have structs of their own: the three above
 * end where they ended before, so a caller built against them is untouched.  A malformed number is refused at the option
 * (NTEDIT_READS_NOT_A_NUMBER; --min_rq is read with strtof); with final = 1 the ranges, one sentence each: --min_read_len
 * 1..2147483647, --min_rq above 0 and at most 1, --min_mean_qual 1..60 (NTEDIT_READS_REFUSED).  The build takes the
 * outcome as the context's setting: ntedit_hip_reads_set_read_filter before ntedit_hip_reads_build or its stages. */
typedef struct ntedit_hip_reads_filter_options
{
	const char *min_read_len, *min_mean_qual, *min_rq;
} ntedit_hip_reads_filter_options;
typedef struct ntedit_hip_reads_filter_rules
{
	uint32_t min_read_len;  /* 0: off */
	uint32_t min_mean_qual; /* 0: off */
	float min_rq;           /* 0: off */
} ntedit_hip_reads_filter_rules;
int ntedit_hip_reads_filter_options_check(const ntedit_hip_reads_filter_options* opts, int dialect, int final,
                                          ntedit_hip_reads_filter_rules* out);
/* --gpu_parse: plain (not gzip) read files parsed on the device.  The host ships raw file bytes, cut at record starts
 * into chunks of about batch_bytes; kernels (nte_reads_parse.hip) make of each chunk, in HBM, exactly the batch text the
 * host parser makes -- every read of k bases or more followed by '\n', in file order -- and that text goes to the passes
 * as a device batch.  A parallel parser cannot follow kseq's rules on arbitrary input, so it verifies a clean grammar
 * (nte_reads_grammar.h: no '\r', no empty line; FASTA: '>' lines are headers, every other line is sequence and starts
 * with none of '>', '+', '@'; FASTQ: 4 lines per record, '@', sequence, '+', a quality line as long as the sequence) and
 * reports a chunk that breaks it unclean; from the first unclean chunk of a range on, the rest of that range goes to the
 * host parser, from that chunk's first byte.  A clean chunk has exactly the host parser's text, so no output changes.
 *   ntedit_hip_reads_parse_device: one chunk.  raw: n_raw host or device bytes (device: 16-byte aligned) that start at
 *           a record start; text_device: 16-byte aligned device memory of text_cap >= n_raw bytes (the text is never
 *           longer than the raw bytes).  res->clean = 1 and the text's length, reads and bases, or clean = 0 and
 *           `broken`, the rules found broken (NTEDIT_PARSE_BAD_*; the device stops at what it finds first, so on an
 *           unclean chunk it may name fewer rules than the model), the text then undefined.  At most 2^31 - 1 bytes and
 *           one line per 8 raw bytes (+ 1), else unclean.  Scratch is the context's, grows only, and is released by
 *           ntedit_hip_sketch_free.
 *   ntedit_hip_reads_parse_model: the same grammar functions run serially on the host (no device; failures through
 *           ntedit_hip_reads_last_error(NULL)): the text into out[0 .. cap), NTEDIT_E_OVERFLOW when it does not fit.
 *   ntedit_hip_reads_set_device_parse: the context's setting that ntedit_hip_reads_pass follows (the stage calls set it
 *           from args->device_parse); gzip files stay with the host parser either way.
 *   ntedit_hip_reads_parse_info: the last pass of the context: chunks parsed on the device, chunks handed to the host
 *           parser after an unclean one, the raw bytes shipped, the text bytes made, milliseconds in the parse kernels. */
#define NTEDIT_PARSE_TILE 16384
#define NTEDIT_PARSE_BAD_FIRST 1
#define NTEDIT_PARSE_BAD_CR 2
#define NTEDIT_PARSE_BAD_EMPTY 4
#define NTEDIT_PARSE_BAD_SEQ_START 8
#define NTEDIT_PARSE_BAD_FQ_LINES 16
#define NTEDIT_PARSE_BAD_FQ_HEADER 32
#define NTEDIT_PARSE_BAD_FQ_PLUS 64
#define NTEDIT_PARSE_BAD_FQ_QUAL 128
#define NTEDIT_PARSE_BAD_TABLE 256
#define NTEDIT_PARSE_BAD_SIZE 512
typedef struct ntedit_hip_reads_parse_result
{
	int clean;        /* 1: in the clean grammar, the text is the host parser's; 0: not */
	uint32_t broken;  /* 0 when clean */
	int kind;         /* the chunk's first byte */
	uint64_t text_len, reads, bases, lines;
} ntedit_hip_reads_parse_result;
typedef struct ntedit_hip_reads_parse_stats
{
	uint64_t device_chunks;   /* clean chunks, parsed on the device */
	uint64_t fallback_chunks; /* unclean chunks: each sends the rest of its range to the host parser */
	uint64_t raw_bytes;       /* shipped to the device */
	uint64_t text_bytes;      /* made there */
	double ms_kernels;
	uint32_t broken;          /* the rules the unclean chunks broke */
	uint32_t host_files;      /* gzip ranges, left to the host parser */
} ntedit_hip_reads_parse_stats;
int ntedit_hip_reads_parse_device(ntedit_hip_ctx* ctx, const char* raw, uint64_t n_raw, int on_device, uint32_t k, char* text_device,
                                  uint64_t text_cap, ntedit_hip_reads_parse_result* res);
int ntedit_hip_reads_parse_model(const char* raw, uint64_t n_raw, uint32_t k, char* out, uint64_t cap, ntedit_hip_reads_parse_result* res);
int ntedit_hip_reads_parse_model_q(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, char* out, uint64_t cap,
                                   ntedit_hip_reads_parse_result* res);
int ntedit_hip_reads_parse_model_f(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, uint32_t min_len, uint32_t min_mean_qual,
                                   float min_rq, char* out, uint64_t cap, ntedit_hip_reads_parse_result* res,
                                   ntedit_hip_reads_read_filter_stats* st);
int ntedit_hip_reads_set_device_parse(ntedit_hip_ctx* ctx, int on);
int ntedit_hip_reads_parse_info(ntedit_hip_ctx* ctx, ntedit_hip_reads_parse_stats* st);
/* --gpu_parse on BGZF reads (the output of bgzip: independent gzip members of at most 64 KiB inflated each, their
 * compressed size in the header's 'BC' subfield, CRC-32 and ISIZE behind each).  ntedit_hip_reads_pass ships such a file
 * compressed, kernels (nte_reads_inflate.hip; the decoder is nte_bgzf_inflate.h) inflate its members in HBM and check
 * their CRCs there, and the inflated bytes go to the parse kernels above; they never exist on the host.  A single-stream
 * .gz stays with the host parser.  A member the device refuses fails the pass; an unclean chunk, or a member in
 * mid-file that is not BGZF, sends the rest of the file to the host parser from an exact record start.
 *   ntedit_hip_bgzf_walk: the member headers of bytes[0 .. n): the members that lie completely inside (at most cap),
 *           in_off / out_off counted from bytes[0] and from the first member's first inflated byte; *consumed: where
 *           the next member starts.  Returns why it stopped: NTEDIT_BGZF_END (the buffer's end), _CUT (the next member
 *           is cut off by the buffer's end), _NOT (what starts there is no BGZF member), _FULL (cap members found).
 *   ntedit_hip_reads_inflate_device: one call inflates a set of members.  comp: host or device bytes; out_device:
 *           device memory; every member must lie inside comp[0 .. n_comp) and out[0 .. out_cap) (else NTEDIT_E_ARG).
 *           status[i] (host): 0, member i is inflated and its CRC-32 holds, or the reason it was refused
 *           (NTEDIT_INFLATE_*); a refused member leaves its output bytes undefined and touches no byte outside them.
 *   ntedit_hip_reads_inflate_model: the same decoder functions run serially on the host (no device; failures through
 *           ntedit_hip_reads_last_error(NULL)), into host memory.
 *   ntedit_hip_reads_last_record_start: the chunk cut's rule on the host (what RawFeeder cuts plain files by): the last
 *           record start in buf[0 .. n) past its first byte -- '>' at a line start (kind '>'), or an '@' line whose
 *           line + 2, inside the buffer, starts with '+' -- or NTEDIT_READS_NO_START.
 *   ntedit_hip_reads_last_start_device: the same from the device's line table; kind is the buffer's first byte ('>' or
 *           '@'; any other: n).  At most 2^31 - 1 bytes and one line per 8 bytes (+ 1).
 *   ntedit_hip_reads_inflate_info: the last pass of the context. */
#define NTEDIT_BGZF_END 0
#define NTEDIT_BGZF_CUT 1
#define NTEDIT_BGZF_NOT 2
#define NTEDIT_BGZF_FULL 3
#define NTEDIT_INFLATE_BAD_BLOCK 1
#define NTEDIT_INFLATE_BAD_CODES 2
#define NTEDIT_INFLATE_BAD_DIST 3
#define NTEDIT_INFLATE_OUT_OVER 4
#define NTEDIT_INFLATE_IN_OVER 5
#define NTEDIT_INFLATE_SHORT_OUT 6
#define NTEDIT_INFLATE_LEFT_IN 7
#define NTEDIT_INFLATE_BAD_CRC 8
#define NTEDIT_INFLATE_BAD_STORED 9
#define NTEDIT_INFLATE_BAD_SYMBOL 10
#define NTEDIT_READS_NO_START (~0ull)
typedef struct ntedit_hip_bgzf_member
{
	uint64_t in_off;  /* of the member's DEFLATE data */
	uint64_t out_off; /* of its inflated bytes */
	uint32_t n_in;    /* bytes of DEFLATE data */
	uint32_t n_out;   /* ISIZE */
	uint32_t crc;     /* CRC-32 of the inflated bytes */
	uint32_t reserved;
} ntedit_hip_bgzf_member;
typedef struct ntedit_hip_reads_inflate_stats
{
	uint64_t members;      /* inflated on the device */
	uint64_t comp_bytes;   /* shipped to the device */
	uint64_t raw_bytes;    /* inflated there */
	double ms_kernels;     /* in the inflate and cut kernels */
	uint32_t files;        /* BGZF files fed to the device */
	uint32_t handed_back;  /* ... of which the host parser finished */
	uint64_t handed_back_at; /* the inflated offset the last of those was handed back at */
	uint64_t bad_member;   /* the first refused member's index in its file (bad_reason != 0) */
	uint32_t bad_reason;   /* NTEDIT_INFLATE_* */
	uint32_t reserved;
} ntedit_hip_reads_inflate_stats;
int ntedit_hip_bgzf_walk(const void* bytes, uint64_t n, ntedit_hip_bgzf_member* members, uint64_t cap, uint64_t* n_members,
                         uint64_t* consumed);
int ntedit_hip_reads_inflate_device(ntedit_hip_ctx* ctx, const void* comp, uint64_t n_comp, int on_device,
                                    const ntedit_hip_bgzf_member* members, uint64_t n_members, void* out_device, uint64_t out_cap,
                                    uint32_t* status);
int ntedit_hip_reads_inflate_model(const void* comp, uint64_t n_comp, const ntedit_hip_bgzf_member* members, uint64_t n_members,
                                   void* out, uint64_t out_cap, uint32_t* status);
uint64_t ntedit_hip_reads_last_record_start(const char* buf, uint64_t n, int kind);
int ntedit_hip_reads_last_start_device(ntedit_hip_ctx* ctx, const void* buf, uint64_t n, int on_device, uint64_t* cut);
int ntedit_hip_reads_inflate_info(ntedit_hip_ctx* ctx, ntedit_hip_reads_inflate_stats* st);
/* --gpu_parse on BAM reads, unaligned or aligned (SAM specification 4.2; a BAM is a BGZF container).  ntedit_hip_reads_pass
 * ships the file compressed and inflates its members as for BGZF FASTQ; kernels (nte_reads_bam.hip; the grammar is
 * nte_bam_grammar.h) then find the records of the inflated chunk and unpack the 4-bit bases of the kept ones into the
 * batch text.  A record is kept when (flag & 0x900) == 0 (secondary and supplementary alignments repeat bases the primary
 * record holds) and l_seq >= min_len; the strand flag 0x10 is not applied (the k-mers are canonical).  The text is every
 * kept record's bases followed by '\n', in file order: exactly the host parser's text for the FASTQ of the same reads.
 * The chain of block_size fields is walked speculatively: the chunk is cut into segments, every segment guesses its
 * first record start and walks from it, and a stitch step keeps a segment's table only when the chain before it arrives
 * at its guess, and walks it again from the true entry otherwise.  The result is the chain from the true entry.
 *   ntedit_hip_reads_is_bam: 1 if the file starts with BGZF members that inflate to "BAM\1" (host only, the inflate
 *           model: members are inflated until four bytes are at hand, so a first member of one to three bytes, or of
 *           none, is taken; those members have to lie in the file's first 68 KiB), else 0.
 *   ntedit_hip_reads_bam_device: one chunk.  raw: n_raw host or device bytes (device: 16-byte aligned) that start at
 *           the file's first byte (at_header = 1) or at a record start (0); text_device: 16-byte aligned device memory
 *           of text_cap >= n_raw bytes (the text is never longer than the raw bytes).  res->clean = 1, `cut` (the offset
 *           of the first record that does not lie completely inside the chunk: the bytes from there on belong in front
 *           of the next chunk; 0 when the header does not fit) and the counts of the records before the cut; or
 *           clean = 0, `broken` (NTEDIT_BAM_BAD_*), `cut` the offset of the header or record that breaks the rule, the
 *           counts 0 and the text undefined.  At most 2^31 - 1 bytes, else NTEDIT_BAM_BAD_SIZE.
 *   ntedit_hip_reads_bam_model: the same grammar functions run serially on the host (no device; failures through
 *           ntedit_hip_reads_last_error(NULL)): the text into out[0 .. cap), NTEDIT_E_OVERFLOW when it does not fit.
 *   ntedit_hip_reads_bam_set_segment: the segment size of the walk, in bytes (0: the default, NTEDIT_BAM_SEGMENT; at
 *           least 64; a size of the chunk's or more makes the walk one chain).  A tuning knob: no result depends on it.
 *   ntedit_hip_reads_bam_info: the context's counters since ntedit_hip_reads_pass last began (the pass zeroes them;
 *           ntedit_hip_reads_bam_device adds to them too). */
#define NTEDIT_BAM_SEGMENT 8192
#define NTEDIT_BAM_BAD_MAGIC 1
#define NTEDIT_BAM_BAD_HEADER 2
#define NTEDIT_BAM_BAD_RECORD 4
#define NTEDIT_BAM_BAD_SIZE 8
typedef struct ntedit_hip_reads_bam_result
{
	int clean;
	uint32_t broken;       /* 0 when clean */
	uint64_t header_len;   /* at_header and the header fits: its bytes; else 0 */
	uint32_t n_ref, reserved;
	uint64_t cut;
	uint64_t records;      /* before the cut */
	uint64_t kept, skipped_flag, skipped_short;
	uint64_t bases;        /* of the kept records */
	uint64_t text_len;     /* bases + kept */
} ntedit_hip_reads_bam_result;
typedef struct ntedit_hip_reads_bam_stats
{
	uint64_t files, chunks;
	uint64_t records, kept, skipped_flag, skipped_short;
	uint64_t segments;     /* walked speculatively */
	uint64_t rewalked;     /* ... of which the stitch walked again from the true entry */
	double ms_walk;        /* in the walk and stitch kernels (the one-lane header kernel, once per file, is not timed) */
	double ms_decode;      /* in the length, scan and unpack kernels */
} ntedit_hip_reads_bam_stats;
int ntedit_hip_reads_is_bam(const char* path);
int ntedit_hip_reads_bam_device(ntedit_hip_ctx* ctx, const void* raw, uint64_t n_raw, int on_device, int at_header, uint32_t min_len,
                                char* text_device, uint64_t text_cap, ntedit_hip_reads_bam_result* res);
int ntedit_hip_reads_bam_model(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, char* out, uint64_t cap,
                               ntedit_hip_reads_bam_result* res);
int ntedit_hip_reads_bam_model_q(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, uint32_t min_qual, char* out,
                                 uint64_t cap, ntedit_hip_reads_bam_result* res);
int ntedit_hip_reads_bam_model_f(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, uint32_t min_qual, uint32_t min_read_len,
                                 uint32_t min_mean_qual, float min_rq, char* out, uint64_t cap, ntedit_hip_reads_bam_result* res,
                                 ntedit_hip_reads_read_filter_stats* st);
/* k_bam_facts (--min_rq, --min_mean_qual on BAM) gives each record a group of 8, 16 or 64 lanes, chosen by the mean length
 * of the reads the chunk before kept; _set_group_width forces one (0: back to the choice), _group_width tells the width
 * the last chunk ran at (0: the kernel has not run). */
int ntedit_hip_reads_bam_set_group_width(ntedit_hip_ctx* ctx, uint32_t lanes);
int ntedit_hip_reads_bam_group_width(ntedit_hip_ctx* ctx);
int ntedit_hip_reads_bam_set_segment(ntedit_hip_ctx* ctx, uint64_t bytes);
int ntedit_hip_reads_bam_info(ntedit_hip_ctx* ctx, ntedit_hip_reads_bam_stats* st);
/* --gpu_parse for genome FASTA (ntedit-make-genome-bf --gpu_parse, ntedit --genome --gpu_parse).  A chromosome does not
 * fit a chunk that has to start at a record start, so a genome chunk is any run of raw bytes of a FASTA file, cut
 * anywhere, entered in a state (nte_genome_grammar.h): at a line start, inside a '>' line, or inside a sequence line.
 * Its text is one '\n' for every header line that begins in the chunk and the bytes of every sequence line or piece of
 * one, in raw order; the texts of consecutive chunks, each entered with its predecessor's exit state, concatenate to the
 * text of the whole file, whose pieces between '\n' are the records' sequences.  A chunk is clean unless it holds a
 * '\r', an empty line that begins in it, a sequence line that begins in it with '+' or '@', is the file's first chunk
 * and does not start with '>', has more than n / 8 + 1 lines or 2^31 bytes or more (NTEDIT_PARSE_BAD_*).
 *   ntedit_hip_genome_parse_device: one chunk.  raw: n_raw host or device bytes (device: 16-byte aligned); text_device:
 *           16-byte aligned device memory of text_cap >= n_raw bytes (the text is never longer than the raw bytes).
 *           Every field of *res is filled whether the chunk is clean or not, and the text is the grammar's either way
 *           (a small chunk of short lines is over the line bound, and chunking still never changes the text); only
 *           with 2^31 bytes or more, or more lines than (n_raw + 2^20) / 8 + 1, the chunk is not looked at further:
 *           `broken` and `lines` are all the result then holds.  Scratch is the context's, as for
 *           ntedit_hip_reads_parse_device.
 *   ntedit_hip_genome_parse_model: the same grammar functions run serially on the host (no device; failures through
 *           ntedit_hip_reads_last_error(NULL)): the text into out[0 .. cap), NTEDIT_E_OVERFLOW when it does not fit.
 *   ntedit_hip_genome_pass: the files, one after the other, in chunks of batch_bytes raw bytes cut wherever they end.
 *           Plain files are read into page-locked buffers and copied while the chunk before is parsed; BGZF files are
 *           shipped compressed in whole members and inflated on the device (ntedit_hip_reads_inflate_device).  insert
 *           != 0: each chunk's text, behind the last k - 1 text bytes of its file before it, goes to
 *           ntedit_hip_filter_insert(slot) as a device batch (the slot's k); insert = 0: the pass only sums the bases
 *           (the sizing pass; no filter needed).  From the first unclean chunk of a file on, the host parser takes the
 *           file, from the file's last known record start at or before that chunk (insertion is idempotent; the sizing
 *           pass reads such a file again from its start); single-stream .gz files and files that do not start with '>'
 *           take the host parser whole, and with batch_bytes 0 every file does (the pass without --gpu_parse).  A BGZF
 *           member the inflater refuses fails the pass.  stats->bases: the bases of
 *           all records, as ntedit-make-genome-bf prints them.
 *   ntedit_hip_genome_pass_get_info: the last pass of the context, as a ntedit_hip_genome_pass_info. */
#define NTEDIT_GENOME_LINE_START 0
#define NTEDIT_GENOME_IN_HEADER 1
#define NTEDIT_GENOME_IN_SEQ 2
typedef struct ntedit_hip_genome_parse_result
{
	int clean;            /* 1: no rule is broken */
	uint32_t broken;      /* NTEDIT_PARSE_BAD_*, 0 when clean */
	int state_out;        /* NTEDIT_GENOME_*: the state the next chunk is entered in */
	int reserved;
	uint64_t text_len;
	uint64_t bases;       /* the sequence bytes copied */
	uint64_t lines;
	uint64_t last_header; /* the raw offset where the last header line that begins in the chunk starts, or NTEDIT_READS_NO_START */
} ntedit_hip_genome_parse_result;
typedef struct ntedit_hip_genome_pass_info
{
	uint64_t device_chunks; /* clean chunks, parsed on the device */
	uint64_t raw_bytes;     /* their raw (inflated) bytes */
	uint64_t text_bytes;    /* the text made of them */
	double ms_kernels;      /* in the parse kernels */
	uint32_t handed_back;   /* files the host parser finished after an unclean chunk */
	uint32_t broken;        /* the rules those chunks broke */
	uint32_t host_files;    /* files left to the host parser whole (single-stream .gz, no '>' at the start) */
	uint32_t bgzf_files;    /* files inflated on the device */
	uint64_t bgzf_members;  /* ... and their members */
} ntedit_hip_genome_pass_info;
int ntedit_hip_genome_parse_device(ntedit_hip_ctx* ctx, const char* raw, uint64_t n_raw, int on_device, int state_in, int first_chunk,
                                   char* text_device, uint64_t text_cap, ntedit_hip_genome_parse_result* res);
int ntedit_hip_genome_parse_model(const char* raw, uint64_t n_raw, int state_in, int first_chunk, char* out, uint64_t cap,
                                  ntedit_hip_genome_parse_result* res);
int ntedit_hip_genome_pass(ntedit_hip_ctx* ctx, int slot, const char* const* files, uint32_t n, uint64_t batch_bytes, int insert,
                           ntedit_hip_reads_pass_stats* stats);
int ntedit_hip_genome_pass_get_info(ntedit_hip_ctx* ctx, ntedit_hip_genome_pass_info* info);
/* the pass's information line(s), as the front ends print them: into out[0 .. cap), '\n' between lines */
int ntedit_hip_genome_pass_line(ntedit_hip_ctx* ctx, char* out, uint64_t cap);


/* ---- hot path ------------------------------------------------------------
 * Batch layout: `bases` holds the contigs of the batch; contig i occupies
 * bases[offsets[i] .. offsets[i]+lens[i]) and every contig is followed by at
 * least one byte that is not an accepted base (the host driver uses '\n').
 * n = total bytes.  on_device: NTEDIT_HIP_BASES_HOST (0) `bases` is host memory, NTEDIT_HIP_BASES_DEVICE (1) it is
 * already in HBM, NTEDIT_HIP_BASES_PACKED (2; ntedit_hip_polish_batch only) it is host memory in the packed form below. */
#define NTEDIT_HIP_BASES_HOST 0
#define NTEDIT_HIP_BASES_DEVICE 1
#define NTEDIT_HIP_BASES_PACKED 2

/* The packed form of a batch: what crosses PCIe when the producer of the batch (a FASTA parser touches every byte
 * anyway) hands it over as 4-bit character codes instead of bytes -- 5 bits per base instead of 8 on a link that is
 * slower than the screening (3 GB of draft: ~110 ms at 27 GB/s against ~95 ms of screening).  Layout, for n bytes:
 *   codes   ceil(n / 32) * 16 bytes: two codes per byte, even position in the low nibble; 0..13 = the accepted bases
 *           A C G T R Y S W K M B D H V (either case), 15 = anything else (N, separators, ...)
 *   case    ceil(n / 128) * 16 bytes, right behind the codes: bit i (LSB first) = byte i is a lower-case letter
 * The device unpacks it into the byte batch every kernel reads (code 15 comes back as 'N' / 'n': to the hot path every
 * non-accepted byte is the same, ntedit.cpp:493-499), so results do not depend on the form.  Bytes that are NOT the
 * same to it -- U / u and the handful of other bytes whose ntHash seed is not zero (nte_common.h, is_exotic) -- cannot
 * be packed: ntedit_hip_pack_bases() then returns 1 and the caller hands the batch over as bytes.
 * `bases` stays the batch for ntedit_hip_write_outputs() either way (the renderer copies draft bytes).
 * threads: 0 = the ntedit_hip_set_host_threads() setting.  Returns 0, 1 (not packable) or NTEDIT_E_ARG. */
uint64_t ntedit_hip_packed_size(uint64_t n);
int ntedit_hip_pack_bases(const char* bases, uint64_t n, void* packed, unsigned threads);

/* Page-locked host memory for batches (optional): a batch handed over from such a buffer crosses PCIe
 * asynchronously, in pieces, while the pieces already in HBM are being screened.  Any other host memory
 * works too (staged by the runtime).  NULL when there is no device / no memory. */
void* ntedit_hip_host_alloc(size_t bytes);
void ntedit_hip_host_free(void* p);

/* Host placement (optional; the reference has no counterpart: its threads compute where the scheduler puts them).  Binds
 * the calling thread -- and the threads and first-touched pages it creates from then on -- to the CPUs of the NUMA node
 * the device hangs off (PCI bus id -> /sys/bus/pci/devices/<id>/numa_node).  A batch that crosses the socket
 * interconnect before it crosses PCIe costs the `ntedit` binary 15 % end to end on a two-socket host.  Returns the
 * node, or -1 when nothing was done (unknown topology, single node, NTEDIT_HIP_NO_BIND set). */
int ntedit_hip_bind_near_device(int device);

/* Start-up costs out of the first batch (optional; the reference's counterpart is what main() does before its
 * "reading/processing" stamp, ntedit.cpp:2589: loading the filters).  Call after the filter(s) and parameters are set:
 * sizes every grow-only device and page-locked buffer for batches of up to max_batch_bytes bytes / max_contigs contigs
 * (events_hint = expected event starts per batch, 0 = one per 400 bases; on_device = how the batches will arrive,
 * NTEDIT_HIP_BASES_*), and runs one small internal batch through the current configuration so that kernel code,
 * kernel attributes and scratch memory are in place.  Fresh device memory maps at ~40 GB/s (the 84 GB of screening
 * records of a 3 Gbp batch: two seconds); without this call the first ntedit_hip_polish_batch pays that, with it the
 * first call costs what a warm one does.  Never changes a result; may be called again when the configuration changes.
 * WHAT IT COSTS NOT TO CALL IT (measured, one MI355X): a context's first 3 Gbp batch takes ~2 s more (the record buffers
 * being mapped) and even with buffers already there its event machine runs 54-57 ms instead of 32 (kernel code objects,
 * scratch memory and workspaces set up inside the call: `[configs3]` against `[nonpow2]` in profiles/r6_gpu_tests*.log);
 * a 250 Mbp batch 22.9 ms instead of 13.4.  A caller that binds this ABI and times its first batch should call it. */
int ntedit_hip_reserve(ntedit_hip_ctx* ctx, uint64_t max_batch_bytes, uint32_t max_contigs, uint64_t events_hint, int on_device);

/* step 1 only (ntedit.cpp:1798-1807): bit i of bitmap (ceil(n/64) words,
 * host memory, or device memory when on_device) is set iff the k-mer starting
 * at byte i consists of accepted bases only and is NOT in the primary filter. */
int ntedit_hip_screen(
    ntedit_hip_ctx* ctx,
    const char* bases,
    uint64_t n,
    int on_device,
    uint64_t* bitmap);

/* steps 1-5 + makeEdit for every contig of the batch.  The result holds the
 * edit records; render it with ntedit_hip_write_outputs(). */
int ntedit_hip_polish_batch(
    ntedit_hip_ctx* ctx,
    const char* bases,
    uint64_t n,
    const uint64_t* offsets,
    const uint32_t* lens,
    uint32_t n_contigs,
    int on_device,
    ntedit_hip_result** out);
void ntedit_hip_result_free(ntedit_hip_result* r); /* (also legal after the context was destroyed) */

typedef struct ntedit_hip_stats
{
	uint64_t bases;          /* bytes screened                               */
	uint64_t absent_kmers;   /* set bits in the screening bitmap             */
	uint64_t events;         /* event threads launched                       */
	uint64_t events_deferred; /* events re-run by the sweep-only second launch */
	uint64_t events_applied; /* events that survive the serial-order filter  */
	uint64_t substitutions, insertions, deletions; /* rope/record counts     */
	float ms_screen;         /* HIP-event time of the screening launches (sum) */
	float ms_extract;        /* the run-map kernel (k_assess: -s 1, counting filters); 0 when it does not run */
	float ms_machine;        /* event machine launches (sum); overlaps screening when pipelined */
	float ms_total;          /* first kernel start -> edit records in host memory */
	uint32_t screen_launches; /* launches of the dominant screening kernel in this batch: k_bin_probe (binned
	                             screening, one per record chunk) or k_screen (direct; pipeline chunks / H2D pieces) */
	uint32_t screen_binned;   /* 1: binned pipeline (k_wc_scatter_b, k_bin_probe), 0: k_screen */
	float ms_partition;       /* binned: HIP-event time of the partition kernels (count + scan + scatter), sum */
	float ms_probe;           /* binned: HIP-event time of the k_bin_probe launches, sum */
	uint32_t events_skipped;  /* events not run because they start inside their cluster primary's run */
	uint32_t screen_chunks_direct; /* binned: record chunks whose overflow list ran out and that k_screen screened again
	                                  (a draft of very few distinct k-mers; 0 on anything like a genome) */
	uint64_t screen_overflow_records; /* binned: entries of the overflow list handed out (blocks of 256 per partition
	                                     wavefront): probes of repeated k-mers that did not fit their slice's run */
} ntedit_hip_stats;
int ntedit_hip_result_stats(const ntedit_hip_result* r, ntedit_hip_stats* s);

/* Host-side rendering of a result (replaces writeEditsToFile, ntedit.cpp:925-1213,
 * for _edited.fa and _changes.tsv; write_outputs_vcf() adds _variants.vcf).
 * bases/offsets/lens: the same batch, in HOST memory.  names[i] is the FASTA
 * header text (name + " " + comment, ntedit.cpp:2224-2229).  Files are opened
 * in append mode when append != 0; the TSV header is written by
 * ntedit_hip_write_tsv_header(). */
int ntedit_hip_write_outputs(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const char* fa_path,
    const char* tsv_path,
    int append);
int ntedit_hip_write_tsv_header(const char* tsv_path, uint32_t k, uint32_t jump, int counting);

/* _variants.vcf (ntedit.cpp:951-977, 986-1162, 1184-1208; header 2192-2211) and the -l
 * annotation map (vcf_entry_to_map, ntedit.cpp:2261-2274; plain or gzipped input).
 * write_outputs_vcf = write_outputs + the VCF body.  SNV mode (unedited positions with supported
 * alternatives are VCF-only records, ntedit.cpp:1428-1443) follows the -s flag the batch was POLISHED
 * with; the `snv` argument is kept for source compatibility and ignored.
 * annot may be NULL (every annotation reads "NA"). */
int ntedit_hip_annot_load(const char* vcf_path, ntedit_hip_annot** out);
void ntedit_hip_annot_free(ntedit_hip_annot* a);
int ntedit_hip_write_vcf_header(const char* vcf_path, const char* draft_filename);
int ntedit_hip_write_outputs_vcf(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const char* fa_path,
    const char* tsv_path,
    const char* vcf_path,
    int append,
    int snv,
    const ntedit_hip_annot* annot);

/* ---- contigs cut into segments (multi-GPU sharding of contigs larger than a GPU's share) -----------
 * The reference polishes a contig serially (kmerizeAndCorrect, ntedit.cpp:1747-2151; its only limit is
 * the 32-bit position, ntedit.cpp:1773-1774), so a single chromosome keeps one OpenMP thread busy while
 * the others idle.  Here a batch entry may be a SEGMENT [a, c) of a contig, handed over with `halo`
 * extra draft bases [c, c + halo) behind it as look-ahead room.  The serial run can be cut at c exactly
 * when it is in its clean state there (both rope cursors in the open position node, window = k untouched
 * draft bases): from then on its state is a function of the draft alone, and the next segment, polished
 * anywhere else, starts from the same state.  The caller places c inside a run of k-mers that are all in
 * the filter (ntedit_amd/dist.py: refine_cut); the library VERIFIES the cut from the edit records --
 * every applied event ended at or before c and nothing behind c was touched -- and refuses to render
 * the entry otherwise (NTEDIT_E_SEGMENT; ntedit_hip_result_cuts_ok() lets the caller check first and
 * re-run the segment joined with its successor).  Concatenating the segments' output is then byte-identical to
 * the unsplit contig's. */
#define NTEDIT_SEG_NO_HEADER 1u  /* not the first segment of its contig: no ">name" line                  */
#define NTEDIT_SEG_NO_NEWLINE 2u /* not the last segment: the sequence line stays open                    */
#define NTEDIT_SEG_SKIP 4u       /* write nothing for this entry (it was superseded by a joined re-run)    */
typedef struct ntedit_hip_segment
{
	uint32_t pos_offset; /* contig position of the entry's first base: added to every reported position */
	uint32_t halo;       /* trailing bases of the entry that belong to the next segment (not rendered) */
	uint32_t flags;      /* NTEDIT_SEG_* */
	uint32_t reserved;
} ntedit_hip_segment;

/* where the serial run of every entry's last applied event ended (entry-relative position; 0 = the entry
 * has no applied event).  A segment with a halo is valid iff cover_end <= lens[i] - halo. */
int ntedit_hip_result_cover_ends(const ntedit_hip_result* r, uint32_t n_contigs, uint32_t* cover_ends);
/* ok[i] = 1 iff write_outputs_ex() will accept entry i with segments[i] (the renderer's own predicate, evaluated
 * from the edit records without rendering: the last applied event ended at or before the cut, the rope was not
 * terminated and ends in the open position node, which starts in front of the cut).  Check BEFORE writing: an entry
 * that fails is polished again joined with its successor. */
int ntedit_hip_result_cuts_ok(const ntedit_hip_result* r, uint32_t n_contigs, const uint32_t* lens, const ntedit_hip_segment* segments, uint8_t* ok);

/* ---- edit records (the reference's per-contig rope + substitution queue, sRec / seqNode,
 * ntedit.cpp:599-620, flattened the way writeEditsToFile walks them, ntedit.cpp:936-1212) -------------
 * One record per _changes.tsv row, in file order; in SNV mode (-s 1) positions that keep their base but
 * have supported alternatives (VCF-only records) come as NTEDIT_EDIT_SNV_KEPT. */
#define NTEDIT_EDIT_SUB 1
#define NTEDIT_EDIT_INS 2
#define NTEDIT_EDIT_DEL 3
#define NTEDIT_EDIT_SNV_KEPT 4
typedef struct ntedit_hip_edit
{
	uint32_t contig;     /* entry index in the batch                                                      */
	uint32_t draft_pos;  /* 0-based draft position: SUB the base; INS the base the insertion precedes;
	                        DEL the first deleted base.  TSV column 2 = draft_pos + 1 (SUB) / draft_pos     */
	uint32_t bases_off;  /* INS / DEL: offset of the inserted / deleted bases in the pool                   */
	uint16_t len;        /* INS / DEL: number of bases; SUB: 1                                              */
	uint16_t support;    /* k-mers supporting the edit (TSV column 5)                                       */
	uint8_t kind;        /* NTEDIT_EDIT_*                                                                   */
	uint8_t draft_base;  /* TSV "OriginalBase"                                                              */
	uint8_t new_base;    /* SUB: the replacement                                                            */
	uint8_t n_alt;       /* SUB: alternate bases with support > 0                                           */
	uint8_t alt_base[3];
	uint8_t alt_support[3];
	uint8_t reserved[2];
} ntedit_hip_edit;
/* Builds (once, cached in the result) and returns the records of the whole batch.  bases/offsets/lens:
 * the batch in HOST memory, segments: NULL or the descriptors the batch will be rendered with.  The
 * pointers stay valid until ntedit_hip_result_free(). */
int ntedit_hip_result_edits(
    ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    uint32_t n_contigs,
    const ntedit_hip_segment* segments,
    const ntedit_hip_edit** edits,
    uint64_t* n_edits,
    const char** base_pool);

/* write_outputs with everything optional in one block.  SNV mode is taken from the parameters the batch
 * was polished with. */
typedef struct ntedit_hip_write_options
{
	const char* fa_path;  /* NULL: skip that stream */
	const char* tsv_path;
	const char* vcf_path;
	int append;
	const ntedit_hip_annot* annot;      /* -l map or NULL */
	const ntedit_hip_segment* segments; /* NULL, or one descriptor per entry */
	uint64_t* out_sizes;                /* NULL, or 3 * n_contigs: bytes every entry appended to fa / tsv / vcf
	                                       (the index the multi-GPU gather merges by) */
} ntedit_hip_write_options;
int ntedit_hip_write_outputs_ex(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const ntedit_hip_write_options* opt);

/* Host threads used by write_outputs() to render contigs concurrently (the reference's -t;
 * output order and bytes do not depend on it).  0 = default (up to 8).  Process-wide.
 * A result may be rendered and freed on another thread than the one that runs
 * polish_batch() on the same context. */
void ntedit_hip_set_host_threads(unsigned n);

/* timings of the last screen()/filter_insert() call (HIP events, ms) */
float ntedit_hip_last_kernel_ms(const ntedit_hip_ctx* ctx);

/* random 1-byte gather micro-benchmark over a filter-sized buffer: the
 * "HBM random-read roofline" denominator of SURVEY.md 8(d).  Returns probes/s. */
int ntedit_hip_gather_bench(ntedit_hip_ctx* ctx, uint64_t nbytes, uint64_t n_probes, double* probes_per_s, float* ms);

/* ---- draft ingest (replaces kseq as used by readAndCorrect, ntedit.cpp:2213-2234; lib/kseq.h:176-215) ------------
 * Reads a whole FASTA / FASTQ draft (plain, gzip or BGZF -- told apart by their magic bytes) with the host binary's
 * readers and keeps the records with >= min_len bases (-z, ntedit.cpp:2242) as ONE buffer in the batch layout of
 * ntedit_hip_polish_batch: every sequence followed by '\n'.  header = name [+ " " + comment] (ntedit.cpp:2224-2229).
 * err (may be NULL) receives a message when the file cannot be opened or turns out to be corrupt / truncated
 * half-way (NTEDIT_E_IO; kseq would stop silently).  threads 0 = default. */
typedef struct ntedit_hip_fasta ntedit_hip_fasta;
int ntedit_hip_fasta_load(const char* path, uint64_t min_len, unsigned threads, ntedit_hip_fasta** out, char* err, size_t errcap);
/* The same records WITHOUT their bases: the file is mapped and indexed (headers, lengths), sequences are read on demand with
 * ntedit_hip_fasta_read -- what a rank of a multi-GPU run needs to plan the partition and then read its own share
 * (python -m ntedit_amd.run).  ntedit_hip_fasta_record() then reports offset = ~0 and ntedit_hip_fasta_blob() nothing.  Inputs
 * the mapped reader does not take (single-stream gzip, FASTQ, ...) are loaded whole; the calls behave the same. */
int ntedit_hip_fasta_open(const char* path, uint64_t min_len, unsigned threads, ntedit_hip_fasta** out, char* err, size_t errcap);
int ntedit_hip_fasta_read(const ntedit_hip_fasta* f, uint64_t i, uint64_t start, uint64_t n, char* dst);
uint64_t ntedit_hip_fasta_count(const ntedit_hip_fasta* f);
const char* ntedit_hip_fasta_blob(const ntedit_hip_fasta* f, uint64_t* nbytes);
int ntedit_hip_fasta_record(const ntedit_hip_fasta* f, uint64_t i, const char** header, uint64_t* header_len, uint64_t* offset, uint64_t* len);
void ntedit_hip_fasta_free(ntedit_hip_fasta* f);

/* Test and tuning knobs (not part of the reference surface).  NONE of them can change a result: they pick between
 * implementations that are bit-identical by construction (and tested to be), split work differently, or print
 * timings.  Keys:
 *   screening   "screen_mode" (overrides params.screen_mode), "bin_chunk" (k-mer starts per record chunk of the
 *               partitioned screening), "bin_cap_percent" (record-run capacity in percent of the expectation: forces the
 *               overflow list), "bin_ovf_cap" (entries of the overflow list: forces a list that runs out, i.e. record chunks
 *               screened again by the direct kernel), "bin_fallback" (1: the direct kernel, like "screen_mode" 1), "bin_scatter"
 *               (1: the barrier-free partition kernel, kept as the second implementation the tests compare; 1024 slices at
 *               most), "bin_slice_log2" (log2 of the slots of a filter slice instead of 2 MiB's, doubled until the partition
 *               kernel has rings for every slice: many slices of a small filter), "bin_ring" (the default partition kernel:
 *               8 = its 2048-slice layout with rings of 8 slots whatever the number of slices, 16 = only its 1024-slice layout),
 *               "bin_wide_min_run" (records a (slice, workgroup) pair must expect before a filter is cut into more than 1024
 *               slices; 0: 4096),
 *               "force_xcc" (x + 1: the probe stage behaves as if every wavefront ran on XCD x), "bin_timing",
 *               "candmap" (1: with -s 1 on a plain filter the first probes of every position's substitution candidates go
 *               through the partitioned pipeline before k_assess; exact, measured slower, off), "h2d_fixed_schedule" (1: a
 *               host batch is screened in round 3's fixed chunk schedule instead of chunks sized by arrival)
 *   batches     "chunk_bytes" (pipeline chunk size), "h2d_piece" (bytes per host-to-device piece)
 *   machine     "inline_tries", "no_rounds", "force_rounds", "no_early_copy", "lanes" (runs of failing positions one
 *               position per lane: 0 off, 1 in the clean state, 2 also behind substitutions), "defer_fail" (failing positions after which the thread-per-event launch hands an event
 *               over; "defer_fail_snv": the same with -s 1, measured slower, 0), "snv_wave" (1: the events of -s 1 go to the
 *               wavefront-per-event launch; measured slower), "defer_run" (hand-over
 *               threshold of the thread-per-event launch), "assess" (the run map: 0 never, 1 always; default: with -s 1
 *               and counting filters), "machine_cfg" (0: the general instantiation of the machine kernels),
 *               "settle" (k_settle in front of the thread-per-event launch: 0 never, 1 wherever it applies; default: see
 *               ntedit_hip_settle_info),
 *               "arena_chunks" (test-only: chunks of the edit-record arena in a batch's first attempt, so that a test
 *               can make it run out and reach the retry with four times as much)
 * (The measured-and-rejected variants of round 3 -- record chunks partitioned while the previous one is probed, slices
 * probed in parts, uncached records, event rounds in pieces, a batch polished in pipeline chunks as it arrives -- are
 * gone from the library; DESIGN.md 8 keeps their numbers, the history their code.)
 * The library reads two environment variables only: NTEDIT_HIP_DEBUG (diagnostics on stderr) and
 * NTEDIT_HIP_NO_BIND (see ntedit_hip_bind_near_device). */
int ntedit_hip_set_tuning(ntedit_hip_ctx* ctx, const char* key, uint64_t value);

/* k_settle: in the configurations it restates the machine for (plain primary filter, no secondary one, no -s 1, -m 0
 * without -a, k <= 64) the plain substitution events of a batch -- one wrong base in clean sequence -- are settled by a
 * kernel of their own in front of the event machine's thread-per-event launch, which runs the rest.  For the context's
 * last polish call: the events those launches were handed, the events k_settle settled, and its time (HIP events on
 * its stream).  All zero where it did not run.  Tuning key "settle". */
typedef struct ntedit_hip_settle_stats
{
	uint64_t events_seen;
	uint64_t events_settled;
	float ms;
} ntedit_hip_settle_stats;
int ntedit_hip_settle_info(ntedit_hip_ctx* ctx, ntedit_hip_settle_stats* st);

/* ---- the edited draft in HBM, and the k-mer QV of a polish (no counterpart in the reference) -----------------
 * The device applier turns a batch's result into the edited contigs in device memory: for every entry exactly the bytes
 * ntedit_hip_write_outputs() puts between the header line and the closing newline of _edited.fa, entry after entry with
 * one separator byte ('\n') behind each -- the layout of an input batch, so the buffer can be screened or polished as it
 * stands.  Segments (ntedit_hip_segment) are not supported: the call takes none.
 * ntedit_hip_set_apply(ctx, flags), for the polish calls that follow:
 *   0                          the default: nothing of this runs
 *   NTEDIT_HIP_APPLY_EDITED    the applier runs inside ntedit_hip_polish_batch, behind the collection of the edit records;
 *                              the result owns the edited bases until ntedit_hip_result_free()
 *   NTEDIT_HIP_APPLY_QV        the applier runs, the edited bases are screened against the primary filter the batch was
 *                              polished with, and per entry the k-mer starts and the absent k-mers are counted before and
 *                              after (ntedit_hip_result_qv); the edited bases go with the call unless APPLY_EDITED is set too
 * A malformed arena fails the polish call with NTEDIT_E_INTERNAL (the message names the renderer's code). */
#define NTEDIT_HIP_APPLY_EDITED 1u
#define NTEDIT_HIP_APPLY_QV 2u
int ntedit_hip_set_apply(ntedit_hip_ctx* ctx, uint32_t flags);
/* The edited bases of a result polished with APPLY_EDITED (NTEDIT_E_ARG otherwise; ntedit_hip_result_last_error() says
 * why).  *dev_ptr: device memory, 16-byte aligned, valid until ntedit_hip_result_free(); *n_bytes: its bytes, separators
 * included; offsets_out / lens_out (n_contigs each, may be NULL): entry i is dev_ptr[offsets_out[i] .. + lens_out[i]). */
int ntedit_hip_result_edited_device(const ntedit_hip_result* r, const char** dev_ptr, uint64_t* n_bytes, uint64_t* offsets_out, uint32_t* lens_out,
                                    uint32_t n_contigs);
/* the same with a download into host_buf[0 .. cap); *n_bytes = bytes needed (NTEDIT_E_OVERFLOW when cap is less) */
int ntedit_hip_result_edited(const ntedit_hip_result* r, char* host_buf, uint64_t cap, uint64_t* n_bytes, uint64_t* offsets_out, uint32_t* lens_out,
                             uint32_t n_contigs);
const char* ntedit_hip_result_last_error(void);

/* One row per entry of a batch polished with APPLY_QV.  kmers: the k-mer starts inside the entry whose k bytes are all
 * A, C, G or T, in either case -- the k-mers a read set can hold.  absent: the set bits of ntedit_hip_screen's bitmap
 * among the entry's starts [offset, offset + len - k + 1): not in the primary filter; a counting filter: below the -p
 * threshold.  (The screening hashes k-mers that hold another IUPAC code too, with zero seeds: such a k-mer is practically
 * always absent and no k-mer of `kmers`.  On a draft of A, C, G, T and N the two definitions are one.)  With -s 1 step 1
 * marks every k-mer, so both screenings run again without it: the counts are those of -s 0.
 * before: the entry as it came, after: as edited. */
typedef struct ntedit_hip_qv_row
{
	uint64_t len_before, len_after;
	uint64_t kmers_before, absent_before;
	uint64_t kmers_after, absent_after;
} ntedit_hip_qv_row;
int ntedit_hip_result_qv(const ntedit_hip_result* r, ntedit_hip_qv_row* rows, uint32_t n_contigs);
/* Merqury's consensus QV from those counts, -10 log10(1 - (1 - absent / kmers)^(1 / k)): +inf for absent == 0, NaN for
 * kmers == 0, 0 for absent >= kmers.  Host arithmetic in double; the only place the formula lives. */
double ntedit_hip_qv_value(uint64_t absent, uint64_t kmers, uint32_t k);
/* <prefix>_qv.tsv as the front ends write it: the header line, and one line per row -- name, len_before, len_after,
 * kmers_before, absent_before, qv_before, kmers_after, absent_after, qv_after; QVs with two decimals, "inf" and "NA" for
 * the two special cases.  The last row, "#total", holds the sums. */
const char* ntedit_hip_qv_header(void);
int ntedit_hip_qv_format_row(const char* name, const ntedit_hip_qv_row* row, uint32_t k, char* out, uint64_t cap);

/* The context's last polish call with an apply flag: HIP-event times of the applier's kernels, of the screening of the
 * edited bases and of the count kernel (both passes), the pieces and bytes the applier wrote, the events it applied. */
typedef struct ntedit_hip_apply_stats
{
	float ms_apply, ms_screen, ms_count;
	uint64_t pieces, bytes, events_applied;
} ntedit_hip_apply_stats;
int ntedit_hip_apply_info(ntedit_hip_ctx* ctx, ntedit_hip_apply_stats* st);
/* output bytes per workgroup of the applier's copy kernel (tests place edits on both sides of a tile's edge) */
uint32_t ntedit_hip_apply_tile(void);

/* ---- k-mer completeness of a polish: the draft's distinct k-mers that the filter holds (no counterpart in the reference)
 * Linear counting on the device.  R is the PRIMARY filter, plain, of 8 x bytes bits and h hashes.  A k-mer
 * is k bytes of ACGTacgt inside one entry (the `kmers` of ntedit_hip_qv_row); it is present iff its bit in the screening's
 * absent bitmap is clear (-s 0 semantics: all its h bits are set in R).  Two mark arrays of R's byte size, M[0] (before) and
 * M[1] (after), start zeroed; marking a present k-mer sets bit filter_slot(R, fh + rh) -- its first probe into R -- of
 * M[which].  Marking is an OR: M[which] is a function of the SET of present k-mers marked since the last reset, whatever the
 * batches, their order or the launch geometry.
 * NTEDIT_HIP_APPLY_SHARED (ntedit_hip_set_apply, beside EDITED and QV): ntedit_hip_polish_batch does everything APPLY_QV
 * does (ntedit_hip_result_qv still answers only with APPLY_QV), begins the marks if that was not done, and marks the batch
 * into M[0] and the edited bases into M[1].
 * The marks belong to the PRIMARY filter they were sized for: every call that gives the slot another filter or releases it
 * (ntedit_hip_set_filter*, _load_filter_file, _filter_alloc*, the reads and genome builds that allocate PRIMARY) releases
 * them too; ntedit_hip_destroy frees them.  A counting PRIMARY filter: NTEDIT_E_UNSUPPORTED (its "present" is a threshold
 * on counters, its slots are no bits); no PRIMARY filter: NTEDIT_E_ARG.  A secondary filter plays no part. */
#define NTEDIT_HIP_APPLY_SHARED 4u
int ntedit_hip_shared_begin(ntedit_hip_ctx* ctx); /* allocate + zero M[0], M[1] for the current PRIMARY filter; idempotent */
int ntedit_hip_shared_reset(ntedit_hip_ctx* ctx); /* zero both, and the counters of ntedit_hip_shared_counts */
void ntedit_hip_shared_free(ntedit_hip_ctx* ctx);
/* stand-alone: screens `bases` (a batch: entries + separators; host or device bytes) against PRIMARY the way a batch of
 * that size is screened, with -s 0 semantics, then marks its present k-mers into M[which] (begins the marks if need be) */
int ntedit_hip_shared_mark(ntedit_hip_ctx* ctx, int which, const char* bases, uint64_t n, int on_device);
int ntedit_hip_shared_download(ntedit_hip_ctx* ctx, int which, uint8_t* bits); /* R's byte size */
typedef struct ntedit_hip_shared_stats
{
	uint64_t bits;
	uint32_t hash_num, k;
	uint64_t filter_set, shared_set[2]; /* popcounts: R, M[0], M[1] */
	uint64_t marked_calls;              /* kernel launches since the last reset */
	float ms_mark[2];                   /* HIP-event time of k_mark, summed since the last reset */
} ntedit_hip_shared_stats;
int ntedit_hip_shared_counts(ntedit_hip_ctx* ctx, ntedit_hip_shared_stats* st); /* NTEDIT_E_ARG while there are no marks */
/* Distinct keys behind `set` occupied slots of `slots`, h slots per key: -(slots / h) * log1p(-set / slots); 0 for set == 0,
 * +inf for set >= slots, NaN for slots == 0 or h == 0.  shared_kmers = (M's popcount, bits, 1), filter_kmers = (R's popcount,
 * bits, h), completeness = their ratio (not clipped at 1).  Host arithmetic in double; the only place the formula lives. */
double ntedit_hip_bloom_cardinality(uint64_t set, uint64_t slots, uint32_t h);
/* <prefix>_completeness.tsv as the front ends write it: the header line, and one line per stage ("before", "after") --
 * stage, filter_bits, filter_set, filter_kmers, shared_set, shared_kmers, completeness; estimates rounded to integers, the
 * completeness a fraction with six decimals, "NA" where a value is not finite. */
const char* ntedit_hip_completeness_header(void);
int ntedit_hip_completeness_format_row(const char* stage, const ntedit_hip_shared_stats* st, int which, char* out, uint64_t cap);

/* ---- the edited draft as BGZF, compressed on the device (no counterpart in the reference) ----------------
 * BGZF (the SAM specification, section 4.1) is a series of gzip members of at most 64 KiB, each with an extra subfield
 * 'B','C' that holds the member's size - 1; a file ends in the 28-byte member of no bytes (ntedit_hip_bgzf_eof).  The
 * writer cuts its input into blocks of 65,280 bytes and makes one member of each: one final DEFLATE block of literals
 * under a dynamic Huffman code limited to 15 bits (no matches: a draft is four letters, which such a code holds at a
 * little over two bits a base), or a stored block where that is not smaller.  A member is a function of its block's
 * bytes alone: the device and the serial host model give the same bytes.  gzip, bgzip, zlib and this library's own
 * readers (ntedit_hip_fasta_*, ntedit_hip_reads_inflate_*) read the result; its bytes are not those bgzip would write.
 *
 * NTEDIT_HIP_APPLY_BGZF (ntedit_hip_set_apply, beside the other flags): the applier runs, and behind it, on the same
 * stream, the _edited.fa text of the batch is laid out in device memory -- for entry i '>' names[i] '\n', the edited
 * bases, '\n': byte for byte what ntedit_hip_write_outputs_ex() appends to fa_path for the batch -- and compressed;
 * only the members cross to the host, into page-locked memory the result owns.  The edited bases go with the call
 * unless APPLY_EDITED is set too.  Segments (ntedit_hip_segment) are not supported.
 * ntedit_hip_set_fa_names copies the header lines (without '>' and newline) for the NEXT polish call; a polish call with
 * the flag and without names, or with another number of names than entries, fails with NTEDIT_E_ARG before anything
 * runs and leaves the names set.  A call whose arguments are accepted uses the names up, whatever becomes of it. */
#define NTEDIT_HIP_APPLY_BGZF 8u
int ntedit_hip_set_fa_names(ntedit_hip_ctx* ctx, const char* const* names, uint32_t n);
/* The members of a result polished with APPLY_BGZF (NTEDIT_E_ARG otherwise; ntedit_hip_result_last_error() says why).
 * *host: *n_bytes bytes, valid until ntedit_hip_result_free(); *n_plain: the bytes they inflate to; *n_members: their
 * number (0 members and 0 bytes for an empty batch).  The outputs may be NULL. */
int ntedit_hip_result_fa_bgzf(const ntedit_hip_result* r, const uint8_t** host, uint64_t* n_bytes, uint64_t* n_plain, uint32_t* n_members);
/* Stand-alone: src[0 .. n) (host bytes, or device bytes with on_device = NTEDIT_HIP_BASES_DEVICE) into members in
 * out[0 .. cap), host memory.  *n_out = the bytes needed; NTEDIT_E_OVERFLOW when cap is less.  n == 0 gives 0 bytes
 * (no EOF member: the caller ends a file with ntedit_hip_bgzf_eof). */
int ntedit_hip_bgzf_deflate(ntedit_hip_ctx* ctx, const void* src, uint64_t n, int on_device, uint8_t* out, uint64_t cap, uint64_t* n_out);
/* the serial host model of the same encoder: no context, no device; arguments and codes as above */
int ntedit_hip_bgzf_deflate_model(const void* src, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* n_out);
/* no n bytes take more: every block as a stored member */
uint64_t ntedit_hip_bgzf_bound(uint64_t n);
/* the member that ends a BGZF file; *n (may be NULL) = 28 */
const uint8_t* ntedit_hip_bgzf_eof(uint32_t* n);
/* The context's last call that compressed (a polish call with APPLY_BGZF, ntedit_hip_bgzf_deflate): HIP-event times of
 * the image kernel, of the deflate and scan kernels, and of the packing kernel with the copy to the host; the bytes in
 * and out, the members, and those among them that hold a stored block. */
typedef struct ntedit_hip_bgzf_stats
{
	float ms_image, ms_deflate, ms_copy;
	uint64_t plain_bytes, bgzf_bytes;
	uint32_t members, stored_members;
} ntedit_hip_bgzf_stats;
int ntedit_hip_bgzf_info(ntedit_hip_ctx* ctx, ntedit_hip_bgzf_stats* st);

/* ---- the unsupported regions of a polish as intervals (no counterpart in the reference) -----------------
 * Where the QV rows say how many k-mers of an entry the filter does not hold, the track says where they lie.  A batch has n
 * positions and entries e in batch order, entry e at [offs[e], offs[e] + lens[e]); entries do not overlap and may abut.  An
 * absent bitmap has one bit per k-mer start: position p is bit p % 64 of word p / 64 (ntedit_hip_screen's layout).
 *   A position p is a MARKED START of entry e iff its bit is set and offs[e] <= p < offs[e] + lens[e] - k + 1 -- the starts
 *   ntedit_hip_qv_row counts as absent.  Bits anywhere else are ignored: separators, the last k - 1 positions of an entry,
 *   padding behind n, entries shorter than k.
 *   An INTERVAL of entry e is a maximal sequence of its marked starts p1 < ... < pm in which consecutive starts are at most
 *   k apart: what `bedtools merge` makes of the k-mers' spans [p, p + k), overlapping and book-ended spans joined.  An
 *   interval never continues into another entry, whatever the gap.
 *   Its record: entry = e, begin = p1 - offs[e], end = pm - offs[e] + k, absent = m.  Records are ordered by entry, then by
 *   begin.  Per entry the absent counts sum to the QV row's absent count; end - begin sums to the unsupported bases.
 * NTEDIT_HIP_APPLY_TRACK (ntedit_hip_set_apply, beside the other flags): ntedit_hip_polish_batch does everything APPLY_QV
 * does (ntedit_hip_result_qv still answers only with APPLY_QV; the same limits: k, no segments) and extracts the intervals
 * of both bitmaps: before, in the batch's coordinates; after, in those of the edited entries. */
#define NTEDIT_HIP_APPLY_TRACK 16u
typedef struct ntedit_hip_track_interval
{
	uint32_t entry, begin, end, absent;
} ntedit_hip_track_interval;
/* The intervals of a result polished with APPLY_TRACK (NTEDIT_E_ARG otherwise; ntedit_hip_result_last_error() says why).
 * which: 0 before, 1 after.  *n = their number; they are copied into out[0 .. cap) (NTEDIT_E_OVERFLOW when cap is less,
 * with *n set).  The result keeps them in host memory of its own until ntedit_hip_result_free(). */
int ntedit_hip_result_track(const ntedit_hip_result* r, int which, ntedit_hip_track_interval* out, uint64_t cap, uint64_t* n);
/* Stand-alone: the intervals of any bitmap.  bitmap: ceil(n_positions / 64) words; offs, lens: n_entries entries as above,
 * inside [0, n_positions); all host arrays, copied in and out by the call.  k: 1 .. 1024.  *n = the number of intervals;
 * NTEDIT_E_OVERFLOW when cap is less. */
int ntedit_hip_track_extract(ntedit_hip_ctx* ctx, const uint64_t* bitmap, uint64_t n_positions, const uint64_t* offs, const uint32_t* lens,
                             uint32_t n_entries, uint32_t k, ntedit_hip_track_interval* out, uint64_t cap, uint64_t* n);
/* The context's last call that extracted (a polish call with APPLY_TRACK: [0] before, [1] after; ntedit_hip_track_extract:
 * [0], and [1] zero): HIP-event time of the extraction's kernels, the intervals, the bases they cover. */
typedef struct ntedit_hip_track_stats
{
	float ms[2];
	uint64_t intervals[2];
	uint64_t bases[2];
} ntedit_hip_track_stats;
int ntedit_hip_track_info(ntedit_hip_ctx* ctx, ntedit_hip_track_stats* st);
/* One BED row, "name<TAB>begin<TAB>end<TAB>absent\n"; name is cut at its first space or tab (the sequence name as faidx
 * and IGV understand it).  Host only: no context, no device. */
int ntedit_hip_track_format_row(const char* name, const ntedit_hip_track_interval* iv, char* out, uint64_t cap);

/* ---- the k-mer multiplicity spectrum of a polish (no counterpart in the reference) ----------------------
 * How often the reads hold the draft's k-mers, before and after, from a COUNTING filter.
 *   F is the context's PRIMARY filter: a counting filter of `bits` 8-bit counters and h hashes (1 .. 8).
 *   A K-MER is k bytes of ACGTacgt inside one entry -- exactly the `kmers` of ntedit_hip_qv_row; a window that holds N,
 *   another IUPAC code, a separator or padding, or that leaves its entry, is none.
 *   Its MULTIPLICITY is m = min over i < h of F.data[slot_i], slot_i the i-th probe of its canonical ntHash: the value -p
 *   and the event machine see.  0 .. 255, and 255 means "255 or more": the counters saturate.
 *   The SPECTRUM of a batch is bins[256], 64-bit: bins[c] = the k-mer OCCURRENCES with m = c (not distinct k-mers).
 *   The DEPTH ROW of entry e: kmers, its occurrences; sum, the sum of their m; saturated, those with m = 255.
 *   BEFORE is the batch as it came, AFTER the edited entries (the applier's buffer).  -p, -q, -s and the secondary filter
 *   play no part; no absent bitmap is read.
 * So sum(bins) = sum of kmers; kmers = the QV row's kmers_before / kmers_after; sum of sum = sum of c * bins[c]; sum of
 * saturated = bins[255]; and on a draft of A, C, G, T, N only, sum(bins[0 .. max(1, p))) = the QV rows' absent counts.
 * ntedit_hip_set_spectrum(ctx, on): a switch of its own beside ntedit_hip_set_apply's flags, for the polish calls that
 * follow.  ON: ntedit_hip_polish_batch runs the applier whatever the flags (the edited bases go with the call unless
 * APPLY_EDITED is set too) and counts both spectra; it fails before anything is polished with NTEDIT_E_UNSUPPORTED when
 * the PRIMARY filter is plain and NTEDIT_E_ARG when there is none.  Segments (ntedit_hip_segment) are not supported: the
 * call takes none.  OFF (the default): nothing runs.  ntedit_hip_reserve's warm-up batch leaves no trace in any figure. */
int ntedit_hip_set_spectrum(ntedit_hip_ctx* ctx, int on);
typedef struct ntedit_hip_depth_row
{
	uint64_t kmers_before, sum_before, saturated_before;
	uint64_t kmers_after, sum_after, saturated_after;
} ntedit_hip_depth_row;
/* The spectrum (which: 0 before, 1 after) and the depth rows of a result polished with the switch on (NTEDIT_E_ARG
 * otherwise; ntedit_hip_result_last_error() names ntedit_hip_set_spectrum).  The result keeps them in host memory of its
 * own until ntedit_hip_result_free(). */
int ntedit_hip_result_spectrum(const ntedit_hip_result* r, int which, uint64_t bins[256]);
int ntedit_hip_result_depth(const ntedit_hip_result* r, ntedit_hip_depth_row* rows, uint32_t n_contigs);
/* Stand-alone: the spectrum of any batch against the PRIMARY counting filter.  bases: n bytes, host (on_device 0) or
 * device (1, 16-byte aligned); offs, lens: n_entries entries in batch order, host arrays; entries do not overlap and may
 * abut.  bins: 256 words; rows: three words per entry {kmers, sum, saturated}, or NULL.  n == 0 or n_entries == 0 gives
 * zeros. */
int ntedit_hip_spectrum_count(ntedit_hip_ctx* ctx, const char* bases, uint64_t n, int on_device, const uint64_t* offs, const uint32_t* lens,
                              uint32_t n_entries, uint64_t* bins, uint64_t* rows);
/* The context's last call that counted (a polish call with the switch on: [0] before, [1] after; ntedit_hip_spectrum_count:
 * [0], and [1] zero): HIP-event time of the k_spectrum launch, the k-mers it counted. */
typedef struct ntedit_hip_spectrum_stats
{
	float ms[2];
	uint64_t kmers[2];
} ntedit_hip_spectrum_stats;
int ntedit_hip_spectrum_info(ntedit_hip_ctx* ctx, ntedit_hip_spectrum_stats* st);
/* <prefix>_spectrum.tsv: "multiplicity<TAB>before<TAB>after\n" and one row per multiplicity 0 .. 255.
 * <prefix>_depth.tsv: name (cut at its first space or tab), kmers_before, mean_before, saturated_before, kmers_after,
 * mean_after, saturated_after; mean = sum / kmers with two decimals, "NA" when kmers is 0 -- a saturated counter counts as
 * 255, so the mean is a lower bound.  A last row "#total" (the caller's sum of the rows) closes the table.  Host only: no
 * context, no device; NTEDIT_E_OVERFLOW when the row does not fit out[0 .. cap). */
const char* ntedit_hip_spectrum_header(void);
int ntedit_hip_spectrum_format_row(uint32_t multiplicity, uint64_t before, uint64_t after, char* out, uint64_t cap);
const char* ntedit_hip_depth_header(void);
int ntedit_hip_depth_format_row(const char* name, const ntedit_hip_depth_row* row, char* out, uint64_t cap);

/* ---- the spectrum split by assembly copy number (Merqury's spectra-cn; no counterpart in the reference) --
 * The spectrum above, split by how many times the ASSEMBLY holds each k-mer.
 *   F, a K-MER and its MULTIPLICITY m are as above.  A SIDE is `before` (0: every batch as it came) or `after` (1: every
 *   batch's edited entries), accumulated over all calls since the last reset: copy number is a property of the whole draft,
 *   so the bytes of both sides stay in device memory (the DRAFT STORE) until ntedit_hip_cn_finish.
 *   For one side, the SKETCH S has `counters` 8-bit counters, a power of two.  It uses the filter's h and the filter's hash
 *   values: every k-mer occurrence of the side adds 1 to all h counters S[hv_i & (counters - 1)], saturating at 255 -- plain
 *   count-min, the same whatever the batching or order.  The COPY NUMBER cn(x) = min_i S[slot_i(x)], 1 .. 255; 255 means "255
 *   or more"; it is never below the true count.  The CLASS c = min(cn, 5): 1, 2, 3, 4, 5plus.
 *   occ[c - 1][m]: the k-mer occurrences of class c with multiplicity m.  w5[m]: the sum of RECIP[cn] over the class-5
 *   occurrences with multiplicity m, RECIP[cn] = (2^32 + cn / 2) / cn in integer arithmetic, cn = 5 .. 255.
 *   A ROW per entry, in the order the entries were appended: kmers and the five class counts of its occurrences.
 *   DISTINCT k-mers (host): distinct[c - 1][m] = (occ[c - 1][m] + c / 2) / c for c = 1 .. 4, distinct[4][m] = (w5[m] + 2^31)
 *   >> 32.
 * So sum over c of occ[c][m] = the spectrum's bins[m] of that side; a row's five classes sum to its kmers = the depth row's
 * kmers; the rows' class counts sum to sum over m of occ[c][m]; and without sketch collisions occ[c - 1][m] is a multiple of c.
 * There is no "read-only" row (a filter cannot be enumerated; --completeness gives that total for plain filters), and copy
 * numbers are count-min estimates: the expected inflated share is (nonzero counters / counters)^h.  h = 1 gives a poor sketch.
 * ntedit_hip_set_cn(ctx, on, store_cap_bytes): a switch of its own, as ntedit_hip_set_spectrum is.  ON: the store begins
 * empty with that cap on the bytes of both sides together; ntedit_hip_polish_batch runs the applier whatever the flags and
 * appends both sides (device-to-device copies), and refuses as ntedit_hip_set_spectrum does before anything is polished:
 * NTEDIT_E_UNSUPPORTED on a plain PRIMARY filter, NTEDIT_E_ARG without one.  A batch that would pass the cap, or an
 * allocation that fails, releases the whole store (NTEDIT_CN_OVER_CAP / NTEDIT_CN_NO_MEMORY) and fails nothing: the polish
 * goes on.  Another PRIMARY filter empties the store (every round of a cascade starts clean); ntedit_hip_reserve's warm-up
 * batch leaves nothing in it.  OFF (the default): nothing runs, the store is released. */
#define NTEDIT_CN_OFF 0
#define NTEDIT_CN_ON 1
#define NTEDIT_CN_OVER_CAP 2
#define NTEDIT_CN_NO_MEMORY 3
#define NTEDIT_CN_STORE_DEFAULT (32ull << 30)
#define NTEDIT_CN_SKETCH_MIN (1ull << 20)
#define NTEDIT_CN_SKETCH_MAX (1ull << 36)
#define NTEDIT_CN_SKETCH_FLOOR (1ull << 6) /* what the library itself takes: a sketch this small is all collisions (the tests' way to force them) */
int ntedit_hip_set_cn(ntedit_hip_ctx* ctx, int on, uint64_t store_cap_bytes);
/* Stand-alone: one batch to side `which`.  bases: n bytes, host (on_device 0) or device (1); offs, lens: n_entries entries
 * in batch order, host arrays; entries do not overlap and may abut.  NTEDIT_E_ARG while the switch is off. */
int ntedit_hip_cn_append(ntedit_hip_ctx* ctx, int which, const char* bases, uint64_t n, int on_device, const uint64_t* offs, const uint32_t* lens,
                         uint32_t n_entries);
/* Both sides from the store: per side the sketch zeroed, k_cn_count over every stored batch, the non-zero counters,
 * k_spectrum_cn over every stored batch; then one copy to the host.  The store stays as it is.  sketch_counters = 0: the
 * smallest power of two at or above 8 times the larger side's stored bytes, within [2^20, 2^36]; anything else must be a
 * power of two (NTEDIT_E_ARG) -- in that range for any use (`ntedit --cn_sketch` takes no other); the call itself also
 * takes the sizes from NTEDIT_CN_SKETCH_FLOOR up to 2^20, where most copy numbers are inflated, so that a test can force
 * collisions.  NTEDIT_E_OVERFLOW with a one-line message when the store was released. */
int ntedit_hip_cn_finish(ntedit_hip_ctx* ctx, uint64_t sketch_counters);
/* The raw results of one side after ntedit_hip_cn_finish (NTEDIT_E_ARG before it): occ[5][256], w5[256]. */
int ntedit_hip_cn_table(ntedit_hip_ctx* ctx, int which, uint64_t* occ, uint64_t* w5);
typedef struct ntedit_hip_cn_row
{
	uint64_t kmers, cn1, cn2, cn3, cn4, cn5plus;
} ntedit_hip_cn_row;
/* The rows of one side, n = the entries appended to it (NTEDIT_E_ARG otherwise, and before ntedit_hip_cn_finish). */
int ntedit_hip_cn_rows(ntedit_hip_ctx* ctx, int which, ntedit_hip_cn_row* rows, uint64_t n);
/* distinct[5][256] from occ[5][256] and w5[256].  Host only: no context, no device. */
int ntedit_hip_cn_distinct(const uint64_t* occ, const uint64_t* w5, uint64_t* distinct);
typedef struct ntedit_hip_cn_stats
{
	uint32_t state;      /* NTEDIT_CN_* */
	uint32_t finished;   /* 1 after ntedit_hip_cn_finish, 0 again after an append or a reset */
	uint64_t batches[2]; /* stored, per side */
	uint64_t bytes[2];
	uint64_t entries[2];
	uint64_t cap;
	uint64_t counters;   /* of the last ntedit_hip_cn_finish */
	uint64_t nonzero[2]; /* its non-zero counters per side */
	float ms[4];         /* HIP-event sums: k_cn_count before, k_spectrum_cn before, k_cn_count after, k_spectrum_cn after */
} ntedit_hip_cn_stats;
int ntedit_hip_cn_info(ntedit_hip_ctx* ctx, ntedit_hip_cn_stats* st);
/* ntedit_hip_cn_reset: the batches and results go, the switch stays.  ntedit_hip_cn_free: the sketch and the result
 * buffers go as well. */
int ntedit_hip_cn_reset(ntedit_hip_ctx* ctx);
int ntedit_hip_cn_free(ntedit_hip_ctx* ctx);
/* <prefix>_spectrum_cn.tsv: "multiplicity", before_cn1 .. before_cn4, before_cn5plus, after_cn1 .. after_cn5plus, in
 * DISTINCT k-mers; one row per multiplicity 0 .. 255 from the two distinct[5][256].  <prefix>_cn_contigs.tsv: name (cut at
 * its first space or tab), then kmers and the five class counts of occurrences before and after; a last row "#total" (the
 * caller's sum) closes it.  Host only; NTEDIT_E_OVERFLOW when the row does not fit out[0 .. cap). */
const char* ntedit_hip_cn_header(void);
int ntedit_hip_cn_format_row(uint32_t multiplicity, const uint64_t* distinct_before, const uint64_t* distinct_after, char* out, uint64_t cap);
const char* ntedit_hip_cn_contig_header(void);
int ntedit_hip_cn_contig_format_row(const char* name, const ntedit_hip_cn_row* before, const ntedit_hip_cn_row* after, char* out, uint64_t cap);

/* The reference's candidate tables -- num_tries, polish_bases_array / snv_bases_array, multi_possible_bases (ntedit.cpp:172,
 * 176-199, 203-348) -- as the device code holds them (one GPU thread runs the machine's own candidate_bases /
 * insertion_candidate), as text: "num_tries 0 1 5 21 85 341", "polish A TCG", ..., "snv N ATCG", "multi A A AA AC ...".
 * tests/ compare its SHA-256 per section with the hashes of the same text extracted from the reference's source
 * (tests/golden/reference_tables.json, tests/tools/reference_tables.py).  *len = bytes needed (without the 0). */
int ntedit_hip_device_tables(ntedit_hip_ctx* ctx, char* out, uint64_t cap, uint64_t* len);

/* Identifies what the library's kernels were built from (a hash of the device-side sources, set by the Makefile):
 * bench.py stamps the counter records it keeps under profiles/ with it and quotes them only for the same build.
 * No counterpart in the reference. */
const char* ntedit_hip_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
