// nte_reads_internal.h -- what the units of the reads and genome front end call of each other beyond the public C ABI
// (include/ntedit_hip.h): every nte_reads:: function that crosses a translation unit, declared once, by the unit that
// defines it.  The device units (nte_reads.hip, nte_reads_parse.hip, nte_reads_inflate.hip, nte_reads_bam.hip,
// nte_bgzf_deflate.hip) and the host sources (host/reads_pass.cpp, reads_build.cpp, reads_options.cpp, genome_pass.cpp)
// all include it; the host sources see no HIP runtime header, so a stream crosses as a void*.
#pragma once

#include "../../include/ntedit_hip.h"
#include "nte_reads_grammar.h" // (ReadFilter, ReadFilterCounts)

#include <stdint.h>

#include <string>

namespace nte_reads {

// ------------------------------------------------------------------ nte_reads.hip
// the store of ntedit_hip_reads_last_error: the failures of every unit and of the host side go to it; returns code
int set_error(const ntedit_hip_ctx* c, int code, const std::string& why);
// the context's reject cutoff (ntedit_hip_reads_set_reject_cutoff); 0: none, and none without a sketch
uint32_t reject_cutoff(const ntedit_hip_ctx* c);
// the shortest record the parsers keep for a sketch at k (ntedit_hip_reads_set_min_read): never above k, so that no
// read with a k-mer is dropped
uint32_t min_read(const ntedit_hip_ctx* c, uint32_t k);

// ------------------------------------------------------------------ nte_reads_parse.hip (--gpu_parse)
// ntedit_hip_sketch_free: the scratch of the three device units goes (parse_release calls inflate_release, which calls
// bam_release; the streams are this unit's and go last), their settings and the last pass's counts stay
void parse_release(const ntedit_hip_ctx* c);
// the inflate and BAM units work on this unit's two streams (hipStream_t) ...
int parse_streams(const ntedit_hip_ctx* c, void** stream, void** copy_stream);
// ... cut a chunk on the line table: the first phases of a parse over device bytes, queued on the stream.
// *broken: RP_BAD_SIZE / RP_BAD_TABLE when the table cannot hold the chunk (nothing is queued then).
int parse_lines(const ntedit_hip_ctx* c, const unsigned char* d_raw, uint64_t n, const uint32_t** line_end, uint64_t* n_lines,
                uint32_t* broken);
// ... have device bytes parsed into the context's text buffer, as parse_copied does for a copied chunk
int parse_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res);
// ... and decode into the same text buffer: room for a chunk of n raw bytes
int parse_text_buffer(const ntedit_hip_ctx* c, uint64_t n, char** text, uint64_t* cap);
// the context's setting (ntedit_hip_reads_set_device_parse) and its counters
int parse_is_on(const ntedit_hip_ctx* c);
ntedit_hip_reads_parse_stats* parse_info(const ntedit_hip_ctx* c);
// host chunk -> raw buffer `which`, on the copy stream; returns at once
int parse_copy_begin(const ntedit_hip_ctx* c, int which, const char* host, uint64_t n);
int parse_copy_wait(const ntedit_hip_ctx* c, int which);
// waits for that copy, then parses the buffer into the context's text buffer (*text: where, 16-byte aligned)
int parse_copied(const ntedit_hip_ctx* c, int which, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res);
// --min_qual: the context's setting, which the device parsers read themselves, and the counts of the last pass (the pass
// zeroes them; the host parser and the BAM unit add theirs)
uint32_t min_qual(const ntedit_hip_ctx* c);
void min_qual_count(const ntedit_hip_ctx* c, int reset, uint64_t qual_bases, uint64_t masked_bases);
// --min_read_len, --min_mean_qual, --min_rq: the context's setting, alike, and what the last pass's records came to
nte_parse::ReadFilter read_filter(const ntedit_hip_ctx* c);
void read_filter_count(const ntedit_hip_ctx* c, int reset, const nte_parse::ReadFilterCounts* add);
// The genome chunks (host/genome_pass.cpp).  The pass's text buffer: genome_pad() bytes that end with the last k - 1 text
// bytes of the file so far ('\n' before them), then the chunk's text; the whole is one device batch for
// ntedit_hip_filter_insert.
ntedit_hip_genome_pass_info* genome_info(const ntedit_hip_ctx* c);
int genome_pad(void);
// a file begins: nothing is carried
int genome_begin_file(const ntedit_hip_ctx* c);
// raw buffer `which` with room for n bytes (a BGZF chunk is inflated into it)
int genome_raw_buffer(const ntedit_hip_ctx* c, int which, uint64_t n, char** d_raw);
// raw buffer `which` (copied: after parse_copy_begin, waits for that copy) parsed behind the pad; *batch: the pad's first
// byte, the text is at *batch + genome_pad()
int genome_parse_buffer(const ntedit_hip_ctx* c, int which, int copied, uint64_t n, int state_in, int first_chunk, const char** batch,
                        ntedit_hip_genome_parse_result* res);
// the chunk's text is inserted: the pad becomes the last `keep` (< genome_pad()) bytes of pad + text, '\n' before them
int genome_carry(const ntedit_hip_ctx* c, uint64_t text_len, uint32_t keep);

// ------------------------------------------------------------------ nte_reads_inflate.hip (--gpu_parse on BGZF files)
void inflate_release(const ntedit_hip_ctx* c); // (its scratch works on the parse unit's streams)
ntedit_hip_reads_inflate_stats* inflate_info(const ntedit_hip_ctx* c);
const char* inflate_reason(uint32_t st); // NTEDIT_INFLATE_* in words
// a chunk's compressed bytes and member table -> buffers `which`, on the copy stream; returns at once
int inflate_copy_begin(const ntedit_hip_ctx* c, int which, const char* comp, uint64_t n_comp, const ntedit_hip_bgzf_member* members,
                       uint64_t n_members);
int inflate_copy_wait(const ntedit_hip_ctx* c, int which);
// Waits for that copy, then inflates its members (the host's copy of the table: `members`, checked here) behind the
// `tail` bytes the current raw buffer already holds.  *raw: the buffer.  *bad: the first refused member, or n_members.
int inflate_copied(const ntedit_hip_ctx* c, int which, uint64_t n_comp, const ntedit_hip_bgzf_member* members, uint64_t n_members,
                   uint64_t tail, uint64_t n_out, const char** raw, uint64_t* bad, uint32_t* reason);
// the last record start of the current raw buffer's first n bytes; *cut = 0: none.  *broken: the line table cannot
// hold the bytes (the chunk is unclean then, whatever the cut)
int inflate_last_start(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint64_t* cut, uint32_t* broken);
// the bytes [cut, total) of the current raw buffer to the front of the other one, which becomes the current
int inflate_carry(const ntedit_hip_ctx* c, uint64_t cut, uint64_t total);

// ------------------------------------------------------------------ nte_reads_bam.hip (--gpu_parse on BAM files)
void bam_release(const ntedit_hip_ctx* c); // (it works on the same streams, behind the inflate unit's chunks)
ntedit_hip_reads_bam_stats* bam_info(const ntedit_hip_ctx* c);
// the first n bytes of the inflated chunk d_raw: walked, and the records before the cut decoded into the context's text
// buffer (the one parse_buffer fills)
int bam_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, int at_header, uint32_t min_len, const char** text,
               ntedit_hip_reads_bam_result* res);

} // namespace nte_reads
