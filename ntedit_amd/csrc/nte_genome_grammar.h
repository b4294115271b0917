// nte_genome_grammar.h -- the stateful grammar of --gpu_parse for genome FASTA, written once beside the reads grammar
// (nte_reads_grammar.h, unchanged): the genome kernels of nte_reads_parse.hip and the serial host model
// (ntedit_hip_genome_parse_model, same unit) are both built from these functions.
//
// A genome chunk is any run of raw bytes of a FASTA file, cut anywhere: a chromosome does not fit a chunk that has to
// start at a record start.  What the cut hides is carried in an entry state:
//   GP_LINE_START   the chunk begins at a line start
//   GP_IN_HEADER    the chunk begins inside a '>' line
//   GP_IN_SEQ       the chunk begins inside a sequence line
// Lines are the runs between '\n', as in the reads grammar.  Line 0 takes its class from the entry state when that is
// IN_HEADER or IN_SEQ; every line that begins in the chunk is a header if its first byte is '>', sequence otherwise.
// The chunk's text, in raw order: one '\n' for every header line that begins in the chunk, and the bytes of every
// sequence line or piece of one.  Nothing else: no line's own '\n', nothing for the continued part of a header.  So
// the texts of consecutive chunks, each entered with its predecessor's exit state, concatenate to the text of the
// file parsed as one chunk, and that text split on '\n' holds the records' sequences in order.
// The exit state is LINE_START when the last raw byte is '\n', else the class of the last line; an empty chunk keeps
// its entry state.
// The chunk is clean unless it holds a '\r', a line that begins in it is empty (a first byte '\n' under LINE_START
// included), a sequence line that begins in it starts with '+' or '@', it is the file's first chunk and does not
// start with '>', it has more than n / 8 + 1 lines, or it has 2^31 bytes or more (the RP_BAD_* bits).  The line bound
// alone depends on where the cuts fall (a line cut in two counts twice, and every chunk has its own "+ 1").
#pragma once

#include "nte_reads_grammar.h"

#include <string.h>

namespace nte_parse {

enum : int { GP_LINE_START = 0, GP_IN_HEADER = 1, GP_IN_SEQ = 2 };

// the class of a line: RP_HEADER (a header that begins in the chunk), RP_SEQ, or the continued part of a header
enum : int { GP_HEADER_REST = 3 };

RP_HD bool
gp_state_ok(int state)
{
	return state == GP_LINE_START || state == GP_IN_HEADER || state == GP_IN_SEQ;
}

// what the chunk as a whole has to satisfy; first: its first byte
RP_HD uint32_t
gp_chunk_broken(int first_chunk, int first, uint64_t n_raw, uint64_t lines)
{
	uint32_t broken = 0;
	if (first_chunk && first != '>') {
		broken |= RP_BAD_FIRST;
	}
	if (n_raw >= RP_MAX_RAW) {
		broken |= RP_BAD_SIZE;
	}
	if (lines > rp_max_lines(n_raw)) {
		broken |= RP_BAD_TABLE;
	}
	return broken;
}

// The line bound is a rule of the grammar, but the line table is built for GP_TABLE_SLACK raw bytes more than the chunk
// has: a small chunk of short lines (a file wrapped at 1, a chunk of 7 bytes with a '\n' in its middle) is unclean and
// still gets its text and its exit state, so that chunking never changes the text.  Only over the table itself, or over
// 32-bit positions, nothing else of the chunk is looked at.
constexpr uint64_t GP_TABLE_SLACK = 1ull << 20;

RP_HD bool
gp_stops(uint64_t n_raw, uint64_t lines)
{
	return n_raw >= RP_MAX_RAW || lines > rp_max_lines(n_raw + GP_TABLE_SLACK);
}

// the class of line `line` of a chunk entered in `state`; first: its first byte, -1 for an empty line; *broken |= its
// rules (a continued line 0 began in an earlier chunk: it may be empty and start with anything)
RP_HD int
gp_line_class(int state, uint64_t line, int first, uint32_t* broken)
{
	if (line == 0 && state == GP_IN_HEADER) {
		return GP_HEADER_REST;
	}
	if (line == 0 && state == GP_IN_SEQ) {
		return RP_SEQ;
	}
	if (first < 0) {
		*broken |= RP_BAD_EMPTY;
	}
	if (first == '>') {
		return RP_HEADER;
	}
	if (first == '+' || first == '@') {
		*broken |= RP_BAD_SEQ_START;
	}
	return RP_SEQ;
}

// what a line of `len` bytes puts into the text, for the scan over the lines: hi = headers begun, lo = text bytes
RP_HD uint64_t
gp_line_emit(int cls, uint64_t len)
{
	return cls == RP_HEADER ? (1ull << 32) | 1ull : cls == RP_SEQ ? len : 0ull;
}

// the exit state of a chunk whose last line has class `cls`; last_nl: its last byte is '\n'
RP_HD int
gp_state_out(int last_nl, int cls)
{
	return last_nl ? GP_LINE_START : cls == RP_SEQ ? GP_IN_SEQ : GP_IN_HEADER;
}

// ------------------------------------------------------------------ the serial model (host)
struct GpResult
{
	int clean;
	uint32_t broken;
	int state_out;
	uint64_t text_len, bases, lines, last_header;
};

constexpr uint64_t GP_NO_START = ~0ull;

// One chunk, one line after the other, by the functions above: the text into out[0 .. cap) as far as it fits.  Returns
// whether it fitted.  Reads raw[0 .. n_raw) and writes out[0 .. min(cap, text_len)), nothing else.
inline bool
gp_model(const char* raw, uint64_t n_raw, int state_in, int first_chunk, char* out, uint64_t cap, GpResult* res)
{
	*res = GpResult();
	res->last_header = GP_NO_START;
	res->state_out = state_in;
	if (n_raw == 0) {
		res->clean = 1;
		return true;
	}
	uint64_t lines = 0;
	bool cr = false;
	for (uint64_t i = 0; i < n_raw; i++) {
		lines += raw[i] == '\n';
		cr = cr || raw[i] == '\r';
	}
	const int last_nl = raw[n_raw - 1] == '\n';
	lines += last_nl ? 0 : 1;
	if (gp_stops(n_raw, lines)) {
		res->broken = n_raw >= RP_MAX_RAW ? (uint32_t)RP_BAD_SIZE : gp_chunk_broken(0, 0, n_raw, lines);
		res->lines = n_raw >= RP_MAX_RAW ? 0 : lines;
		res->state_out = 0;
		return true;
	}
	uint32_t broken = gp_chunk_broken(first_chunk != 0, (unsigned char)raw[0], n_raw, lines) | (cr ? (uint32_t)RP_BAD_CR : 0u);
	uint64_t used = 0, headers = 0, line = 0;
	int cls = 0;
	for (uint64_t s = 0; s < n_raw; line++) {
		const char* nl = (const char*)memchr(raw + s, '\n', n_raw - s);
		const uint64_t e = nl ? (uint64_t)(nl - raw) : n_raw;
		cls = gp_line_class(state_in, line, e > s ? (int)(unsigned char)raw[s] : -1, &broken);
		if (cls == RP_HEADER) {
			if (used < cap) {
				out[used] = '\n';
			}
			res->last_header = s;
			headers++;
		} else if (cls == RP_SEQ && e > s && used + (e - s) <= cap) {
			memcpy(out + used, raw + s, e - s);
		}
		used += (uint32_t)gp_line_emit(cls, e - s);
		s = e + 1;
	}
	res->broken = broken;
	res->clean = broken == 0;
	res->state_out = gp_state_out(last_nl, cls);
	res->text_len = used;
	res->bases = used - headers;
	res->lines = lines;
	return used <= cap;
}

} // namespace nte_parse
