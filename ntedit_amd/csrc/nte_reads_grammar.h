// nte_reads_grammar.h -- the clean grammar of --gpu_parse, written once: the class of a line, what makes a chunk clean,
// which records are kept, and what --min_qual makes of a base.  The parse kernels (nte_reads_parse.hip) and the serial
// host model (rp_model of nte_reads_model.h: ntedit_hip_reads_parse_model) are both built from these functions, as
// nte_lanes.h serves the machine.
//
// A chunk is a run of raw file bytes that starts at a record start.  Its kind is its first byte, '>' (FASTA) or '@'
// (4-line FASTQ).  Lines are the runs between '\n'; bytes behind the last '\n' are a last line of their own.  The
// chunk is clean when no rule below is broken, and then its text -- every record of k bases or more, followed by
// '\n', in order -- is exactly what kseq's rules (FastaReader::next) make of it:
//   every chunk   no '\r' anywhere (kseq strips one from an accumulated string: not reproduced); no empty line (kseq
//                 skips them inside a sequence; narrower than needed, and one rule less to prove)
//   FASTA         a line that starts with '>' is a header, every other line is sequence and starts with neither '+'
//                 (kseq would read a quality string) nor '@' (kseq would start a record); a record's sequence is the
//                 concatenation of its sequence lines
//   FASTQ         line 4i starts with '@', line 4i+1 is the sequence and starts with none of '>', '+', '@', line 4i+2
//                 starts with '+', line 4i+3 is as long as line 4i+1 whatever its first byte; the lines are a multiple
//                 of 4
// and the line table holds it: at most one line per 8 raw bytes (+ 1).
#pragma once

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RP_HD __host__ __device__ inline __attribute__((always_inline)) // (spelled out: a host source may see no HIP runtime header)
#else
#define RP_HD inline
#endif

namespace nte_parse {

enum : int { RP_HEADER = 0, RP_SEQ = 1, RP_SKIP = 2 };

// the rules, as bits of `broken` (NTEDIT_PARSE_BAD_* in ntedit_hip.h)
enum : uint32_t {
	RP_BAD_FIRST = 1,      // the first byte is neither '>' nor '@'
	RP_BAD_CR = 2,         // a '\r'
	RP_BAD_EMPTY = 4,      // an empty line
	RP_BAD_SEQ_START = 8,  // a sequence line that starts with '>', '+' or '@'
	RP_BAD_FQ_LINES = 16,  // FASTQ: the lines are not a multiple of 4
	RP_BAD_FQ_HEADER = 32, // FASTQ: line 4i does not start with '@'
	RP_BAD_FQ_PLUS = 64,   // FASTQ: line 4i+2 does not start with '+'
	RP_BAD_FQ_QUAL = 128,  // FASTQ: line 4i+3 is not as long as line 4i+1
	RP_BAD_TABLE = 256,    // more lines than the line table holds
	RP_BAD_SIZE = 512,     // the chunk is too large for 32-bit positions
};

constexpr uint64_t RP_MAX_RAW = 1ull << 31;

// the line table's bound for a chunk of n raw bytes
RP_HD uint64_t
rp_max_lines(uint64_t n_raw)
{
	return n_raw / 8 + 1;
}

// what the chunk as a whole has to satisfy: its kind, its size, its number of lines
RP_HD uint32_t
rp_chunk_broken(int kind, uint64_t n_raw, uint64_t lines)
{
	uint32_t broken = 0;
	if (kind != '>' && kind != '@') {
		broken |= RP_BAD_FIRST;
	}
	if (n_raw >= RP_MAX_RAW) {
		broken |= RP_BAD_SIZE;
	}
	if (lines > rp_max_lines(n_raw)) {
		broken |= RP_BAD_TABLE;
	}
	if (kind == '@' && lines % 4 != 0) {
		broken |= RP_BAD_FQ_LINES;
	}
	return broken;
}

// the class of line `line` of a chunk of `kind`; first: its first byte, -1 for an empty line; *broken |= its rules
RP_HD int
rp_line_class(int kind, uint64_t line, int first, uint32_t* broken)
{
	if (first < 0) {
		*broken |= RP_BAD_EMPTY;
	}
	const bool starter = first == '>' || first == '+' || first == '@';
	if (kind != '@') {
		if (first == '>') {
			return RP_HEADER;
		}
		if (starter) {
			*broken |= RP_BAD_SEQ_START;
		}
		return RP_SEQ;
	}
	switch (line % 4) {
	case 0:
		if (first != '@') {
			*broken |= RP_BAD_FQ_HEADER;
		}
		return RP_HEADER;
	case 1:
		if (starter) {
			*broken |= RP_BAD_SEQ_START;
		}
		return RP_SEQ;
	case 2:
		if (first != '+') {
			*broken |= RP_BAD_FQ_PLUS;
		}
		return RP_SKIP;
	default:
		return RP_SKIP;
	}
}

// FASTQ line 4i+3 against line 4i+1
RP_HD uint32_t
rp_quality_broken(uint64_t seq_len, uint64_t qual_len)
{
	return seq_len == qual_len ? 0u : (uint32_t)RP_BAD_FQ_QUAL;
}

// a record of `len` bases goes into the text (len bytes and a '\n') when it can hold a k-mer
RP_HD bool
rp_record_kept(uint64_t len, uint32_t k)
{
	return len >= k;
}

// --min_qual Q (1..93, 0: off): the byte a base enters the text as, given its quality -- 'N' below the minimum, else the
// base.  `qual` is the Phred quality itself (a FASTQ byte less RP_QUAL_OFFSET, Phred+33; a BAM byte as stored); a FASTQ
// byte below the offset is below every minimum.  Written once: the copy and decode kernels, the two models and the host
// parser (FastaReader) all call it.
constexpr int RP_QUAL_OFFSET = 33;
constexpr uint32_t RP_MAX_MIN_QUAL = 93;

// the one comparison: whether a base of this quality is masked
RP_HD bool
rp_masked(int qual, uint32_t min_qual)
{
	return qual < (int)min_qual;
}

// ... and the one place a masked base becomes 'N' (for a caller that counts what rp_masked said)
RP_HD uint8_t
rp_mask_base(uint8_t base, bool masked)
{
	return masked ? (uint8_t)'N' : base;
}

RP_HD uint8_t
rp_mask_base(uint8_t base, int qual, uint32_t min_qual)
{
	return rp_mask_base(base, rp_masked(qual, min_qual));
}

} // namespace nte_parse
