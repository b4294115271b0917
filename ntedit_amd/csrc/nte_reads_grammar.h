// nte_reads_grammar.h -- the clean grammar of --gpu_parse, written once: the class of a line, what makes a chunk clean,
// which records are kept (by length, and by the read filter's rules), and what --min_qual makes of a base.  The parse
// kernels (nte_reads_parse.hip) and the serial host model (rp_model of nte_reads_model.h: ntedit_hip_reads_parse_model)
// are both built from these functions, as nte_lanes.h serves the machine.
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

// --min_read_len L, --min_mean_qual Q, --min_rq R: which records are kept, beyond their length against k.  A record goes
// into the text when it passes every rule; a dropped one is counted under the first rule that drops it, in the order
// flag (BAM), length, rq, mean quality.  Written once: the record kernels, the two models and the host parser call these.
struct ReadFilter
{
	uint32_t min_len;       // --min_read_len (0: off): the shortest record kept is max(min_len, what it is without)
	uint32_t min_mean_qual; // --min_mean_qual (0: off), 1 to RP_MAX_MEAN_QUAL
	uint32_t rq_bits;       // --min_rq R as the bits of the float (0: off); nte_bam_grammar.h applies it
};

enum : uint32_t { RP_KEPT = 0, RP_DROP_FLAG = 1, RP_DROP_LENGTH = 2, RP_DROP_RQ = 3, RP_DROP_MEAN_QUAL = 4 };

// what the last pass's records came to (ntedit_hip_reads_read_filter_stats, field for field)
struct ReadFilterCounts
{
	uint64_t records, by_length, by_rq, by_mean_qual, rq_tagged, aux_malformed;
};

constexpr uint32_t RP_MAX_MEAN_QUAL = 60;
constexpr uint32_t RP_MAX_MIN_READ_LEN = 0x7FFFFFFFu;
constexpr uint32_t RP_MAX_QUAL = 93;

// R as ReadFilter keeps it: the float's bits, and 0 (off) for every value that is not above 0, -0.0 among them (host only)
inline uint32_t
rp_rq_bits(float min_rq)
{
	union { float f; uint32_t u; } v;
	v.f = min_rq;
	return min_rq > 0.0f ? v.u : 0u;
}

// the filter of (L, Q, R) as the options and the calls give them; false when one is out of range: L above
// RP_MAX_MIN_READ_LEN, Q above RP_MAX_MEAN_QUAL, R not within [0, 1] (written so that a NaN is refused) (host only)
inline bool
rp_make_filter(uint32_t min_len, uint32_t min_mean_qual, float min_rq, ReadFilter* f)
{
	if (min_len > RP_MAX_MIN_READ_LEN || min_mean_qual > RP_MAX_MEAN_QUAL || !(min_rq >= 0.0f && min_rq <= 1.0f)) {
		return false;
	}
	f->min_len = min_len;
	f->min_mean_qual = min_mean_qual;
	f->rq_bits = rp_rq_bits(min_rq);
	return true;
}

// a chunk's counts onto the pass's (host only)
inline void
rp_counts_add(ReadFilterCounts* to, const ReadFilterCounts& add)
{
	to->records += add.records;
	to->by_length += add.by_length;
	to->by_rq += add.by_rq;
	to->by_mean_qual += add.by_mean_qual;
	to->rq_tagged += add.rq_tagged;
	to->aux_malformed += add.aux_malformed;
}

RP_HD bool
rp_filter_on(const ReadFilter& f)
{
	return f.min_len || f.min_mean_qual || f.rq_bits;
}

// the shortest record kept: max(L, what it is without the option)
RP_HD uint32_t
rp_min_len(const ReadFilter& f, uint32_t k)
{
	return f.min_len > k ? f.min_len : k;
}

// A read's mean quality is the Phred value of its mean error probability (as NanoFilt, chopper and fastplong take it),
// not the mean of the Phred values, and it is computed in integers so that every adder agrees to the bit whatever its
// order: E[q] = round(2^31 * 10^(-q/10)) for q = 0 .. 93, no entry a rounding tie (computed with 60 decimal digits).
constexpr uint32_t RP_QUAL_WEIGHT[94] = {
	2147483648u, 1705806895u, 1354970580u, 1076291389u, 854928639u, 679093957u, 539423504u, 428479319u,
	340353221u, 270352174u, 214748365u, 170580690u, 135497058u, 107629139u, 85492864u, 67909396u,
	53942350u, 42847932u, 34035322u, 27035217u, 21474836u, 17058069u, 13549706u, 10762914u,
	8549286u, 6790940u, 5394235u, 4284793u, 3403532u, 2703522u, 2147484u, 1705807u,
	1354971u, 1076291u, 854929u, 679094u, 539424u, 428479u, 340353u, 270352u,
	214748u, 170581u, 135497u, 107629u, 85493u, 67909u, 53942u, 42848u,
	34035u, 27035u, 21475u, 17058u, 13550u, 10763u, 8549u, 6791u,
	5394u, 4285u, 3404u, 2704u, 2147u, 1706u, 1355u, 1076u,
	855u, 679u, 539u, 428u, 340u, 270u, 215u, 171u,
	135u, 108u, 85u, 68u, 54u, 43u, 34u, 27u,
	21u, 17u, 14u, 11u, 9u, 7u, 5u, 4u,
	3u, 3u, 2u, 2u, 1u, 1u,
};

// the table's index for a Phred quality: a FASTQ byte below the offset counts as 0, a quality above 93 as 93
RP_HD uint32_t
rp_qual_index(int qual)
{
	return qual < 0 ? 0u : qual > (int)RP_MAX_QUAL ? RP_MAX_QUAL : (uint32_t)qual;
}

// what a base of Phred quality `qual` adds to its read's sum (a kernel reads its own copy of the table at rp_qual_index)
RP_HD uint32_t
rp_qual_weight(int qual)
{
	return RP_QUAL_WEIGHT[rp_qual_index(qual)];
}

// the one comparison: a read of `len` bases (< 2^31, so sum < 2^62) whose weights sum to `sum` has a mean quality of
// Q or more
RP_HD bool
rp_mean_qual_kept(uint64_t sum, uint64_t len, uint32_t min_mean_qual)
{
	return sum <= len * (uint64_t)RP_QUAL_WEIGHT[min_mean_qual];
}

// a text record (FASTA: has_qual false) of len bases whose quality weights sum to `sum`: RP_KEPT or the rule that drops it
RP_HD uint32_t
rp_record_reason(uint64_t len, uint32_t k, const ReadFilter& f, bool has_qual, uint64_t sum)
{
	if (!rp_record_kept(len, rp_min_len(f, k))) {
		return RP_DROP_LENGTH;
	}
	if (f.min_mean_qual && has_qual && !rp_mean_qual_kept(sum, len, f.min_mean_qual)) {
		return RP_DROP_MEAN_QUAL;
	}
	return RP_KEPT;
}

} // namespace nte_parse
