// nte_reads_model.h -- the serial host model of the clean grammar (nte_reads_grammar.h), apart from it so that the header
// the kernels share stays free of host-only code: ntedit_hip_reads_parse_model_q is this function, and a host program
// (tests/min_qual/min_qual_host.cpp) builds it without HIP.
#pragma once

#include "nte_reads_grammar.h"

#include <string.h>

#include <string>

namespace nte_parse {

struct RpResult // (ntedit_hip_reads_parse_result, field for field)
{
	int clean;
	uint32_t broken;
	int kind;
	uint64_t text_len, reads, bases, lines;
};

// The serial model (ntedit_hip_reads_parse_model_q): the functions above, one line after the other.  The text into
// out[0 .. cap) as far as it fits; res->text_len is its whole length either way (false: it did not fit).  With min_qual a
// FASTQ record's bases are masked by its quality line as far as that line reaches: in a clean chunk all of them, and an
// unclean chunk has no text.
// With a filter (rp_record_reason) a FASTQ record's quality weights are summed over its quality line as stored, whatever
// min_qual masks; fc (may be NULL) += what the records of a clean chunk came to.
inline bool
rp_model_f(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, const ReadFilter& f, char* out, uint64_t cap, RpResult* res,
           ReadFilterCounts* fc)
{
	*res = RpResult();
	if (n_raw == 0) {
		res->clean = 1;
		return true;
	}
	const int kind = (unsigned char)raw[0];
	uint32_t broken = memchr(raw, '\r', n_raw) ? (uint32_t)RP_BAD_CR : 0u;
	uint64_t lines = 0, used = 0, reads = 0, bases = 0, seq_len = 0, qual_sum = 0;
	std::string cur;
	bool open = false, has_qual = false;
	ReadFilterCounts seen = ReadFilterCounts();
	auto flush = [&]() {
		const uint32_t why = open ? rp_record_reason(cur.size(), k, f, has_qual, qual_sum) : (uint32_t)RP_DROP_LENGTH;
		if (open && rp_filter_on(f)) {
			seen.records++;
			seen.by_length += why == RP_DROP_LENGTH;
			seen.by_mean_qual += why == RP_DROP_MEAN_QUAL;
		}
		qual_sum = 0;
		has_qual = false;
		if (open && why == RP_KEPT) {
			if (used + cur.size() + 1 <= cap) {
				memcpy(out + used, cur.data(), cur.size());
				out[used + cur.size()] = '\n';
			}
			used += cur.size() + 1;
			reads++;
			bases += cur.size();
		}
		cur.clear();
	};
	for (uint64_t s = 0; s < n_raw; lines++) {
		const char* nl = (const char*)memchr(raw + s, '\n', n_raw - s);
		const uint64_t e = nl ? (uint64_t)(nl - raw) : n_raw;
		const int c = rp_line_class(kind, lines, e > s ? (int)(unsigned char)raw[s] : -1, &broken);
		if (c == RP_HEADER) {
			flush();
			open = true;
			seq_len = 0;
		} else if (c == RP_SEQ) {
			cur.append(raw + s, e - s);
			seq_len = e - s;
		} else if (kind == '@' && lines % 4 == 3) {
			broken |= rp_quality_broken(seq_len, e - s);
			has_qual = true;
			for (uint64_t j = 0; f.min_mean_qual && j < e - s; j++) {
				qual_sum += rp_qual_weight((int)(unsigned char)raw[s + j] - RP_QUAL_OFFSET);
			}
			for (uint64_t j = 0; min_qual && j < seq_len && j < e - s; j++) { // (cur ends with the sequence line's seq_len bytes)
				char& base = cur[cur.size() - seq_len + j];
				base = (char)rp_mask_base((uint8_t)base, (int)(unsigned char)raw[s + j] - RP_QUAL_OFFSET, min_qual);
			}
		}
		s = e + 1;
	}
	flush();
	broken |= rp_chunk_broken(kind, n_raw, lines);
	res->kind = kind;
	res->lines = lines;
	res->broken = broken;
	if (broken) {
		return true;
	}
	res->clean = 1;
	res->text_len = used;
	res->reads = reads;
	res->bases = bases;
	if (fc) {
		fc->records += seen.records;
		fc->by_length += seen.by_length;
		fc->by_mean_qual += seen.by_mean_qual;
	}
	return used <= cap;
}

inline bool
rp_model(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, char* out, uint64_t cap, RpResult* res)
{
	return rp_model_f(raw, n_raw, k, min_qual, ReadFilter(), out, cap, res, nullptr);
}

} // namespace nte_parse
