// qv.cpp -- the k-mer QV of a polish: the formula and the lines of <prefix>_qv.tsv (host arithmetic only; the counts come
// from nte_apply.hip through ntedit_hip_result_qv).
#include "../../include/ntedit_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

extern "C" {

double
ntedit_hip_qv_value(uint64_t absent, uint64_t kmers, uint32_t k)
{
	if (kmers == 0 || k == 0) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	if (absent == 0) {
		return std::numeric_limits<double>::infinity();
	}
	if (absent >= kmers) {
		return 0.0; // (no k-mer shared: an error rate of 1)
	}
	const double shared = 1.0 - (double)absent / (double)kmers;
	const double err = 1.0 - std::pow(shared, 1.0 / (double)k);
	return -10.0 * std::log10(err);
}

const char*
ntedit_hip_qv_header(void)
{
	return "name\tlen_before\tlen_after\tkmers_before\tabsent_before\tqv_before\tkmers_after\tabsent_after\tqv_after\n";
}

static std::string
qv_text(uint64_t absent, uint64_t kmers, uint32_t k)
{
	const double q = ntedit_hip_qv_value(absent, kmers, k);
	if (std::isnan(q)) {
		return "NA";
	}
	if (std::isinf(q)) {
		return "inf";
	}
	char b[64];
	snprintf(b, sizeof b, "%.2f", q);
	return b;
}

int
ntedit_hip_qv_format_row(const char* name, const ntedit_hip_qv_row* row, uint32_t k, char* out, uint64_t cap)
{
	if (!name || !row || !out) {
		return NTEDIT_E_ARG;
	}
	std::string s(name);
	auto num = [&](uint64_t v) {
		s.push_back('\t');
		s += std::to_string(v);
	};
	num(row->len_before);
	num(row->len_after);
	num(row->kmers_before);
	num(row->absent_before);
	s.push_back('\t');
	s += qv_text(row->absent_before, row->kmers_before, k);
	num(row->kmers_after);
	num(row->absent_after);
	s.push_back('\t');
	s += qv_text(row->absent_after, row->kmers_after, k);
	s.push_back('\n');
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

// ---- the unsupported regions as BED rows (the intervals come from nte_track.hip through ntedit_hip_result_track)

int
ntedit_hip_track_format_row(const char* name, const ntedit_hip_track_interval* iv, char* out, uint64_t cap)
{
	if (!name || !iv || !out) {
		return NTEDIT_E_ARG;
	}
	std::string s(name, strcspn(name, " \t")); // (the sequence name as faidx and IGV understand it)
	s += '\t' + std::to_string(iv->begin) + '\t' + std::to_string(iv->end) + '\t' + std::to_string(iv->absent) + '\n';
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

// ---- the k-mer spectrum and the depth rows (the counts come from k_spectrum through ntedit_hip_result_spectrum / _depth)

const char*
ntedit_hip_spectrum_header(void)
{
	return "multiplicity\tbefore\tafter\n";
}

int
ntedit_hip_spectrum_format_row(uint32_t multiplicity, uint64_t before, uint64_t after, char* out, uint64_t cap)
{
	if (!out || multiplicity > 255) {
		return NTEDIT_E_ARG;
	}
	const std::string s = std::to_string(multiplicity) + '\t' + std::to_string(before) + '\t' + std::to_string(after) + '\n';
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

const char*
ntedit_hip_depth_header(void)
{
	return "name\tkmers_before\tmean_before\tsaturated_before\tkmers_after\tmean_after\tsaturated_after\n";
}

static std::string
mean_text(uint64_t sum, uint64_t kmers)
{
	if (kmers == 0) {
		return "NA";
	}
	char b[64];
	snprintf(b, sizeof b, "%.2f", (double)sum / (double)kmers);
	return b;
}

int
ntedit_hip_depth_format_row(const char* name, const ntedit_hip_depth_row* row, char* out, uint64_t cap)
{
	if (!name || !row || !out) {
		return NTEDIT_E_ARG;
	}
	std::string s(name, strcspn(name, " \t")); // (the sequence name as faidx understands it)
	s += '\t' + std::to_string(row->kmers_before) + '\t' + mean_text(row->sum_before, row->kmers_before) + '\t' + std::to_string(row->saturated_before);
	s += '\t' + std::to_string(row->kmers_after) + '\t' + mean_text(row->sum_after, row->kmers_after) + '\t' + std::to_string(row->saturated_after) + '\n';
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

// ---- the spectrum by copy number (the counts come from k_spectrum_cn through ntedit_hip_cn_table / _rows)

// Distinct k-mers from occurrences, beside ntedit_hip_reads_hist_summary's rule f[e] = round(occ[e] / e): a k-mer of copy
// number c occurs c times, so class c holds occ / c of them, rounded (exact without sketch collisions); class 5plus mixes
// copy numbers, so the kernel summed 2^32 / cn per occurrence instead and the sum is rounded here.
int
ntedit_hip_cn_distinct(const uint64_t* occ, const uint64_t* w5, uint64_t* distinct)
{
	if (!occ || !w5 || !distinct) {
		return NTEDIT_E_ARG;
	}
	for (uint64_t c = 1; c <= 4; c++) {
		for (int m = 0; m < 256; m++) {
			distinct[(c - 1) * 256 + m] = (occ[(c - 1) * 256 + m] + c / 2) / c;
		}
	}
	for (int m = 0; m < 256; m++) {
		distinct[4 * 256 + m] = (w5[m] + (1ull << 31)) >> 32;
	}
	return 0;
}

const char*
ntedit_hip_cn_header(void)
{
	return "multiplicity\tbefore_cn1\tbefore_cn2\tbefore_cn3\tbefore_cn4\tbefore_cn5plus\tafter_cn1\tafter_cn2\tafter_cn3\tafter_cn4\tafter_cn5plus\n";
}

int
ntedit_hip_cn_format_row(uint32_t multiplicity, const uint64_t* distinct_before, const uint64_t* distinct_after, char* out, uint64_t cap)
{
	if (!out || !distinct_before || !distinct_after || multiplicity > 255) {
		return NTEDIT_E_ARG;
	}
	std::string s = std::to_string(multiplicity);
	for (const uint64_t* d : { distinct_before, distinct_after }) {
		for (int c = 0; c < 5; c++) {
			s += '\t' + std::to_string(d[c * 256 + multiplicity]);
		}
	}
	s += '\n';
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

const char*
ntedit_hip_cn_contig_header(void)
{
	return "name\tkmers_before\tbefore_cn1\tbefore_cn2\tbefore_cn3\tbefore_cn4\tbefore_cn5plus\tkmers_after\tafter_cn1\tafter_cn2\tafter_cn3\tafter_cn4\t"
	       "after_cn5plus\n";
}

int
ntedit_hip_cn_contig_format_row(const char* name, const ntedit_hip_cn_row* before, const ntedit_hip_cn_row* after, char* out, uint64_t cap)
{
	if (!name || !before || !after || !out) {
		return NTEDIT_E_ARG;
	}
	std::string s(name, strcspn(name, " \t")); // (the sequence name as faidx understands it)
	for (const ntedit_hip_cn_row* r : { before, after }) {
		for (uint64_t v : { r->kmers, r->cn1, r->cn2, r->cn3, r->cn4, r->cn5plus }) {
			s += '\t' + std::to_string(v);
		}
	}
	s += '\n';
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

// ---- k-mer completeness (linear counting: the marks come from k_mark through ntedit_hip_shared_counts)

double
ntedit_hip_bloom_cardinality(uint64_t set, uint64_t slots, uint32_t h)
{
	if (slots == 0 || h == 0) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	if (set == 0) {
		return 0.0;
	}
	if (set >= slots) {
		return std::numeric_limits<double>::infinity();
	}
	return -((double)slots / (double)h) * std::log1p(-(double)set / (double)slots);
}

const char*
ntedit_hip_completeness_header(void)
{
	return "stage\tfilter_bits\tfilter_set\tfilter_kmers\tshared_set\tshared_kmers\tcompleteness\n";
}

int
ntedit_hip_completeness_format_row(const char* stage, const ntedit_hip_shared_stats* st, int which, char* out, uint64_t cap)
{
	if (!stage || !st || !out || which < 0 || which > 1) {
		return NTEDIT_E_ARG;
	}
	const double filter_kmers = ntedit_hip_bloom_cardinality(st->filter_set, st->bits, st->hash_num);
	const double shared_kmers = ntedit_hip_bloom_cardinality(st->shared_set[which], st->bits, 1);
	const bool both = std::isfinite(filter_kmers) && std::isfinite(shared_kmers) && filter_kmers != 0.0;
	auto rounded = [](double v) { return std::isfinite(v) ? std::to_string(std::llround(v)) : std::string("NA"); };
	std::string s(stage);
	s += '\t' + std::to_string(st->bits) + '\t' + std::to_string(st->filter_set) + '\t' + rounded(filter_kmers);
	s += '\t' + std::to_string(st->shared_set[which]) + '\t' + rounded(shared_kmers) + '\t';
	if (both) {
		char b[64];
		snprintf(b, sizeof b, "%.6f", shared_kmers / filter_kmers);
		s += b;
	} else {
		s += "NA";
	}
	s.push_back('\n');
	if (s.size() + 1 > cap) {
		return NTEDIT_E_OVERFLOW;
	}
	memcpy(out, s.c_str(), s.size() + 1);
	return 0;
}

} // extern "C"
