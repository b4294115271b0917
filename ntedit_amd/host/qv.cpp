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

} // extern "C"
