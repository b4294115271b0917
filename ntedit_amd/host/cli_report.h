// cli_report.h -- what a polishing round says at its end: the QV table's total and summary line, the completeness table and
// line, the --bgzip and --bed lines, the --spectrum table and line, and the --report JSON lines.
#pragma once

#include "../../include/ntedit_hip.h"

#include <cstdio>
#include <string>
#include <vector>

namespace nte_cli {

// the totals of a round, summed over its batches
struct RoundTotals
{
	unsigned long long bases = 0;
	double seconds = 0, s_before_index = 0, s_index = 0, s_read = 0, s_call = 0, s_write = 0;
	double ms_gpu = 0, ms_screen = 0, ms_machine = 0;
	// which screening kernels ran: batches on the partitioned pipeline / on the direct kernel, record chunks the direct
	// kernel had to screen again, overflow-list entries
	unsigned n_batches_binned = 0, n_batches_direct = 0, n_chunks_direct = 0;
	unsigned long long n_ovf_records = 0;
	ntedit_hip_stats events = {};
	// --qv
	ntedit_hip_qv_row qv = {};
	double ms_apply = 0, ms_qv_screen = 0, ms_qv_count = 0;
	// --bgzip: the sums of ntedit_hip_bgzf_info over the batches
	double ms_bgzf_image = 0, ms_bgzf_deflate = 0, ms_bgzf_copy = 0;
	unsigned long long bgzf_plain = 0, bgzf_bytes = 0, bgzf_members = 0, bgzf_stored = 0;

	// --bed: intervals and covered bases before [0] and after [1], the extraction's times
	unsigned long long bed_intervals[2] = { 0, 0 }, bed_bases[2] = { 0, 0 };
	double ms_track[2] = { 0, 0 };

	// --spectrum: the bins before [0] and after [1] and the depth rows, summed; the two launches' times
	unsigned long long spectrum[2][256] = {};
	ntedit_hip_depth_row depth = {};
	double ms_spectrum[2] = { 0, 0 };

	void add(const ntedit_hip_stats& st);
	void add(const ntedit_hip_bgzf_stats& bs);
	void add(const ntedit_hip_qv_row& row);
};

// --qv: the "#total" row, the table closed, the summary line
void finish_qv(ntedit_hip_ctx* ctx, FILE* qv_f, const std::string& qv_path, uint32_t k, const RoundTotals& t);
// --completeness: <prefix>_completeness.tsv and one line, from the marks of all batches of the round; with --report its JSON
void finish_completeness(ntedit_hip_ctx* ctx, const std::string& prefix, uint32_t k, bool report);
// --bgzip: the summary line (the file's end-of-file member is counted in neither figure); with --report its JSON
void finish_bgzip(const RoundTotals& t, const std::string& fa_path, bool report);
// --bed: the summary line; with --report its JSON
void finish_bed(const RoundTotals& t, const std::string paths[2], bool report);
// --spectrum: <prefix>_spectrum.tsv from the summed bins, the "#total" row and the depth table closed, the summary line;
// with --report its JSON
void finish_spectrum(const RoundTotals& t, FILE* depth_f, const std::string paths[2], uint32_t k, bool report);
// --cn: ntedit_hip_cn_finish, <prefix>_spectrum_cn.tsv and <prefix>_cn_contigs.tsv under the names of the round's entries, the
// summary line; with --report its JSON.  A released store: one line on standard error, no file
void finish_cn(ntedit_hip_ctx* ctx, const std::vector<std::string>& names, const std::string paths[2], uint32_t k, unsigned long long sketch,
               bool report);
// --report
void report_qv(const RoundTotals& t);
void report_round(const RoundTotals& t);

} // namespace nte_cli
