// cli_report.cpp -- see cli_report.h
#include "cli_report.h"
#include "cli_common.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace nte_cli {

void
RoundTotals::add(const ntedit_hip_stats& st)
{
	ms_gpu += st.ms_total;
	ms_screen += st.ms_screen;
	n_batches_binned += st.screen_binned ? 1 : 0;
	n_batches_direct += st.screen_binned ? 0 : 1;
	n_chunks_direct += st.screen_chunks_direct;
	n_ovf_records += st.screen_overflow_records;
	ms_machine += st.ms_machine;
	events.events += st.events;
	events.events_applied += st.events_applied;
	events.absent_kmers += st.absent_kmers;
	events.substitutions += st.substitutions;
	events.insertions += st.insertions;
	events.deletions += st.deletions;
}

void
RoundTotals::add(const ntedit_hip_qv_row& row)
{
	qv.len_before += row.len_before;
	qv.len_after += row.len_after;
	qv.kmers_before += row.kmers_before;
	qv.absent_before += row.absent_before;
	qv.kmers_after += row.kmers_after;
	qv.absent_after += row.absent_after;
}

void
RoundTotals::add(const ntedit_hip_bgzf_stats& bs)
{
	ms_bgzf_image += bs.ms_image;
	ms_bgzf_deflate += bs.ms_deflate;
	ms_bgzf_copy += bs.ms_copy;
	bgzf_plain += bs.plain_bytes;
	bgzf_bytes += bs.bgzf_bytes;
	bgzf_members += bs.members;
	bgzf_stored += bs.stored_members;
}

static std::string
qv_text(uint64_t absent, uint64_t kmers, uint32_t k)
{
	const double q = ntedit_hip_qv_value(absent, kmers, k);
	char t[32];
	if (q != q) {
		return "NA";
	}
	snprintf(t, sizeof t, "%.2f", q);
	return q > 1e300 ? "inf" : t;
}

static std::string
count_text(double v)
{
	return std::isfinite(v) ? std::to_string(std::llround(v)) : std::string("NA");
}

static std::string
percent_text(double v)
{
	char t[32];
	snprintf(t, sizeof t, "%.4f %%", 100.0 * v);
	return std::isfinite(v) ? std::string(t) : std::string("NA");
}

static std::string
json_num(double v, const char* fmt)
{
	char t[48];
	snprintf(t, sizeof t, fmt, v);
	return std::isfinite(v) ? std::string(t) : std::string("null");
}

void
finish_qv(ntedit_hip_ctx* ctx, FILE* qv_f, const std::string& qv_path, uint32_t k, const RoundTotals& t)
{
	char line[512];
	bool ok = ntedit_hip_qv_format_row("#total", &t.qv, k, line, sizeof line) == 0 && fputs(line, qv_f) >= 0;
	ok = fclose(qv_f) == 0 && ok;
	if (!ok) {
		fail("cannot write `%s'", qv_path.c_str());
	}
	uint64_t occ = 0, slots = 0;
	uint32_t hn = 0;
	ntedit_hip_filter_info(ctx, NTEDIT_FILTER_PRIMARY, nullptr, &hn, nullptr, nullptr);
	double fpr = 0;
	if (ntedit_hip_filter_occupancy(ctx, NTEDIT_FILTER_PRIMARY, &occ, &slots) == 0 && slots) {
		fpr = pow((double)occ / (double)slots, (double)hn);
	}
	printf("k-mer QV (k=%u): before %s (%llu of %llu k-mers absent), after %s (%llu of %llu); Bloom false positives make "
	       "`absent' an undercount by about the filter's false-positive rate (occupancy^h = %.3g); table: %s\n",
	       k, qv_text(t.qv.absent_before, t.qv.kmers_before, k).c_str(), (unsigned long long)t.qv.absent_before,
	       (unsigned long long)t.qv.kmers_before, qv_text(t.qv.absent_after, t.qv.kmers_after, k).c_str(),
	       (unsigned long long)t.qv.absent_after, (unsigned long long)t.qv.kmers_after, fpr, qv_path.c_str());
}

void
finish_completeness(ntedit_hip_ctx* ctx, const std::string& prefix, uint32_t k, bool report)
{
	const std::string cp_path = prefix + "_completeness.tsv";
	ntedit_hip_shared_stats ss;
	if (ntedit_hip_shared_counts(ctx, &ss) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	char rows[2][512];
	FILE* cf = fopen(cp_path.c_str(), "wb");
	bool ok = cf != nullptr && ntedit_hip_completeness_format_row("before", &ss, 0, rows[0], sizeof rows[0]) == 0 &&
	          ntedit_hip_completeness_format_row("after", &ss, 1, rows[1], sizeof rows[1]) == 0 &&
	          fputs(ntedit_hip_completeness_header(), cf) >= 0 && fputs(rows[0], cf) >= 0 && fputs(rows[1], cf) >= 0;
	if (cf) {
		ok = fclose(cf) == 0 && ok;
	}
	if (!ok) {
		fail("cannot write `%s'", cp_path.c_str());
	}
	const double filter_kmers = ntedit_hip_bloom_cardinality(ss.filter_set, ss.bits, ss.hash_num);
	const double shared_kmers[2] = { ntedit_hip_bloom_cardinality(ss.shared_set[0], ss.bits, 1),
		                             ntedit_hip_bloom_cardinality(ss.shared_set[1], ss.bits, 1) };
	auto share = [&](int w) { // (the ratio of two estimates; NaN where the table says NA)
		return std::isfinite(filter_kmers) && std::isfinite(shared_kmers[w]) && filter_kmers != 0 ? shared_kmers[w] / filter_kmers : std::nan("");
	};
	const double fpr = ss.bits ? pow((double)ss.filter_set / (double)ss.bits, (double)ss.hash_num) : 0.0;
	printf("k-mer completeness (k=%u): before %s (%s of the filter's %s k-mers in the draft), after %s (%s); draft k-mers the filter "
	       "holds only as false positives are counted too, at most about fpr / (1 - fpr) of the absent k-mers (occupancy^h = %.3g); "
	       "table: %s\n",
	       k, percent_text(share(0)).c_str(), count_text(shared_kmers[0]).c_str(), count_text(filter_kmers).c_str(),
	       percent_text(share(1)).c_str(), count_text(shared_kmers[1]).c_str(), fpr, cp_path.c_str());
	if (report) {
		printf("{\"completeness\": {\"filter_bits\": %llu, \"filter_set\": %llu, \"filter_kmers\": %s, \"shared_set_before\": %llu, "
		       "\"shared_kmers_before\": %s, \"shared_set_after\": %llu, \"shared_kmers_after\": %s, \"completeness_before\": %s, "
		       "\"completeness_after\": %s, \"ms_mark\": [%.3f, %.3f]}}\n",
		       (unsigned long long)ss.bits, (unsigned long long)ss.filter_set, json_num(std::round(filter_kmers), "%.0f").c_str(),
		       (unsigned long long)ss.shared_set[0], json_num(std::round(shared_kmers[0]), "%.0f").c_str(), (unsigned long long)ss.shared_set[1],
		       json_num(std::round(shared_kmers[1]), "%.0f").c_str(), json_num(share(0), "%.6f").c_str(), json_num(share(1), "%.6f").c_str(),
		       ss.ms_mark[0], ss.ms_mark[1]);
	}
}

void
finish_bgzip(const RoundTotals& t, const std::string& fa_path, bool report)
{
	const double ratio = t.bgzf_bytes ? (double)t.bgzf_plain / (double)t.bgzf_bytes : 0.0;
	printf("BGZF: %llu plain bytes in %llu BGZF bytes (ratio %.3f), %llu members, %llu of them stored; file: %s\n", t.bgzf_plain, t.bgzf_bytes,
	       ratio, t.bgzf_members, t.bgzf_stored, fa_path.c_str());
	if (report) {
		printf("{\"bgzip\": {\"plain_bytes\": %llu, \"bgzf_bytes\": %llu, \"members\": %llu, \"stored_members\": %llu, \"image_ms\": %.3f, "
		       "\"deflate_ms\": %.3f, \"copy_ms\": %.3f}}\n",
		       t.bgzf_plain, t.bgzf_bytes, t.bgzf_members, t.bgzf_stored, t.ms_bgzf_image, t.ms_bgzf_deflate, t.ms_bgzf_copy);
	}
}

void
finish_bed(const RoundTotals& t, const std::string paths[2], bool report)
{
	printf("unsupported regions: before %llu intervals over %llu bases, after %llu over %llu; tracks: %s, %s\n", t.bed_intervals[0],
	       t.bed_bases[0], t.bed_intervals[1], t.bed_bases[1], paths[0].c_str(), paths[1].c_str());
	if (report) {
		printf("{\"bed\": {\"intervals_before\": %llu, \"bases_before\": %llu, \"intervals_after\": %llu, \"bases_after\": %llu, "
		       "\"extract_before_ms\": %.3f, \"extract_after_ms\": %.3f}}\n",
		       t.bed_intervals[0], t.bed_bases[0], t.bed_intervals[1], t.bed_bases[1], t.ms_track[0], t.ms_track[1]);
	}
}

// the figures of one spectrum: occurrences, those at 0 and at 255, the sum of the multiplicities, and the peak -- the
// smallest multiplicity in 1..254 with the largest bin (-1: all of those bins are empty)
struct SpectrumFigures
{
	unsigned long long kmers = 0, zero = 0, saturated = 0, sum = 0;
	int peak = -1;
};

static SpectrumFigures
spectrum_figures(const unsigned long long bins[256])
{
	SpectrumFigures f;
	unsigned long long best = 0;
	for (int c = 0; c < 256; c++) {
		f.kmers += bins[c];
		f.sum += bins[c] * (unsigned long long)c;
		if (c >= 1 && c <= 254 && bins[c] > best) {
			best = bins[c];
			f.peak = c;
		}
	}
	f.zero = bins[0];
	f.saturated = bins[255];
	return f;
}

void
finish_spectrum(const RoundTotals& t, FILE* depth_f, const std::string paths[2], uint32_t k, bool report)
{
	char line[512];
	bool ok = ntedit_hip_depth_format_row("#total", &t.depth, line, sizeof line) == 0 && fputs(line, depth_f) >= 0;
	ok = fclose(depth_f) == 0 && ok;
	if (!ok) {
		fail("cannot write `%s'", paths[1].c_str());
	}
	FILE* sf = fopen(paths[0].c_str(), "wb");
	ok = sf != nullptr && fputs(ntedit_hip_spectrum_header(), sf) >= 0;
	for (uint32_t c = 0; ok && c < 256; c++) {
		ok = ntedit_hip_spectrum_format_row(c, t.spectrum[0][c], t.spectrum[1][c], line, sizeof line) == 0 && fputs(line, sf) >= 0;
	}
	if (sf) {
		ok = fclose(sf) == 0 && ok;
	}
	if (!ok) {
		fail("cannot write `%s'", paths[0].c_str());
	}
	const SpectrumFigures f[2] = { spectrum_figures(t.spectrum[0]), spectrum_figures(t.spectrum[1]) };
	auto share = [](unsigned long long part, unsigned long long all) { return all ? (double)part / (double)all : std::nan(""); };
	auto mean = [](const SpectrumFigures& g) { return g.kmers ? (double)g.sum / (double)g.kmers : std::nan(""); };
	auto mean_text = [&](const SpectrumFigures& g) { return g.kmers ? json_num(mean(g), "%.2f") : std::string("NA"); };
	auto peak_text = [](const SpectrumFigures& g) { return g.peak < 0 ? std::string("NA") : std::to_string(g.peak); };
	printf("k-mer spectrum (k=%u): before %llu k-mers, %s at multiplicity 0, mean %s, peak %s, %s saturated; after %llu k-mers, %s at "
	       "multiplicity 0, mean %s, peak %s, %s saturated; tables: %s, %s\n",
	       k, f[0].kmers, percent_text(share(f[0].zero, f[0].kmers)).c_str(), mean_text(f[0]).c_str(), peak_text(f[0]).c_str(),
	       percent_text(share(f[0].saturated, f[0].kmers)).c_str(), f[1].kmers, percent_text(share(f[1].zero, f[1].kmers)).c_str(),
	       mean_text(f[1]).c_str(), peak_text(f[1]).c_str(), percent_text(share(f[1].saturated, f[1].kmers)).c_str(), paths[0].c_str(),
	       paths[1].c_str());
	if (report) {
		auto peak_json = [](const SpectrumFigures& g) { return g.peak < 0 ? std::string("null") : std::to_string(g.peak); };
		printf("{\"spectrum\": {\"kmers_before\": %llu, \"zero_before\": %llu, \"mean_before\": %s, \"peak_before\": %s, \"saturated_before\": %llu, "
		       "\"kmers_after\": %llu, \"zero_after\": %llu, \"mean_after\": %s, \"peak_after\": %s, \"saturated_after\": %llu, "
		       "\"spectrum_before_ms\": %.3f, \"spectrum_after_ms\": %.3f}}\n",
		       f[0].kmers, f[0].zero, json_num(mean(f[0]), "%.4f").c_str(), peak_json(f[0]).c_str(), f[0].saturated, f[1].kmers, f[1].zero,
		       json_num(mean(f[1]), "%.4f").c_str(), peak_json(f[1]).c_str(), f[1].saturated, t.ms_spectrum[0], t.ms_spectrum[1]);
	}
}

// --cn: counts the draft store, writes both tables and says what they hold.  A store that was released (its cap, or no
// memory) costs one line on standard error and no file; the run goes on.
void
finish_cn(ntedit_hip_ctx* ctx, const std::vector<std::string>& names, const std::string paths[2], uint32_t k, unsigned long long sketch,
          bool report)
{
	ntedit_hip_cn_stats st;
	const int rc = ntedit_hip_cn_finish(ctx, sketch);
	if (ntedit_hip_cn_info(ctx, &st) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	static const char* const STATES[] = { "off", "on", "over_cap", "no_memory" };
	const char* state = st.state < 4 ? STATES[st.state] : "unknown";
	if (rc == NTEDIT_E_OVERFLOW) {
		fprintf(stderr, PROGRAM ": --cn: %s; no copy-number table is written (--cn_store BYTES raises the cap)\n", ntedit_hip_last_error(ctx));
		if (report) {
			printf("{\"cn\": {\"state\": \"%s\", \"store_cap\": %llu}}\n", state, (unsigned long long)st.cap);
		}
		return;
	}
	if (rc != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	std::vector<uint64_t> occ[2], w5[2], distinct[2];
	std::vector<ntedit_hip_cn_row> rows[2];
	for (int which = 0; which < 2; which++) {
		occ[which].resize(5 * 256);
		w5[which].resize(256);
		distinct[which].resize(5 * 256);
		rows[which].resize(names.size());
		if (ntedit_hip_cn_table(ctx, which, occ[which].data(), w5[which].data()) != 0 ||
		    ntedit_hip_cn_rows(ctx, which, rows[which].data(), names.size()) != 0 ||
		    ntedit_hip_cn_distinct(occ[which].data(), w5[which].data(), distinct[which].data()) != 0) {
			fail("%s", ntedit_hip_last_error(ctx));
		}
	}
	char line[1024];
	FILE* f = fopen(paths[0].c_str(), "wb");
	bool ok = f != nullptr && fputs(ntedit_hip_cn_header(), f) >= 0;
	for (uint32_t m = 0; ok && m < 256; m++) {
		ok = ntedit_hip_cn_format_row(m, distinct[0].data(), distinct[1].data(), line, sizeof line) == 0 && fputs(line, f) >= 0;
	}
	if (f) {
		ok = fclose(f) == 0 && ok;
	}
	if (!ok) {
		fail("cannot write `%s'", paths[0].c_str());
	}
	f = fopen(paths[1].c_str(), "wb");
	ok = f != nullptr && fputs(ntedit_hip_cn_contig_header(), f) >= 0;
	ntedit_hip_cn_row total[2] = {};
	std::string text;
	for (size_t i = 0; ok && i <= names.size(); i++) {
		const bool last = i == names.size();
		for (int which = 0; which < 2 && !last; which++) {
			total[which].kmers += rows[which][i].kmers;
			total[which].cn1 += rows[which][i].cn1;
			total[which].cn2 += rows[which][i].cn2;
			total[which].cn3 += rows[which][i].cn3;
			total[which].cn4 += rows[which][i].cn4;
			total[which].cn5plus += rows[which][i].cn5plus;
		}
		const char* name = last ? "#total" : names[i].c_str();
		text.resize(strlen(name) + 512);
		ok = ntedit_hip_cn_contig_format_row(name, last ? &total[0] : &rows[0][i], last ? &total[1] : &rows[1][i], &text[0], text.size()) == 0 &&
		     fputs(text.c_str(), f) >= 0;
	}
	if (f) {
		ok = fclose(f) == 0 && ok;
	}
	if (!ok) {
		fail("cannot write `%s'", paths[1].c_str());
	}
	// per side: the distinct k-mers, the single-copy share of them, the share of occurrences with cn >= 2, and the share of
	// copy numbers a collision is expected to have inflated, (non-zero counters / counters)^h
	unsigned long long n_distinct[2] = { 0, 0 }, single[2] = { 0, 0 }, n_occ[2] = { 0, 0 }, multi[2] = { 0, 0 };
	double inflated[2];
	uint32_t fk = 0, h = 1;
	uint64_t fbytes = 0;
	int fcounting = 0;
	if (ntedit_hip_filter_info(ctx, 0, &fk, &h, &fbytes, &fcounting) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	for (int which = 0; which < 2; which++) {
		for (int c = 0; c < 5; c++) {
			for (int m = 0; m < 256; m++) {
				n_distinct[which] += distinct[which][c * 256 + m];
				n_occ[which] += occ[which][c * 256 + m];
				if (c == 0) {
					single[which] += distinct[which][m];
				} else {
					multi[which] += occ[which][c * 256 + m];
				}
			}
		}
		inflated[which] = st.counters ? std::pow((double)st.nonzero[which] / (double)st.counters, (double)h) : std::nan("");
	}
	auto share = [](unsigned long long part, unsigned long long all) { return all ? (double)part / (double)all : std::nan(""); };
	printf("k-mer copy numbers (k=%u): before %llu distinct k-mers, %s single-copy, %s of occurrences at copy number 2 or more; after %llu "
	       "distinct k-mers, %s single-copy, %s of occurrences at copy number 2 or more; sketch %llu counters, expected inflated %s before, %s "
	       "after; tables: %s, %s\n",
	       k, n_distinct[0], percent_text(share(single[0], n_distinct[0])).c_str(), percent_text(share(multi[0], n_occ[0])).c_str(), n_distinct[1],
	       percent_text(share(single[1], n_distinct[1])).c_str(), percent_text(share(multi[1], n_occ[1])).c_str(), (unsigned long long)st.counters,
	       percent_text(inflated[0]).c_str(), percent_text(inflated[1]).c_str(), paths[0].c_str(), paths[1].c_str());
	if (report) {
		printf("{\"cn\": {\"state\": \"%s\", \"store_cap\": %llu, \"store_bytes_before\": %llu, \"store_bytes_after\": %llu, "
		       "\"distinct_before\": %llu, \"single_copy_before\": %llu, \"occurrences_before\": %llu, \"multi_copy_occurrences_before\": %llu, "
		       "\"distinct_after\": %llu, \"single_copy_after\": %llu, \"occurrences_after\": %llu, \"multi_copy_occurrences_after\": %llu, "
		       "\"sketch_counters\": %llu, \"nonzero_before\": %llu, \"nonzero_after\": %llu, \"inflated_before\": %s, \"inflated_after\": %s, "
		       "\"cn_count_before_ms\": %.3f, \"spectrum_cn_before_ms\": %.3f, \"cn_count_after_ms\": %.3f, \"spectrum_cn_after_ms\": %.3f}}\n",
		       state, (unsigned long long)st.cap, (unsigned long long)st.bytes[0], (unsigned long long)st.bytes[1], n_distinct[0], single[0], n_occ[0],
		       multi[0], n_distinct[1], single[1], n_occ[1], multi[1], (unsigned long long)st.counters, (unsigned long long)st.nonzero[0],
		       (unsigned long long)st.nonzero[1], json_num(inflated[0], "%.6g").c_str(), json_num(inflated[1], "%.6g").c_str(), st.ms[0], st.ms[1],
		       st.ms[2], st.ms[3]);
	}
}

void
report_qv(const RoundTotals& t)
{
	printf("{\"qv\": {\"kmers_before\": %llu, \"absent_before\": %llu, \"kmers_after\": %llu, \"absent_after\": %llu, \"apply_ms\": %.3f, "
	       "\"screen_ms\": %.3f, \"count_ms\": %.3f}}\n",
	       (unsigned long long)t.qv.kmers_before, (unsigned long long)t.qv.absent_before, (unsigned long long)t.qv.kmers_after,
	       (unsigned long long)t.qv.absent_after, t.ms_apply, t.ms_qv_screen, t.ms_qv_count);
}

void
report_round(const RoundTotals& t)
{
	printf("{\"bases\": %llu, \"seconds\": %.6f, \"open_outputs_s\": %.3f, \"index_s\": %.3f, \"read_s\": %.3f, \"polish_call_s\": %.3f, \"write_s\": %.3f, \"gpu_ms\": %.3f, \"screen_ms\": %.3f, \"machine_ms\": %.3f, "
	       "\"screening\": {\"batches_partitioned\": %u, \"batches_direct_kernel\": %u, \"record_chunks_rescreened_direct\": %u, \"overflow_records\": %llu}, \"events\": %llu, "
	       "\"events_applied\": %llu, \"absent_kmers\": %llu, \"substitutions\": %llu, \"insertions\": %llu, "
	       "\"deletions\": %llu}\n",
	       t.bases, t.seconds, t.s_before_index, t.s_index, t.s_read, t.s_call, t.s_write, t.ms_gpu, t.ms_screen, t.ms_machine,
	       t.n_batches_binned, t.n_batches_direct, t.n_chunks_direct, t.n_ovf_records, (unsigned long long)t.events.events,
	       (unsigned long long)t.events.events_applied, (unsigned long long)t.events.absent_kmers,
	       (unsigned long long)t.events.substitutions, (unsigned long long)t.events.insertions,
	       (unsigned long long)t.events.deletions);
}

} // namespace nte_cli
