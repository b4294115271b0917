// reads_build.cpp -- the reads filter build as ntedit-make-reads-bf, the sharded driver (ntedit_amd/make_reads.py) and
// `ntedit --reads` run it: the sketch, pass 1, the histogram pass, the decision about cutoff and sizes, and pass 2, in four
// stages that the tool walks in one call (ntedit_hip_reads_build) and the driver one by one with its merges in between; the
// build's console lines; and the --hist writer.  The passes themselves are ntedit_hip_reads_pass (reads_pass.cpp).
#include "../csrc/nte_reads_internal.h"

#include <chrono>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

namespace {

const uint64_t WHOLE = ~0ull; // `end` of a range that runs to the end of its file

int
pfail(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return nte_reads::set_error(c, code, why); // (ntedit_hip_reads_last_error's store, nte_reads.hip)
}

// the build's console lines; a rank's share of a sharded build (ranges) names the rank on its pass and store lines, and
// only rank 0 (the one process of an unsharded build is rank 0) says what every rank decides alike
struct BuildLog
{
	const ntedit_hip_reads_build_args* a;
	bool first_only = false;
	bool ranged() const { return a->begins != nullptr; }
	void rank_info(const std::string& s) const
	{
		info(ranged() ? "rank " + std::to_string(a->rank) + "/" + std::to_string(a->world) + ": " + s : s);
	}
	void info(const std::string& s) const { line(0, s); }
	void out(const std::string& s) const { line(1, s); }
	void line(int to_stdout, const std::string& s) const
	{
		if (a->log && !(first_only && a->rank != 0)) {
			a->log(a->user, to_stdout, s.c_str());
		}
	}
};

// one pass, over the ranges (the files whole) or over the resident store (the store's bases: pass 1's), and its line
// (the large-run tests read it).  Pass 1 reads the store only when the build began with one (r->from_store, set by
// stage_count from the store's state at entry); the later passes whenever the store is ON.
int
build_pass(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, int pass, ntedit_hip_reads_build_result* r, uint64_t* starts,
           uint64_t* nexts)
{
	static const char* const names[] = { "1 (count)", "H (histogram)", "2 (solid k-mers)" };
	const BuildLog lg{ a };
	ntedit_hip_reads_pass_stats& st = r->pass[pass];
	std::string what;
	int rc;
	const bool from_store = r->from_store != 0;
	uint64_t store_bases = 0; // of a store the build began with: its bytes, reads and separators (nobody kept its reads' bases)
	if (from_store) {
		ntedit_hip_resident_stats ss;
		if (ntedit_hip_resident_info(ctx, &ss) != 0) {
			return NTEDIT_E_DEVICE;
		}
		store_bases = ss.bases;
	}
	const bool read_files = r->store_state != NTEDIT_RESIDENT_ON || (pass == NTEDIT_READS_PASS_COUNT && !from_store);
	if (!read_files) {
		const auto t0 = std::chrono::steady_clock::now();
		rc = pass == NTEDIT_READS_PASS_COUNT  ? ntedit_hip_resident_count(ctx)
		     : pass == NTEDIT_READS_PASS_HIST ? ntedit_hip_resident_histogram(ctx)
		     : a->reject_cmin               ? ntedit_hip_resident_insert_solid2(ctx, r->cmin, a->reject_cmin)
		                                    : ntedit_hip_resident_insert_solid(ctx, NTEDIT_FILTER_PRIMARY, r->cmin);
		st.bases = from_store ? store_bases : r->pass[NTEDIT_READS_PASS_COUNT].bases;
		st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		st.ms_gpu = st.ms_wall;
		what = std::to_string(r->store_batches) + " batches of the resident store";
	} else {
		const std::vector<uint64_t> begins(a->n_files, 0), ends(a->n_files, WHOLE);
		rc = ntedit_hip_reads_pass(ctx, pass, a->files, lg.ranged() ? a->begins : begins.data(), lg.ranged() ? a->ends : ends.data(),
		                           a->n_files, a->batch_bytes, r->cmin, &st, starts, nexts);
		what = std::to_string(a->n_files) + " ranges";
	}
	if (rc != 0) {
		return NTEDIT_E_IO; // (the message is the pass's)
	}
	char line[256];
	snprintf(line, sizeof line, "Pass %s: %llu bases, %.1f ms, %.3f Gbases/s (GPU calls %.1f ms, %.3f Gbases/s)", names[pass],
	         (unsigned long long)st.bases, st.ms_wall, st.ms_wall > 0 ? st.bases / st.ms_wall / 1e6 : 0.0, st.ms_gpu,
	         st.ms_gpu > 0 ? st.bases / st.ms_gpu / 1e6 : 0.0);
	lg.rank_info(lg.ranged() || from_store ? line + (", " + what) : line);
	uint64_t qual_bases = 0, masked_bases = 0;
	if (a->min_qual && read_files && ntedit_hip_reads_min_qual_info(ctx, &qual_bases, &masked_bases) == 0) {
		// the pass's one line about --min_qual (the tests read it)
		lg.rank_info("--min_qual " + std::to_string(a->min_qual) + ": " + std::to_string(masked_bases) + " of " + std::to_string(qual_bases) +
		             " bases with a quality masked");
	}
	ntedit_hip_reads_read_filter_stats fs;
	uint32_t f_len = 0, f_mean = 0;
	float f_rq = 0.0f;
	if (read_files && ntedit_hip_reads_get_read_filter(ctx, &f_len, &f_mean, &f_rq) == 0 && (f_len || f_mean || f_rq > 0.0f) &&
	    ntedit_hip_reads_read_filter_info(ctx, &fs) == 0) {
		// the pass's one line about the read filter (the tests read it)
		lg.rank_info("read filter: " + std::to_string(fs.dropped_length + fs.dropped_rq + fs.dropped_mean_qual) + " of " +
		             std::to_string(fs.records) + " records dropped (length " + std::to_string(fs.dropped_length) + ", rq " +
		             std::to_string(fs.dropped_rq) + ", mean quality " + std::to_string(fs.dropped_mean_qual) + ")" +
		             (f_rq > 0.0f && fs.rq_tagged == 0 ? "; --min_rq: no record had an rq tag" : "") +
		             (fs.aux_malformed ? "; " + std::to_string(fs.aux_malformed) + " records with malformed aux fields" : ""));
	}
	ntedit_hip_reads_parse_stats ps;
	if (a->device_parse && read_files && ntedit_hip_reads_parse_info(ctx, &ps) == 0) {
		// the pass's one line about --gpu_parse (the tests read it)
		std::string l = "--gpu_parse: " + std::to_string(ps.device_chunks) + " chunks parsed on the device (" + std::to_string(ps.raw_bytes) +
		                " raw bytes, " + std::to_string(ps.text_bytes) + " text bytes, ";
		snprintf(line, sizeof line, "%.1f ms in the parse kernels)", ps.ms_kernels);
		l += line;
		if (ps.fallback_chunks) {
			static const char* const rules[] = { "the first byte is neither '>' nor '@'", "a carriage return", "an empty line",
				                                 "a sequence line that starts with '>', '+' or '@'", "FASTQ lines not a multiple of 4",
				                                 "a FASTQ header without '@'", "a FASTQ line 3 without '+'",
				                                 "a quality line not as long as its sequence", "more than one line per 8 bytes",
				                                 "a chunk of 2 GiB or more" };
			std::string whys;
			for (int b = 0; b < 10; b++) {
				if (ps.broken & (1u << b)) {
					whys += (whys.empty() ? "" : "; ") + std::string(rules[b]);
				}
			}
			l += ", " + std::to_string(ps.fallback_chunks) + " unclean chunks sent the rest of their ranges to the host parser (" + whys + ")";
		}
		if (ps.host_files) {
			l += ", " + std::to_string(ps.host_files) + " gzip inputs stay with the host parser";
		}
		lg.rank_info(l);
		ntedit_hip_reads_inflate_stats zs;
		if (ntedit_hip_reads_inflate_info(ctx, &zs) == 0 && zs.files) {
			// ... and one about its BGZF inputs (the tests read it)
			l = "--gpu_parse: BGZF: " + std::to_string(zs.members) + " members of " + std::to_string(zs.files) +
			    (zs.files == 1 ? " file" : " files") + " inflated on the device (" + std::to_string(zs.comp_bytes) +
			    " compressed bytes, " + std::to_string(zs.raw_bytes) + " inflated bytes, ";
			snprintf(line, sizeof line, "%.1f ms in the inflate kernels), ", zs.ms_kernels);
			l += line + std::to_string(zs.handed_back) + (zs.handed_back == 1 ? " file" : " files") + " handed back";
			if (zs.handed_back) {
				l += " to the host parser (the last at inflated offset " + std::to_string(zs.handed_back_at) + ")";
			}
			l += "; " + std::to_string(ps.host_files) + " gzip inputs stay with the host parser";
			lg.rank_info(l);
		}
		ntedit_hip_reads_bam_stats bs;
		if (ntedit_hip_reads_bam_info(ctx, &bs) == 0 && bs.files) {
			// ... and one about its BAM inputs (the tests read it)
			l = "--gpu_parse: BAM: " + std::to_string(bs.records) + " records of " + std::to_string(bs.files) +
			    (bs.files == 1 ? " file" : " files") + " walked on the device (" + std::to_string(bs.kept) + " kept, " +
			    std::to_string(bs.skipped_flag) + " secondary or supplementary, " + std::to_string(bs.skipped_short) + " too short; " +
			    std::to_string(bs.chunks) + " chunks, " + std::to_string(bs.segments) + " segments, " + std::to_string(bs.rewalked) +
			    " walked again by the stitch, ";
			snprintf(line, sizeof line, "%.1f ms in the walk kernels, %.1f ms in the decode kernels)", bs.ms_walk, bs.ms_decode);
			lg.rank_info(l + line);
		}
	}
	return 0;
}

// the end of a build: the sketch freed and the store with it, or (keep_store, the build succeeded and its store is ON)
// the counters alone released and the store kept for the next build
void
end_build(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, const ntedit_hip_reads_build_result* r, int rc)
{
	if (rc == 0 && a && r && a->keep_store && r->store_state == NTEDIT_RESIDENT_ON && ntedit_hip_sketch_reset(ctx, 0, 0, 0) == 0) {
		return;
	}
	ntedit_hip_sketch_free(ctx);
}

bool
bad_build_args(const ntedit_hip_reads_build_args* a, const ntedit_hip_reads_build_result* r)
{
	return !a || !r || (a->n_files && !a->files) || (a->begins && !a->ends) || a->batch_bytes < 4096 || a->min_qual > 93 ||
	       (!a->solid && (a->cmin < 1 || a->cmin > 255)) || (a->bf_bytes == 0 && !a->solid && !a->hist_path) ||
	       (a->reject_cmin && (a->reject_cmin > 255 || a->counts || (a->reject_bf_bytes == 0 && !a->solid && !a->hist_path)));
}

} // namespace

extern "C" {

int
ntedit_hip_reads_stage_count(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r,
                             uint64_t* starts, uint64_t* nexts)
{
	if (!ctx || bad_build_args(a, r)) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_count: bad argument");
	}
	const BuildLog lg{ a };
	*r = ntedit_hip_reads_build_result();
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	ntedit_hip_reads_set_min_qual(ctx, a->min_qual);
	// a store an earlier build left ON (keep_store): this build's three passes read it, and no file is opened
	ntedit_hip_resident_stats at_entry;
	const bool from_store = !lg.ranged() && a->use_store && ntedit_hip_resident_info(ctx, &at_entry) == 0 &&
	                        at_entry.state == NTEDIT_RESIDENT_ON;
	if (from_store) {
		if (ntedit_hip_sketch_reset(ctx, a->sketch_counters, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE; // (the message is sketch_reset's)
		}
		r->from_store = 1;
		r->store_state = at_entry.state; // (build_pass routes by both)
		r->store_batches = at_entry.batches;
	} else {
		if (!lg.ranged() && ntedit_hip_sketch_alloc(ctx, a->sketch_counters, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE; // (the message is sketch_alloc's)
		}
		if (ntedit_hip_reads_set_min_read(ctx, a->min_read) != 0) {
			return NTEDIT_E_DEVICE;
		}
		if (a->use_store && ntedit_hip_resident_begin(ctx, a->store_cap) != 0) {
			return NTEDIT_E_DEVICE;
		}
	}
	lg.rank_info("Pass 1: counting k-mers");
	if (build_pass(ctx, a, NTEDIT_READS_PASS_COUNT, r, starts, nexts) != 0) {
		return NTEDIT_E_IO;
	}
	if (a->use_store) {
		ntedit_hip_resident_stats ss;
		if (ntedit_hip_resident_info(ctx, &ss) != 0) {
			return NTEDIT_E_DEVICE;
		}
		r->store_state = ss.state;
		r->store_bytes = ss.bytes;
		r->store_batches = ss.batches;
		const std::string later = a->solid || a->hist_path ? "the histogram pass and pass 2" : "pass 2";
		if (from_store) {
			lg.rank_info("Resident store: kept from the build before, " + std::to_string(ss.batches) + " batches, " + std::to_string(ss.bytes) +
			             " bytes of HBM (3 bits per base); every pass of this build reads it, no file is opened");
		} else if (ss.state == NTEDIT_RESIDENT_ON) {
			lg.rank_info("Resident store: " + std::to_string(ss.batches) + " batches, " + std::to_string(ss.bytes) +
			             " bytes of HBM (3 bits per base); " + later + " read it");
		} else {
			lg.rank_info(std::string("Resident store: released (") +
			             (ss.state == NTEDIT_RESIDENT_OVER_CAP ? "the reads would pass its cap of " + std::to_string(ss.cap) + " bytes"
			                                                      : std::string("a device allocation failed")) +
			             "); " + later + " read the files");
		}
	}
	return 0;
}

int
ntedit_hip_reads_stage_histogram(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r,
                                 uint64_t occ[256])
{
	if (!ctx || bad_build_args(a, r) || !occ) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_histogram: bad argument");
	}
	const BuildLog lg{ a };
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	ntedit_hip_reads_set_min_qual(ctx, a->min_qual);
	lg.rank_info("Histogram pass: the k-mer histogram of the sketch's estimates");
	if (build_pass(ctx, a, NTEDIT_READS_PASS_HIST, r, nullptr, nullptr) != 0) {
		return NTEDIT_E_IO;
	}
	return ntedit_hip_sketch_histogram_download(ctx, occ) != 0 ? NTEDIT_E_DEVICE : 0;
}

int
ntedit_hip_reads_stage_decide(const ntedit_hip_reads_build_args* a, const uint64_t occ[256], ntedit_hip_reads_build_result* r)
{
	if (bad_build_args(a, r) || (!occ && (a->solid || a->bf_bytes == 0 || (a->reject_cmin && a->reject_bf_bytes == 0)))) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_stage_decide: bad argument");
	}
	const BuildLog lg{ a, true };
	r->cmin = a->cmin;
	r->bf_bytes = a->bf_bytes;
	r->reject_bf_bytes = a->reject_cmin ? a->reject_bf_bytes : 0;
	const std::string reject = "--reject_cutoff " + std::to_string(a->reject_cmin);
	if (occ) {
		uint64_t f[256], F0 = 0, F1 = 0;
		ntedit_hip_reads_hist_summary(occ, f, &F0, &F1);
		lg.info("k-mer histogram: F1 = " + std::to_string(F1) + " (k-mers), F0 = " + std::to_string(F0) + " (distinct k-mers)");
		// written first: a refused --solid still leaves the histogram to look at
		if (a->hist_path && a->rank == 0) {
			if (ntedit_hip_reads_write_hist(a->hist_path, f, F0, F1) != 0) {
				return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + a->hist_path);
			}
			lg.info(std::string("Histogram written to ") + a->hist_path);
		}
		if (a->solid) {
			if (ntedit_hip_reads_solid_cutoff(f, &r->cmin) != 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "--solid: the k-mer histogram has no valley after the error peak (no c with "
				                                    "f[c+1] > f[c]); pass -c");
			}
			lg.info("--solid: minimum k-mer count " + std::to_string(r->cmin));
			if (a->reject_cmin && a->reject_cmin <= r->cmin) {
				return pfail(nullptr, NTEDIT_E_ARG, reject + ": the reject count must be above the minimum count, and --solid found " +
				                                        std::to_string(r->cmin));
			}
		}
		if (a->reject_cmin && a->reject_bf_bytes == 0) {
			uint64_t num_elements = 0;
			for (uint64_t c = a->reject_cmin; c < 256; c++) {
				num_elements += f[c];
			}
			r->reject_bf_bytes = ntedit_hip_reads_bf_size(num_elements, a->hash_num, a->fpr);
			lg.info("Reject filter sized from the k-mer histogram: --reject_num_elements " + std::to_string(num_elements) + " (k-mers at " +
			        std::to_string(a->reject_cmin) + " or above), " + std::to_string(r->reject_bf_bytes) + " bytes");
			if (r->reject_bf_bytes == 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "The reject filter would be empty (no k-mer at " + reject + " or above).");
			}
			lg.out("Reject BF size (bytes): " + std::to_string(r->reject_bf_bytes));
		}
		if (a->bf_bytes == 0) {
			uint64_t num_elements = 0;
			for (uint64_t c = r->cmin; c < 256; c++) {
				num_elements += f[c];
			}
			r->bf_bytes = ntedit_hip_reads_bf_size(num_elements, a->hash_num, a->fpr);
			lg.info("Sized from the k-mer histogram: --num_elements " + std::to_string(num_elements) + " (k-mers at " +
			        std::to_string(r->cmin) + " or above), " + std::to_string(r->bf_bytes) + " bytes");
			if (r->bf_bytes == 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "The output filter would be empty (no k-mer at the minimum count or above).");
			}
			lg.out("BF size (bytes): " + std::to_string(r->bf_bytes));
		}
	}
	if (r->bf_bytes == 0) {
		return pfail(nullptr, NTEDIT_E_ARG, "The output filter would be empty (--bf 0 or --num_elements too small).");
	}
	if (a->reject_cmin && a->reject_cmin <= r->cmin) {
		return pfail(nullptr, NTEDIT_E_ARG, reject + ": the reject count must be above the minimum count " + std::to_string(r->cmin));
	}
	if (a->reject_cmin && r->reject_bf_bytes == 0) {
		return pfail(nullptr, NTEDIT_E_ARG, "The reject filter would be empty (--reject_bf 0 or --reject_num_elements too small).");
	}
	return 0;
}

int
ntedit_hip_reads_stage_insert(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r)
{
	if (!ctx || bad_build_args(a, r) || r->bf_bytes == 0 || r->cmin < 1 || r->cmin > 255 ||
	    (a->reject_cmin && (r->reject_bf_bytes == 0 || a->reject_cmin <= r->cmin))) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_insert: bad argument");
	}
	const BuildLog lg{ a };
	if (lg.ranged()) { // (the filter is the one the caller adopted in the PRIMARY slot)
	} else if (a->counts) {
		if (ntedit_hip_filter_alloc_counting(ctx, NTEDIT_FILTER_PRIMARY, r->bf_bytes, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE;
		}
	} else if (ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_PRIMARY, r->bf_bytes, a->hash_num, a->k) != 0) {
		return pfail(ctx, NTEDIT_E_DEVICE, ntedit_hip_last_error(ctx));
	}
	// the reject filter: plain, same k and hash count, in the SECONDARY slot (a sharded build: the adopted one)
	if (a->reject_cmin && !lg.ranged() &&
	    ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_SECONDARY, r->reject_bf_bytes, a->hash_num, a->k) != 0) {
		return pfail(ctx, NTEDIT_E_DEVICE, ntedit_hip_last_error(ctx));
	}
	if (a->reject_cmin && ntedit_hip_reads_set_reject_cutoff(ctx, a->reject_cmin) != 0) { // (for a pass 2 over the files)
		return NTEDIT_E_ARG;
	}
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	ntedit_hip_reads_set_min_qual(ctx, a->min_qual);
	lg.rank_info("Pass 2: inserting k-mers seen at least " + std::to_string(r->cmin) + " times" +
	             (a->reject_cmin ? ", and into the reject filter those seen at least " + std::to_string(a->reject_cmin) + " times" : ""));
	const int rc = build_pass(ctx, a, NTEDIT_READS_PASS_SOLID, r, nullptr, nullptr);
	end_build(ctx, a, r, rc);
	return rc;
}

int
ntedit_hip_reads_build(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r)
{
	const auto t0 = std::chrono::steady_clock::now();
	uint64_t occ[256], nonzero = 0, counters = 0;
	const bool hist = a && (a->solid || a->hist_path);
	int rc = ntedit_hip_reads_stage_count(ctx, a, r, nullptr, nullptr);
	if (rc == 0 && ntedit_hip_sketch_occupancy(ctx, &nonzero, &counters) != 0) {
		rc = NTEDIT_E_DEVICE;
	}
	if (rc == 0) {
		std::ostringstream o;
		o << "Sketch occupancy: " << nonzero << " / " << counters << " counters (" << (double)nonzero / (double)counters << ")";
		BuildLog{ a }.out(o.str());
		if (a->sketch_path && ntedit_hip_sketch_save_file(ctx, a->sketch_path) != 0) {
			rc = NTEDIT_E_IO;
		}
	}
	if (rc == 0 && hist) {
		rc = ntedit_hip_reads_stage_histogram(ctx, a, r, occ);
	}
	if (rc == 0 && (rc = ntedit_hip_reads_stage_decide(a, hist ? occ : nullptr, r)) != 0) {
		pfail(ctx, rc, ntedit_hip_reads_last_error(nullptr)); // (the message of a call without a context, to the context's)
	}
	if (rc == 0) {
		rc = ntedit_hip_reads_stage_insert(ctx, a, r);
	}
	if (ctx) {
		end_build(ctx, a, r, rc);
	}
	if (r) {
		r->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	return rc;
}

} // extern "C"

extern "C" {

// ntCard's histogram file: "F1\t<n>", "F0\t<n>", then "c\tf[c]" for c = 1..255 (zeros included)
int
ntedit_hip_reads_write_hist(const char* path, const uint64_t f[256], uint64_t F0, uint64_t F1)
{
	if (!path || !f) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_write_hist: bad argument");
	}
	FILE* fp = fopen(path, "w");
	if (!fp) {
		return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + path);
	}
	fprintf(fp, "F1\t%llu\nF0\t%llu\n", (unsigned long long)F1, (unsigned long long)F0);
	for (int c = 1; c < 256; c++) {
		fprintf(fp, "%d\t%llu\n", c, (unsigned long long)f[c]);
	}
	const bool ok = !ferror(fp);
	if (fclose(fp) != 0 || !ok) {
		return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + path);
	}
	return 0;
}

} // extern "C"
