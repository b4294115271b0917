// cli_filter.cpp -- see cli_filter.h
#include "cli_filter.h"
#include "cli_common.h"
#include "log_info.h"

namespace nte_cli {

// saves a filter slot to a file and says so
static void
save_filter(ntedit_hip_ctx* ctx, int slot, const std::string& path, const char* label)
{
	if (path.empty()) {
		return;
	}
	if (ntedit_hip_filter_save_file(ctx, slot, path.c_str()) != 0) {
		fail("cannot write `%s'", path.c_str());
	}
	printf("%s saved to %s\n", label, path.c_str());
}

FilterStage
filter_from_genome(ntedit_hip_ctx* ctx, const CliOptions& o, const RoundNames& names)
{
	// built into the primary slot: sized as the tool sizes it, every k-mer of every record of k bases or more inserted;
	// without --gpu_parse the host parser reads the files (batch_bytes 0)
	const GenomeRules& gr = o.genome;
	printf("---------- building Bloom filter from genome        : %s\n", now_text());
	fflush(stdout);
	const Stopwatch clock;
	const uint64_t batch = gr.gpu_parse ? gr.batch_bytes : 0;
	auto pass = [&](int insert) {
		ntedit_hip_reads_pass_stats st;
		if (ntedit_hip_genome_pass(ctx, NTEDIT_FILTER_PRIMARY, o.paths.data(), (uint32_t)o.paths.size(), batch, insert, &st) != 0) {
			fail("%s", ntedit_hip_reads_last_error(ctx));
		}
		char line[1024];
		if (gr.gpu_parse && ntedit_hip_genome_pass_line(ctx, line, sizeof line) == 0) {
			fprintf(stderr, "%s pass: %llu bases, %.1f ms (GPU calls %.1f ms)\n%s\n", insert ? "Insert" : "Sizing",
			        (unsigned long long)st.bases, st.ms_wall, st.ms_gpu, line);
		}
		return st.bases;
	};
	uint64_t bf_size = gr.bf_bytes;
	if (!gr.have_bf && gr.have_ne) {
		bf_size = ntedit_hip_reads_bf_size(gr.num_elements, gr.hash_num, gr.fpr);
	} else if (!gr.have_bf) {
		const uint64_t genome_size = pass(0);
		printf("Genome size (bp): %llu\n", (unsigned long long)genome_size);
		bf_size = ntedit_hip_reads_bf_size(genome_size, gr.hash_num, gr.fpr);
		if (bf_size == 0) {
			fail("--genome: no bases in the genome files: the filter would be empty");
		}
	}
	printf("BF size (bytes): %llu\n", (unsigned long long)bf_size);
	if (ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_PRIMARY, bf_size, gr.hash_num, gr.k) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	(void)pass(1);
	ntedit_hip_sketch_free(ctx); // (the device parser's scratch: the polish sizes its own buffers next)
	printf("Genome filter built in %.1f ms\n", clock.ms());
	save_filter(ctx, NTEDIT_FILTER_PRIMARY, names.save_bf, "Bloom filter");
	FilterStage fs;
	fs.bf = names.save_bf.empty() ? "genome_bf.bf" : names.save_bf;
	fs.bfrep = o.bfrep;
	return fs;
}

// the sizes of the filters of a round, as the rules found them
static void
echo_reads_sizes(const ntedit_hip_reads_rules& rr)
{
	printf("BF size (bytes): ");
	if (rr.size_from_hist) {
		printf("from the k-mer histogram\n");
	} else {
		printf("%llu\n", (unsigned long long)rr.bf_bytes);
	}
	if (rr.reject_cmin && rr.reject_size_from_hist) {
		printf("Reject BF size (bytes): from the k-mer histogram\n");
	} else if (rr.reject_cmin) {
		printf("Reject BF size (bytes): %llu\n", (unsigned long long)rr.reject_bf_bytes);
	}
	printf("Sketch size (counters): %llu\n", (unsigned long long)rr.sketch_counters);
}

FilterStage
filter_from_reads(ntedit_hip_ctx* ctx, const CliOptions& o, size_t round, const RoundNames& names, bool* store_lost)
{
	// built into the primary slot; the reads stay resident in HBM after pass 1 unless they would pass store_cap, so that the
	// later passes do not parse them again
	const size_t n_rounds = o.rounds.size();
	const bool cascade = n_rounds > 1, last_round = round + 1 == n_rounds;
	const ntedit_hip_reads_rules& rr = o.rounds[round];
	if (cascade) {
		printf("---------- round %zu of %zu: k = %u\n", round + 1, n_rounds, rr.k);
	}
	printf("---------- building Bloom filter from reads         : %s\n", now_text());
	fflush(stdout);
	echo_reads_sizes(rr);
	ntedit_hip_reads_build_args ba = {};
	ba.files = o.paths.data();
	ba.n_files = (uint32_t)o.paths.size();
	ba.k = rr.k;
	ba.hash_num = rr.hash_num;
	ba.cmin = rr.cmin;
	ba.solid = o.ro.solid;
	ba.counts = o.counts;
	ba.bf_bytes = rr.bf_bytes;
	ba.fpr = rr.fpr;
	ba.sketch_counters = rr.sketch_counters;
	ba.batch_bytes = rr.batch_bytes;
	ba.hist_path = names.hist.empty() ? nullptr : names.hist.c_str();
	ba.use_store = 1;
	ba.store_cap = rr.store_cap;
	ba.device_parse = rr.gpu_parse;
	ba.reject_cmin = rr.reject_cmin;
	ba.reject_bf_bytes = rr.reject_bf_bytes;
	ba.reject_num_elements = rr.reject_num_elements;
	ba.min_qual = rr.min_qual;
	ntedit_hip_reads_set_read_filter(ctx, o.filter_rules.min_read_len, o.filter_rules.min_mean_qual, o.filter_rules.min_rq); // (every round alike)
	if (cascade) {
		// round 1 fills the store with every read a later round has to count (the shortest k decides) and every
		// round but the last leaves it to the next; a round that finds it ON reads nothing else
		uint32_t min_k = rr.k;
		for (const ntedit_hip_reads_rules& other : o.rounds) {
			min_k = other.k < min_k ? other.k : min_k;
		}
		// (every round that reads files keeps the reads of min_k bases or more: whichever round fills the store, a
		// later round at a smaller k finds in it all it has to count)
		ba.min_read = min_k;
		ba.keep_store = last_round ? 0 : 1;
		// a store that was released once is not tried again: every later round reads the files, as separate runs would
		ba.use_store = *store_lost ? 0 : 1;
	}
	ba.log = nte_host::reads_log;
	ntedit_hip_reads_build_result br;
	if (ntedit_hip_reads_build(ctx, &ba, &br) != 0) {
		fail("%s", ntedit_hip_reads_last_error(ctx));
	}
	const bool store_on = br.store_state == NTEDIT_RESIDENT_ON;
	if (br.from_store) {
		printf("Reads filter built in %.1f ms (minimum count %u; pass 1, the histogram pass and pass 2 read the resident store)\n",
		       br.ms_total, br.cmin);
	} else {
		printf("Reads filter built in %.1f ms (minimum count %u; the histogram pass and pass 2 read %s)\n", br.ms_total, br.cmin,
		       store_on ? "the resident store" : "the files");
	}
	if (cascade) {
		printf("Round %zu of %zu: k = %u, minimum count %u, %s\n", round + 1, n_rounds, rr.k, br.cmin,
		       br.from_store ? "every pass read the resident store, no read file was opened"
		       : store_on    ? "pass 1 read the files and filled the resident store, the later passes read it"
		                     : "every pass read the files (the resident store was released)");
	}
	FilterStage fs;
	fs.store_held = cascade && !last_round && store_on;
	*store_lost = *store_lost || (cascade && !store_on);
	save_filter(ctx, NTEDIT_FILTER_PRIMARY, names.save_bf, "Bloom filter");
	fs.bfrep = o.bfrep;
	// the reject filter, built into the secondary slot by the same pass 2: no -e file is loaded
	if (rr.reject_cmin) {
		printf("Reject filter built (reject count %u, %llu bytes)\n", rr.reject_cmin, (unsigned long long)br.reject_bf_bytes);
		save_filter(ctx, NTEDIT_FILTER_SECONDARY, names.save_reject_bf, "Reject Bloom filter");
		// (the -e line of the parameter echo; the reference's prefix has no -e part)
		fs.bfrep = names.save_reject_bf.empty() ? "reads_k" + std::to_string(rr.k) + "_reject.bf" : names.save_reject_bf;
	}
	fs.bf = names.save_bf.empty() ? "reads_k" + std::to_string(rr.k) + ".bf" : names.save_bf;
	return fs;
}

FilterStage
filter_from_file(ntedit_hip_ctx* ctx, const CliOptions& o)
{
	printf("---------- loading Bloom filter from file           : %s\n", now_text());
	if (ntedit_hip_load_filter_file(ctx, NTEDIT_FILTER_PRIMARY, o.bf.c_str()) != 0) {
		fail("Bloom filter file supplied (-r) is incorrect. (%s)", ntedit_hip_last_error(ctx));
	}
	FilterStage fs;
	fs.bf = o.bf;
	fs.bfrep = o.bfrep;
	return fs;
}

} // namespace nte_cli
