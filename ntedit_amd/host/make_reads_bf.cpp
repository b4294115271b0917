// make_reads_bf.cpp -- `ntedit-make-reads-bf`: the k-mer filter of a read set, built on one MI355X, for `ntedit -r`.
//
//   --reads FILE [FILE ...]  -k K  (-c CMIN | --solid)  [--hist FILE]  [--counts]  [--hashes 3]  [--fpr 0.01]
//   [--bf BYTES | --num_elements N]  [--sketch_bytes S]  [-o reads_kK.bf]  [-t THREADS]
//   [--reject_cutoff R  [--reject_bf BYTES | --reject_num_elements N]  [--reject_out reads_kK_reject.bf]]  [--min_qual Q]
//   [--min_read_len L]  [--min_mean_qual Q]  [--min_rq R]
//
// The reference leaves this step to ntHits / ntStat on the CPU (ntedit-make: `nthits -c<cutoff> --outbloom`;
// ntedit_run_pipeline.smk: `ntstat filter -cmin C`).  This tool is neither: it counts in a plain count-min sketch of
// 8-bit counters (pass 1, ntedit_hip_sketch_count) and keeps the k-mers whose estimate -- the minimum of their h
// counters -- is at least CMIN (pass 2, ntedit_hip_filter_insert_solid), so its counts and its sizing differ from
// theirs.  The output is a btllib-format filter that ntedit -r loads unchanged: a plain Bloom filter, or with --counts
// a counting filter holding each solid k-mer's estimate (for ntedit -p / -q).  Both passes read the inputs (FASTA or
// FASTQ, plain or gzip) through FastaReader, in bounded batches double-buffered through page-locked memory: a second
// thread parses the next batch while the GPU works on the current one (ntedit_hip_reads_pass, reads_pass.cpp, which
// the sharded driver ntedit_amd/make_reads.py runs over byte ranges of the same files).
//
// With --solid or --hist a histogram pass runs between the two (ntedit_hip_sketch_histogram): the k-mer histogram of
// the sketch's estimates, in place of the reference's ntCard run.  --hist writes it in ntCard's text format, --solid
// takes CMIN from its first valley (ntedit_hip_reads_solid_cutoff), and without --bf / --num_elements the output is
// sized from it: --num_elements N with N = the distinct k-mers the histogram puts at CMIN or above.
//
// With --reject_cutoff R the same pass 2 also fills a second plain filter with the k-mers whose estimate is at least R
// (ntedit_hip_filter_insert_solid2): the reject filter for `ntedit -e`, the file a second run with -c R would write.
#include "../../include/ntedit_hip.h"
#include "log_info.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <vector>

using nte_host::log_info;

// (the option rules, the sizing, the passes, the build and the --hist writer live in the library: reads_options.cpp,
// reads_pass.cpp and reads_build.cpp, shared with the sharded driver and `ntedit --reads`)
static void
usage(const char* why)
{
	if (why) {
		std::cerr << why << std::endl;
	}
	std::cerr
	    << "Usage: make_reads_bf [--help] --reads VAR... -k VAR (-c VAR | --solid) [--hist VAR] [--counts] [--hashes VAR] "
	       "[--fpr VAR] [--bf VAR] [--num_elements VAR] [--sketch_bytes VAR] [--gpu_parse] [-o VAR] [-t VAR] "
	       "[--reject_cutoff VAR] [--reject_bf VAR] [--reject_num_elements VAR] [--reject_out VAR] [--min_qual VAR] "
	       "[--min_read_len VAR] [--min_mean_qual VAR] [--min_rq VAR]\n\n"
	       "Builds the k-mer filter of a read set on the GPU: pass 1 counts every k-mer in a count-min sketch of 8-bit\n"
	       "counters, pass 2 keeps the k-mers whose estimate (the minimum of their counters) is at least -c.  Neither\n"
	       "ntHits nor ntStat: the counts (plain count-min, no conservative update) and the sizing are this tool's own.\n"
	       "With --solid or --hist a histogram pass between them gathers the k-mer histogram of the estimates.  Neither\n"
	       "ntCard nor ntStat: --solid's cutoff is the first c with f[c+1] > f[c], this tool's own rule, not a model fit.\n\n"
	       "Optional arguments:\n"
	       "  -h, --help      shows help message and exits\n"
	       "  --reads         Input reads, FASTA or FASTQ, plain or gzip, or BAM, unaligned or aligned (BAM needs\n"
	       "                  --gpu_parse) [nargs: 1 or more] [required]\n"
	       "  -k              k-mer size (bp), 12 to 200 [required]\n"
	       "  -c              Minimum k-mer count (cmin), 1 to 255 [required, unless --solid]\n"
	       "  --solid         Take cmin from the k-mer histogram: the first c with f[c+1] > f[c] (the valley after\n"
	       "                  the error peak); refused when there is none\n"
	       "  --hist          Write the k-mer histogram to this file, in ntCard's text format (F1, F0, then c and f[c]\n"
	       "                  for c = 1 to 255; the last bin counts 255 or more, ntCard stops at 64)\n"
	       "  --counts        Write a counting filter (each solid k-mer's estimate) for ntedit -p / -q\n"
	       "  --hashes        Number of hash functions, 1 to 8 [default: 3]\n"
	       "  --fpr           False positive rate for Bloom filter (with --num_elements) [default: 0.01]\n"
	       "  --bf            Output filter size in bytes\n"
	       "  --num_elements  Approximate number of solid k-mers (output size through the genome tool's formula)\n"
	       "                  (one of --bf / --num_elements is required, unless --solid or --hist: then by default\n"
	       "                  --num_elements is the number of k-mers the histogram puts at cmin or above)\n"
	       "  --sketch_bytes  Counters of the count-min sketch [default: 16 x the output bytes, or sized from the\n"
	       "                  histogram one per input byte (gzip: 4 x), 64 MiB to 32 GiB]\n"
	       "  --gpu_parse     Parse plain and bgzip-compressed (BGZF) read files on the GPU: the host ships the file's bytes,\n"
	       "                  BGZF still compressed, and the device inflates them.  The output is the same; single-stream\n"
	       "                  gzip files and files outside the clean FASTA / 4-line FASTQ grammar stay with the host\n"
	       "                  parser (recompress with `bgzip -@ 16 reads.fq`).  BAM files are inflated, walked and decoded\n"
	       "                  on the device: every primary record's bases (flags 0x100 and 0x800 are left out), as stored\n"
	       "  -o              Name for output filter [default: \"reads_k<K>.bf\"]\n"
	       "  -t              Number of threads (accepted; the k-mers are counted on the GPU) [default: 12]\n"
	       "  --reject_cutoff Also write the reject filter for ntedit -e (k-mers to reject, e.g. repeats): a plain filter of\n"
	       "                  the k-mers seen at least this many times, 2 to 255 and above -c, from the same pass 2 (the\n"
	       "                  file a second run with -c R would write); not with --counts\n"
	       "  --reject_bf     Reject filter size in bytes\n"
	       "  --reject_num_elements  Approximate number of k-mers in the reject filter (sized as --num_elements, with\n"
	       "                  --fpr) (one of the two is required with --reject_cutoff, unless --solid or --hist: then by\n"
	       "                  default it is the number of k-mers the histogram puts at the reject cutoff or above)\n"
	       "  --reject_out    Name for the reject filter [default: \"reads_k<K>_reject.bf\"]\n"
	       "  --min_qual      Minimum base quality, 1 to 93 (Phred+33; Phred+64 is not built): a base whose quality is below\n"
	       "                  it counts as N, so no k-mer that spans it is counted or kept.  FASTQ: a quality character below\n"
	       "                  33 + Q; BAM: a quality byte below Q.  Reads are still kept by their length; records without\n"
	       "                  qualities (FASTA, BAM records whose qualities are absent) pass as they are [default: off]\n"
	       "  --min_read_len  Minimum read length, 1 to 2147483647: the shortest read kept is the larger of it and k\n"
	       "                  [default: off]\n"
	       "  --min_mean_qual Minimum mean read quality, 1 to 60: the Phred value of the read's mean error probability (as\n"
	       "                  NanoFilt, chopper and fastplong take it, not the mean of the Phred values), over the qualities\n"
	       "                  as stored.  Reads without qualities pass [default: off]\n"
	       "  --min_rq        Minimum read accuracy, above 0 and at most 1: a BAM read whose rq tag (type f) is below it is\n"
	       "                  dropped; reads without the tag pass, so every FASTA and FASTQ read does [default: off]\n";
}

static bool
is_option(const char* a)
{
	return a[0] == '-' && a[1] != 0 && !(a[1] >= '0' && a[1] <= '9');
}

static void
die(ntedit_hip_ctx* ctx, const std::string& why)
{
	std::cerr << "make_reads_bf: error: " << why << std::endl;
	if (ctx) {
		ntedit_hip_sketch_free(ctx);
		ntedit_hip_destroy(ctx);
	}
	exit(1);
}

int
main(int argc, char** argv)
{
	std::vector<const char*> paths;
	ntedit_hip_reads_options ro = {};
	ntedit_hip_reads_rules rr;
	ntedit_hip_reads_filter_options fo = {}; // --min_read_len, --min_mean_qual, --min_rq
	ntedit_hip_reads_filter_rules fr = {};
	bool counts = false;
	std::string out_file, sketch_out, hist_out, reject_out;
	for (int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		auto value = [&](const char* name) -> const char* {
			if (i + 1 >= argc) {
				usage((std::string("Too few arguments for '") + name + "'.").c_str());
				exit(1);
			}
			return argv[++i];
		};
		// an option of the shared rules: what they refuse at the option itself is refused here
		auto given = [&](const char* name, const char*& text) {
			text = value(name);
			if (ntedit_hip_reads_options_check(&ro, NTEDIT_READS_DIALECT_TOOL, 0, &rr) != 0 ||
			    ntedit_hip_reads_filter_options_check(&fo, NTEDIT_READS_DIALECT_TOOL, 0, &fr) != 0) {
				usage(ntedit_hip_reads_last_error(nullptr));
				exit(1);
			}
		};
		if (a == "-h" || a == "--help") {
			usage(nullptr);
			return 0;
		} else if (a == "--reads") {
			while (i + 1 < argc && !is_option(argv[i + 1])) {
				paths.push_back(argv[++i]);
			}
		} else if (a == "-k") {
			given("-k", ro.k);
		} else if (a == "-c") {
			given("-c", ro.cutoff);
		} else if (a == "--solid") {
			ro.solid = 1;
		} else if (a == "--hist") {
			hist_out = value("--hist");
		} else if (a == "--gpu_parse") {
			ro.gpu_parse = 1;
		} else if (a == "--counts") {
			counts = true;
		} else if (a == "--hashes") {
			given("--hashes", ro.hashes);
		} else if (a == "--fpr") {
			given("--fpr", ro.fpr);
		} else if (a == "--bf") {
			given("--bf", ro.bf);
		} else if (a == "--num_elements") {
			given("--num_elements", ro.num_elements);
		} else if (a == "--sketch_bytes") {
			given("--sketch_bytes", ro.sketch_bytes);
		} else if (a == "--batch_bytes") { // (not in the usage text: tests force many small batches with it)
			given("--batch_bytes", ro.batch_bytes);
		} else if (a == "--save_sketch") { // (not in the usage text: tests compare the sketch itself)
			sketch_out = value("--save_sketch");
		} else if (a == "--reject_cutoff") {
			given("--reject_cutoff", ro.reject_cutoff);
		} else if (a == "--reject_bf") {
			given("--reject_bf", ro.reject_bf);
		} else if (a == "--reject_num_elements") {
			given("--reject_num_elements", ro.reject_num_elements);
		} else if (a == "--min_qual") {
			given("--min_qual", ro.min_qual);
		} else if (a == "--min_read_len") {
			given("--min_read_len", fo.min_read_len);
		} else if (a == "--min_mean_qual") {
			given("--min_mean_qual", fo.min_mean_qual);
		} else if (a == "--min_rq") {
			given("--min_rq", fo.min_rq);
		} else if (a == "--reject_out") {
			reject_out = value("--reject_out");
			ro.reject_out = 1;
		} else if (a == "-o") {
			out_file = value("-o");
		} else if (a == "-t") {
			given("-t", ro.threads);
		} else {
			usage(("Unknown argument: " + a).c_str());
			return 1;
		}
	}
	if (paths.empty()) {
		usage("--reads: 1 or more argument(s) expected. 0 provided.");
		return 1;
	}
	ro.hist = !hist_out.empty();
	ro.counts = counts;
	ro.files = paths.data();
	ro.n_files = (uint32_t)paths.size();
	const int refused = ntedit_hip_reads_options_check(&ro, NTEDIT_READS_DIALECT_TOOL, 1, &rr);
	if (refused && refused != NTEDIT_READS_EMPTY) {
		usage(ntedit_hip_reads_last_error(nullptr));
		return 1;
	}
	if (ntedit_hip_reads_filter_options_check(&fo, NTEDIT_READS_DIALECT_TOOL, 1, &fr) != 0) { // (behind --min_qual's rules)
		usage(ntedit_hip_reads_last_error(nullptr));
		return 1;
	}
	if (out_file.empty()) {
		out_file = "reads_k" + std::to_string(rr.k) + ".bf";
	}
	if (reject_out.empty()) {
		reject_out = "reads_k" + std::to_string(rr.k) + "_reject.bf";
	}

	std::cout << "Parameters:" << std::endl;
	std::cout << "\t\t--reads ";
	for (const char* r : paths) {
		std::cout << r << " ";
	}
	std::cout << std::endl;
	std::cout << "\t\t-t " << rr.threads << std::endl;
	std::cout << "\t\t-k " << rr.k << std::endl;
	if (ro.solid) {
		std::cout << "\t\t--solid" << std::endl;
	} else {
		std::cout << "\t\t-c " << rr.cmin << std::endl;
	}
	if (!hist_out.empty()) {
		std::cout << "\t\t--hist " << hist_out << std::endl;
	}
	std::cout << "\t\t--fpr " << rr.fpr << std::endl;
	std::cout << "\t\t--hashes " << rr.hash_num << std::endl;
	std::cout << "\t\t-o " << out_file << std::endl;
	if (counts) {
		std::cout << "\t\t--counts" << std::endl;
	}
	if (rr.gpu_parse) {
		std::cout << "\t\t--gpu_parse" << std::endl;
	}
	if (ro.bf) {
		std::cout << "\t\t--bf " << rr.bf_bytes << std::endl;
	} else if (ro.num_elements) {
		std::cout << "\t\t--num_elements " << rr.num_elements << std::endl;
	}
	if (rr.reject_cmin) {
		std::cout << "\t\t--reject_cutoff " << rr.reject_cmin << std::endl;
		std::cout << "\t\t--reject_out " << reject_out << std::endl;
		if (ro.reject_bf) {
			std::cout << "\t\t--reject_bf " << rr.reject_bf_bytes << std::endl;
		} else if (ro.reject_num_elements) {
			std::cout << "\t\t--reject_num_elements " << rr.reject_num_elements << std::endl;
		}
	}
	if (rr.min_qual) {
		std::cout << "\t\t--min_qual " << rr.min_qual << std::endl;
	}
	if (fr.min_read_len) {
		std::cout << "\t\t--min_read_len " << fr.min_read_len << std::endl;
	}
	if (fr.min_mean_qual) {
		std::cout << "\t\t--min_mean_qual " << fr.min_mean_qual << std::endl;
	}
	if (fr.min_rq > 0.0f) {
		std::cout << "\t\t--min_rq " << fo.min_rq << std::endl;
	}
	if (refused) { // (the output filter would be empty)
		usage(ntedit_hip_reads_last_error(nullptr));
		return 1;
	}
	if (rr.size_from_hist) {
		std::cout << "BF size (bytes): from the k-mer histogram" << std::endl;
	} else {
		std::cout << "BF size (bytes): " << rr.bf_bytes << std::endl;
	}
	if (rr.reject_cmin && rr.reject_size_from_hist) {
		std::cout << "Reject BF size (bytes): from the k-mer histogram" << std::endl;
	} else if (rr.reject_cmin) {
		std::cout << "Reject BF size (bytes): " << rr.reject_bf_bytes << std::endl;
	}
	std::cout << "Sketch size (counters): " << rr.sketch_counters << std::endl;

	ntedit_hip_ctx* ctx = nullptr;
	if (ntedit_hip_create(0, &ctx) != 0) {
		std::cerr << "make_reads_bf: error: " << (ctx ? ntedit_hip_last_error(ctx) : "no HIP device") << std::endl;
		return 1;
	}
	// sketch, pass 1, the histogram pass, the output filter, pass 2 (reads_build.cpp, shared with `ntedit --reads`)
	ntedit_hip_reads_build_args ba = {};
	ba.files = paths.data();
	ba.n_files = (uint32_t)paths.size();
	ba.k = rr.k;
	ba.hash_num = rr.hash_num;
	ba.cmin = rr.cmin;
	ba.solid = ro.solid;
	ba.counts = counts;
	ba.bf_bytes = rr.bf_bytes;
	ba.fpr = rr.fpr;
	ba.sketch_counters = rr.sketch_counters;
	ba.batch_bytes = rr.batch_bytes;
	ba.hist_path = hist_out.empty() ? nullptr : hist_out.c_str();
	ba.sketch_path = sketch_out.empty() ? nullptr : sketch_out.c_str();
	ba.log = nte_host::reads_log;
	ba.device_parse = rr.gpu_parse;
	ba.reject_cmin = rr.reject_cmin;
	ba.reject_bf_bytes = rr.reject_bf_bytes;
	ba.reject_num_elements = rr.reject_num_elements;
	ba.min_qual = rr.min_qual;
	ntedit_hip_reads_set_read_filter(ctx, fr.min_read_len, fr.min_mean_qual, fr.min_rq);
	ntedit_hip_reads_build_result br;
	if (ntedit_hip_reads_build(ctx, &ba, &br) != 0) {
		die(ctx, ntedit_hip_reads_last_error(ctx));
	}

	uint64_t occupied = 0, slots = 0;
	if (ntedit_hip_filter_occupancy(ctx, NTEDIT_FILTER_PRIMARY, &occupied, &slots) != 0) {
		die(ctx, ntedit_hip_last_error(ctx));
	}
	// btllib get_fpr(): occupancy ^ hash_num
	std::cout << "Bloom filter FPR: " << pow((double)occupied / (double)slots, (double)rr.hash_num) << std::endl;

	log_info(counts ? "Saving counting Bloom filter" : "Saving Bloom filter");
	if (ntedit_hip_filter_save_file(ctx, NTEDIT_FILTER_PRIMARY, out_file.c_str()) != 0) {
		die(ctx, "cannot write " + out_file);
	}
	if (rr.reject_cmin) {
		if (ntedit_hip_filter_occupancy(ctx, NTEDIT_FILTER_SECONDARY, &occupied, &slots) != 0) {
			die(ctx, ntedit_hip_last_error(ctx));
		}
		std::cout << "Reject Bloom filter FPR: " << pow((double)occupied / (double)slots, (double)rr.hash_num) << std::endl;
		log_info("Saving reject Bloom filter");
		if (ntedit_hip_filter_save_file(ctx, NTEDIT_FILTER_SECONDARY, reject_out.c_str()) != 0) {
			die(ctx, "cannot write " + reject_out);
		}
	}
	log_info("Done!");
	ntedit_hip_destroy(ctx);
	return 0;
}
