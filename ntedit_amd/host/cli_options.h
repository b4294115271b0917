// cli_options.h -- everything the `ntedit` command line decides, and every refusal that happens before the device is opened
// and before any file is written.
#pragma once

#include "../../include/ntedit_hip.h"

#include <string>
#include <utility>
#include <vector>

namespace nte_cli {

// the settings of ntedit --genome (its rules: genome_rules in cli_options.cpp)
struct GenomeRules
{
	uint32_t k = 0, hash_num = 3;
	double fpr = 0.01;
	bool have_bf = false, have_ne = false;
	uint64_t bf_bytes = 0, num_elements = 0, batch_bytes = 256ull << 20;
	int gpu_parse = 0;
};

struct CliOptions
{
	ntedit_hip_params params; // as given: each round works on a copy
	std::string draft, bf, bfrep, prefix, vcf;
	unsigned nthreads = 4;
	bool threads_given = false;
	int verbose = 0, gpu = 0, report = 0;
	unsigned long long batch_bases = 1ull << 30;
	bool batch_given = false;
	unsigned shard_i = 0, shard_n = 1;
	bool shard_given = false, no_map = false, no_pack = true, qv = false, completeness = false, bgzip = false, bed = false, spectrum = false;
	// --cn (with --spectrum): the cap of the draft store in bytes, the sketch's counters (0: the library picks)
	bool cn = false;
	const char *cn_store_text = nullptr, *cn_sketch_text = nullptr;
	unsigned long long cn_store = 32ull << 30, cn_sketch = 0;
	std::vector<std::pair<std::string, unsigned long long>> tunes;
	// --reads FILE... / --genome FILE...: `paths` are the files of whichever was given
	bool reads_mode = false, genome_mode = false;
	std::vector<std::string> read_files, genome_files;
	std::vector<const char*> paths;
	bool counts = false;
	ntedit_hip_reads_options ro = {};                 // the reads options as given
	ntedit_hip_reads_filter_options fo = {};          // --min_read_len, --min_mean_qual, --min_rq as given ...
	ntedit_hip_reads_filter_rules filter_rules = {};  // ... and their rules' outcome (zeros: off)
	std::vector<ntedit_hip_reads_rules> rounds = std::vector<ntedit_hip_reads_rules>(1); // the rules of each round (one, unless -k is a list); zeros without --reads
	std::string hist, save_bf, save_reject_bf;        // as given: a round of a cascade puts its k in place of {k}
	GenomeRules genome;
};

// Parses the command line.  Prints the "initializing" stamp, the usage or version text, the SNV note; ends the run on any
// refusal.  Opens no device.
CliOptions parse_cli(int argc, char** argv);

} // namespace nte_cli
