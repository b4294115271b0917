// main.cpp -- `ntedit` host driver for the MI355X hot path.
//
// Keeps the reference's command-line surface (ntedit.cpp:135-169, 2276-2364):
//   -t -f -r -e -b -z -i -d -x -y -X -Y -c -j -m -s -l -a -v -p -q -k --help --version
// (-k is accepted and ignored: k comes from the Bloom filter header.  The reference lists -k in its
// option string but has no `case 'k'`, so `-k N` trips its "invalid option" check, ntedit.cpp:2360-2363;
// being lenient here keeps old command lines working.  -c is parsed and overwritten by k*1.5; -t sets the host
// threads that render the output, contigs themselves are polished on the GPU and
// the output order is the input order, i.e. the reference at -t 1).  Reads the draft with kseq semantics, batches
// contigs, calls the C ABI (include/ntedit_hip.h) and writes
// <prefix>_edited.fa and <prefix>_changes.tsv byte-identically to the
// reference, plus <prefix>_variants.vcf (the ##fileDate line carries today's date, as in
// the reference).
#include "../../include/ntedit_hip.h"
#include "fasta.h"
#include "fasta_map.h"
#include "k_list.h"
#include "log_info.h"

#include <algorithm>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <getopt.h>
#include <sstream>
#include <memory>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

#define PROGRAM "ntEdit v2.1.1"

static const char USAGE[] = PROGRAM
    " (MI355X HIP hot path)\n\n"
    " Options:\n"
    "	-t,	number of host threads rendering the output (contigs are polished on the GPU)\n"
    "	-f,	draft genome assembly (FASTA, Multi-FASTA, and/or gzipped compatible), REQUIRED\n"
    "	-r,	Bloom filter (BF) or counting BF (CBF) file (btllib format, e.g. from ntStat v1.0.0+), REQUIRED unless --reads\n"
    "	-e,	secondary BF with k-mers to reject, OPTIONAL\n"
    "	-b,	output file prefix, OPTIONAL\n"
    "	-z,	minimum contig length [default=100]\n"
    "	-i,	maximum number of insertion bases to try, range 0-5, [default=5]\n"
    "	-d,	maximum number of deletions bases to try, range 0-10, [default=5]\n"
    "	-x,	k/x ratio for the number of k-mers that should be missing, [default=5.000]\n"
    "	-y, 	k/y ratio for the number of edited k-mers that should be present, [default=9.000]\n"
    "	-X, 	ratio of number of k-mers in the k subset that should be missing, [default=0.5]\n"
    "	-Y, 	ratio of number of k-mers in the k subset that should be present, [default=0.5]\n"
    "	-c,	cap for the number of base insertions at one position (parsed; k*1.5 is used)\n"
    "	-j, 	controls size of k-mer subset, check every jth k-mer, [default=3]\n"
    "	-m,	mode of editing, range 0-2, [default=0]\n"
    "	-s,     SNV mode. Overrides draft k-mer checks, forcing reassessment at each position (-s 1 = yes, default = 0, no)\n"
    "	-l,	input VCF file with annotated variants (e.g., clinvar.vcf[.gz]), OPTIONAL\n"
    "	-a,	soft masks missing k-mer positions having no fix (1 = yes, default = 0, no)\n"
    "	-v,	verbose mode (accepted)\n"
    "	-p,	minimum k-mer coverage threshold (CBF only) [default=1]\n"
    "	-q,	maximum k-mer coverage threshold (CBF only) [default=255]\n"
    "	--gpu N,	HIP device index [default=0]\n"
    "	--batch-bases N,	bases per GPU batch [default: the first batch 134217728, doubling up to 536870912]\n"
    "	--tune KEY=VALUE,	library tuning knob (ntedit_hip_set_tuning; repeatable; none of them changes a result)\n"
    "	--qv,	k-mer QV of the draft before and after the polish, against the filter the run polishes with: writes\n"
    "			<prefix>_qv.tsv (name, len_before, len_after, kmers_before, absent_before, qv_before, kmers_after,\n"
    "			absent_after, qv_after per contig and a last row #total) and prints one summary line.  The edited contigs are\n"
    "			built and screened in HBM; no second pass over reads or k-mer database.  Not with --shard\n"
    "	--completeness,	with --qv: k-mer completeness before and after the polish -- the share of the filter's k-mers that the\n"
    "			draft holds, by linear counting of the draft's distinct present k-mers in HBM.  Writes\n"
    "			<prefix>_completeness.tsv (stage, filter_bits, filter_set, filter_kmers, shared_set, shared_kmers, completeness;\n"
    "			a row `before' and a row `after') and prints one summary line.  A plain filter only.  Not with --shard\n"
    "	--shard I/N,	polish share I of N of the contigs, split by BASES (greedy longest-first over whole contigs, the\n"
    "			same on every process); writes <prefix>.index.tsv for `python -m ntedit_amd.merge`.\n"
    "			(`python -m ntedit_amd.run` is the full multi-GPU driver: one filter broadcast, large contigs cut)\n"
    "\n Polishing straight from reads (--reads replaces -r; the filter is the one ntedit-make-reads-bf builds with the\n"
    " same settings, built on the GPU into the context that polishes, no filter file needed):\n"
    "	--reads FILE...,	input reads, FASTA or FASTQ, plain or gzip (1 or more files)\n"
    "	-k,	k-mer size (bp), 12 to 200, REQUIRED with --reads (accepted and ignored without it)\n"
    "	-k K1,K2,...,	a list of 2 to 8 different k: polish in a cascade of rounds, in that order (needs -b).  Round i builds\n"
    "			the filter for Ki and polishes round i-1's _edited.fa; the last round writes <prefix>_edited.fa, an\n"
    "			earlier one <prefix>_k<Ki>_edited.fa (and _changes.tsv, _variants.vcf).  The read files are parsed\n"
    "			once: from round 2 on every pass reads the reads kept in HBM.  --hist, --save_bf and\n"
    "			--save_reject_bf then need {k} in the name (each round puts its k there)\n"
    "	--cutoff C,	minimum k-mer count of the filter, 1 to 255 (ntedit-make-reads-bf -c)\n"
    "	--solid,	take the minimum count from the k-mer histogram instead (give --cutoff or --solid)\n"
    "	--counts,	build a counting filter (enables -p / -q)\n"
    "	--hashes H,	number of hash functions, 1 to 8 [default=3]\n"
    "	--fpr F,	false positive rate of the filter (with --num_elements) [default=0.01]\n"
    "	--bf BYTES,	filter size in bytes\n"
    "	--num_elements N,	approximate number of solid k-mers (one of --bf / --num_elements is required, unless\n"
    "			--solid or --hist: then the filter is sized from the k-mer histogram)\n"
    "	--sketch_bytes S,	counters of the count-min sketch [default: as ntedit-make-reads-bf]\n"
    "	--hist FILE,	write the k-mer histogram (ntCard's text format)\n"
    "	--save_bf FILE,	write the filter that was built (the same bytes as ntedit-make-reads-bf -o); its name is the\n"
    "			_r part of the default prefix [default name: reads_k<K>.bf, not written]\n"
    "	--gpu_parse,	parse plain and bgzip-compressed (BGZF) read files on the GPU: the host ships the file's bytes, BGZF\n"
    "			still compressed, and the device inflates them (same outputs; single-stream gzip files and files\n"
    "			outside the clean FASTA / 4-line FASTQ grammar stay with the host parser)\n"
    "	--reject_cutoff R,	also build the -e filter (k-mers to reject, e.g. repeats) from the same pass over the reads: a\n"
    "			plain filter of the k-mers seen at least R times, 2 to 255 and above the cutoff (replaces -e;\n"
    "			not with --counts)\n"
    "	--reject_bf BYTES,	reject filter size in bytes\n"
    "	--reject_num_elements N,	approximate number of k-mers in the reject filter (one of the two is required with\n"
    "			--reject_cutoff, unless --solid or --hist: then it is sized from the k-mer histogram)\n"
    "	--save_reject_bf FILE,	write the reject filter that was built (the bytes ntedit-make-reads-bf -c R would write)\n"
    "			[default name: reads_k<K>_reject.bf, not written]\n"
    "\n Polishing straight from genome assemblies (--genome replaces -r; the filter is the one ntedit-make-genome-bf builds\n"
    " with the same settings, built on the GPU into the context that polishes, no filter file needed):\n"
    "	--genome FILE...,	genome FASTA, plain or gzip (1 or more files)\n"
    "	-k,	k-mer size (bp), 12 to 200, REQUIRED with --genome\n"
    "	--hashes H, --fpr F,	as above [defaults 3, 0.01]\n"
    "	--bf BYTES | --num_elements N,	the filter's size [default: from the genome's size, as the tool sizes it]\n"
    "	--save_bf FILE,	write the filter that was built (the same bytes as ntedit-make-genome-bf -o); its name is the _r\n"
    "			part of the default prefix [default name: genome_bf.bf, not written]\n"
    "	--gpu_parse,	parse plain and bgzip-compressed (BGZF) genome FASTA on the GPU, records of any length (same\n"
    "			outputs; single-stream gzip files stay with the host parser)\n"
    "	--help,		display this message and exit \n"
    "	--version,	output version information and exit\n\n";

static const char shortopts[] = "t:f:s:k:z:b:r:v:d:i:X:Y:x:y:m:c:j:s:e:a:l:p:q:";
enum
{
	OPT_HELP = 1000,
	OPT_VERSION,
	OPT_GPU,
	OPT_BATCH,
	OPT_SHARD,
	OPT_REPORT,
	OPT_QV,
	OPT_COMPLETENESS,
	OPT_START_GRID,
	OPT_EVENT_BUDGET,
	OPT_NO_MAP,
	OPT_PACK,
	OPT_TUNE,
	OPT_CUTOFF,
	OPT_SOLID,
	OPT_COUNTS,
	OPT_HASHES,
	OPT_FPR,
	OPT_BF,
	OPT_NUM_ELEMENTS,
	OPT_SKETCH_BYTES,
	OPT_HIST,
	OPT_SAVE_BF,
	OPT_REJECT_CUTOFF,
	OPT_REJECT_BF,
	OPT_REJECT_NUM_ELEMENTS,
	OPT_SAVE_REJECT_BF,
	OPT_READS_BATCH,
	OPT_STORE_CAP,
	OPT_GPU_PARSE
};
static const struct option longopts[] = {
	{ "threads", required_argument, nullptr, 't' },
	{ "draft_file", required_argument, nullptr, 'f' },
	{ "k", required_argument, nullptr, 'k' },
	{ "minimum_contig_length", required_argument, nullptr, 'z' },
	{ "maximum_insertions", required_argument, nullptr, 'i' },
	{ "maximum_deletions", required_argument, nullptr, 'd' },
	{ "insertion_cap", required_argument, nullptr, 'c' },
	{ "edit_threshold", required_argument, nullptr, 'y' },
	{ "missing_threshold", required_argument, nullptr, 'x' },
	{ "edit_ratio", required_argument, nullptr, 'Y' },
	{ "missing_ratio", required_argument, nullptr, 'X' },
	{ "jump", required_argument, nullptr, 'j' },
	{ "bloom_filename", required_argument, nullptr, 'r' },
	{ "bloomrep_filename", required_argument, nullptr, 'e' },
	{ "outfile_prefix", required_argument, nullptr, 'b' },
	{ "mode", required_argument, nullptr, 'm' },
	{ "snv", required_argument, nullptr, 's' },
	{ "vcf_file", required_argument, nullptr, 'l' },
	{ "mask", required_argument, nullptr, 'a' },
	{ "verbose", required_argument, nullptr, 'v' },
	{ "minimum_kmer_coverage", required_argument, nullptr, 'p' },
	{ "maximum_kmer_coverage", required_argument, nullptr, 'q' },
	{ "gpu", required_argument, nullptr, OPT_GPU },
	{ "batch-bases", required_argument, nullptr, OPT_BATCH },
	{ "start-grid", required_argument, nullptr, OPT_START_GRID },     // tuning / tests: ntedit_hip_params.start_grid
	{ "event-budget", required_argument, nullptr, OPT_EVENT_BUDGET }, // tuning / tests: ntedit_hip_params.event_budget
	{ "shard", required_argument, nullptr, OPT_SHARD },
	{ "tune", required_argument, nullptr, OPT_TUNE },                 // tuning / tests: ntedit_hip_set_tuning key=value (repeatable)
	{ "no-map", no_argument, nullptr, OPT_NO_MAP }, // tests: plain FASTA through the streaming reader as well
	{ "pack", no_argument, nullptr, OPT_PACK }, // batches cross PCIe in the packed form (off: packing costs the reader stage more than the link saves)
	{ "report", no_argument, nullptr, OPT_REPORT },
	{ "qv", no_argument, nullptr, OPT_QV },
	{ "completeness", no_argument, nullptr, OPT_COMPLETENESS },
	// --reads (taken out of argv before getopt: it takes one or more files) and the reads filter's options
	{ "cutoff", required_argument, nullptr, OPT_CUTOFF },
	{ "solid", no_argument, nullptr, OPT_SOLID },
	{ "counts", no_argument, nullptr, OPT_COUNTS },
	{ "hashes", required_argument, nullptr, OPT_HASHES },
	{ "fpr", required_argument, nullptr, OPT_FPR },
	{ "bf", required_argument, nullptr, OPT_BF },
	{ "num_elements", required_argument, nullptr, OPT_NUM_ELEMENTS },
	{ "sketch_bytes", required_argument, nullptr, OPT_SKETCH_BYTES },
	{ "hist", required_argument, nullptr, OPT_HIST },
	{ "save_bf", required_argument, nullptr, OPT_SAVE_BF },
	{ "reject_cutoff", required_argument, nullptr, OPT_REJECT_CUTOFF },
	{ "reject_bf", required_argument, nullptr, OPT_REJECT_BF },
	{ "reject_num_elements", required_argument, nullptr, OPT_REJECT_NUM_ELEMENTS },
	{ "save_reject_bf", required_argument, nullptr, OPT_SAVE_REJECT_BF },
	{ "batch_bytes", required_argument, nullptr, OPT_READS_BATCH }, // tests: many small read batches
	{ "resident_cap", required_argument, nullptr, OPT_STORE_CAP }, // tests: the resident store's cap (0: off)
	{ "gpu_parse", no_argument, nullptr, OPT_GPU_PARSE },
	{ "help", no_argument, nullptr, OPT_HELP },
	{ "version", no_argument, nullptr, OPT_VERSION },
	{ nullptr, 0, nullptr, 0 }
};

static void
die_unreadable(const std::string& path)
{
	// ntedit.cpp:476-483
	if (access(path.c_str(), R_OK) == -1) {
		fprintf(stderr, PROGRAM ": error: `%s': %s\n", path.c_str(), strerror(errno));
		exit(EXIT_FAILURE);
	}
}

static std::string
base_name(const std::string& p)
{
	return p.substr(p.find_last_of("/\\") + 1);
}

template<typename T>
static void
parse(int c, const char* arg, T& out)
{
	std::istringstream ss(arg ? arg : "");
	ss >> out;
	if (arg && (!ss.eof() || ss.fail())) {
		// ntedit.cpp:2360-2363
		fprintf(stderr, PROGRAM ": invalid option: `-%c%s'\n", (char)c, arg);
		exit(EXIT_FAILURE);
	}
}

static void
refuse(const std::string& why)
{
	fprintf(stderr, PROGRAM ": error: %s\nTry `" PROGRAM " --help' for more information.\n", why.c_str());
	exit(EXIT_FAILURE);
}

// the reads options through the library's rules (reads_options.cpp); a refusal ends the run, in the words and the form it
// always had: a malformed number as getopt's invalid options are
static ntedit_hip_reads_rules
reads_rules(const ntedit_hip_reads_options& ro, int final)
{
	ntedit_hip_reads_rules rr;
	const int rc = ntedit_hip_reads_options_check(&ro, NTEDIT_READS_DIALECT_POLISHER, final, &rr);
	if (rc == NTEDIT_READS_NOT_A_NUMBER) {
		fprintf(stderr, PROGRAM ": %s\n", ntedit_hip_reads_last_error(nullptr));
		exit(EXIT_FAILURE);
	}
	if (rc != 0) {
		refuse(ntedit_hip_reads_last_error(nullptr));
	}
	return rr;
}

// The rules of ntedit --genome, apart from the reads options' (reads_options.cpp knows nothing of them): what is refused
// before the device is opened and before any file is written.  The numbers arrive well-formed (reads_rules refuses a
// malformed one at its option); -k is checked here.  Returns the refusal, or "" and the settings.
struct GenomeRules
{
	uint32_t k = 0, hash_num = 3;
	double fpr = 0.01;
	bool have_bf = false, have_ne = false;
	uint64_t bf_bytes = 0, num_elements = 0, batch_bytes = 256ull << 20;
	int gpu_parse = 0;
};

static std::string
genome_rules(const ntedit_hip_reads_options& ro, bool have_r, bool reads_mode, bool shard_given, size_t n_files,
             const std::vector<std::string>& given, GenomeRules* g)
{
	static const char* const reads_only[] = { "--cutoff", "--solid", "--counts", "--hist", "--sketch_bytes", "--reject_cutoff", "--reject_bf",
		                                      "--reject_num_elements", "--save_reject_bf", "--resident_cap" };
	if (have_r) {
		return "--genome and -r: give one of them (--genome builds the filter that -r would load)";
	}
	if (reads_mode) {
		return "--genome and --reads: give one of them (each builds the filter that -r would load)";
	}
	if (shard_given) {
		return "--genome and --shard: every shard would build the whole filter again; build it once with "
		       "ntedit-make-genome-bf and give each shard -r";
	}
	if (n_files == 0) {
		return "--genome: 1 or more files expected";
	}
	for (const std::string& name : given) {
		for (const char* r : reads_only) {
			if (name == r) {
				return name + ": only with --reads (--genome builds the plain filter of every k-mer of the assemblies)";
			}
		}
	}
	if (!ro.k) {
		return "-k: required with --genome";
	}
	char* end = nullptr;
	const unsigned long long k = strtoull(ro.k, &end, 10);
	if (!*ro.k || *end || ro.k[0] == '-' || k < 12 || k > 200) {
		return std::string("-k ") + ro.k + ": k must be between 12 and 200";
	}
	g->k = (uint32_t)k;
	if (ro.hashes) {
		const unsigned long long h = strtoull(ro.hashes, nullptr, 10);
		if (h < 1 || h > 8) {
			return "--hashes " + std::to_string(h) + ": the number of hash functions must be between 1 and 8";
		}
		g->hash_num = (uint32_t)h;
	}
	if (ro.fpr) {
		g->fpr = strtod(ro.fpr, nullptr);
	}
	if (ro.bf) {
		g->have_bf = true;
		g->bf_bytes = strtoull(ro.bf, nullptr, 10);
	}
	if (ro.num_elements) {
		g->have_ne = true;
		g->num_elements = strtoull(ro.num_elements, nullptr, 10);
	}
	if ((g->have_bf && g->bf_bytes == 0) ||
	    (!g->have_bf && g->have_ne && ntedit_hip_reads_bf_size(g->num_elements, g->hash_num, g->fpr) == 0)) {
		return "--bf / --num_elements: the filter would be empty";
	}
	if (ro.batch_bytes) {
		g->batch_bytes = strtoull(ro.batch_bytes, nullptr, 10);
		if (g->batch_bytes == 0) {
			return "--batch_bytes: at least 1";
		}
	}
	g->gpu_parse = ro.gpu_parse ? 1 : 0;
	return "";
}

struct Batch
{
	std::string blob; // filled by the streaming reader (append per line) ...
	char* raw = nullptr; // ... or by the mapped reader (whole records copied concurrently; never zero-filled)
	size_t raw_n = 0, raw_cap = 0;
	const char* data() const { return raw_n ? raw : blob.data(); }
	size_t size() const { return raw_n ? raw_n : blob.size(); }
	bool raw_pinned = false; // raw came from ntedit_hip_host_alloc (page-locked: asynchronous H2D at link speed)
	void release_raw()
	{
		if (raw_pinned) {
			ntedit_hip_host_free(raw);
		} else {
			free(raw);
		}
		raw = nullptr;
		raw_cap = 0;
		raw_pinned = false;
	}
	bool reserve_raw(size_t n)
	{
		if (n > raw_cap) {
			release_raw();
			raw_cap = n + n / 8 + (1u << 20);
			raw = (char*)malloc(raw_cap);
			if (raw) {
				const uintptr_t lo = ((uintptr_t)raw + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
				const uintptr_t hi = ((uintptr_t)raw + raw_cap) & ~(uintptr_t)((2u << 20) - 1);
				if (hi > lo) {
					(void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
				}
			} else {
				raw_cap = 0;
			}
		}
		return raw != nullptr;
	}
	// the batch in the packed form (include/ntedit_hip.h: 4-bit codes + a case bit per base), written by the reader stage:
	// that is what crosses PCIe; the bytes stay for the renderer
	std::vector<char> packed;
	bool is_packed = false;
	std::vector<uint64_t> offs;
	std::vector<uint32_t> lens;
	std::vector<std::string> names;
	std::vector<uint64_t> ordinals; // position of the contig among the contigs >= -z of the whole draft
	void clear()
	{
		blob.clear();
		raw_n = 0;
		is_packed = false;
		offs.clear();
		lens.clear();
		names.clear();
		ordinals.clear();
	}
};

struct Work
{
	Batch b;
	ntedit_hip_result* res = nullptr;
};

// blocking hand-over queue between the pipeline stages (nullptr = end of stream)
class Channel
{
  public:
	void push(Work* w)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			q_.push_back(w);
		}
		cv_.notify_one();
	}
	Work* pop()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [&]() { return !q_.empty(); });
		Work* w = q_.front();
		q_.pop_front();
		return w;
	}

  private:
	std::mutex mu_;
	std::condition_variable cv_;
	std::deque<Work*> q_;
};

int
main(int argc, char** argv)
{
	ntedit_hip_params p_given; // (the options as given: each round works on a copy)
	ntedit_hip_params_default(&p_given);
	std::string draft_given, bf_given, bfrep_given, prefix_given, vcf;
	unsigned nthreads = 4, ignored_u = 0;
	bool threads_given = false;
	int verbose = 0, gpu = 0, report = 0;
	unsigned long long batch_bases = 1ull << 30;
	bool batch_given = false;
	unsigned shard_i = 0, shard_n = 1;
	bool die = false, no_map = false, no_pack = true;
	std::vector<std::pair<std::string, unsigned long long>> tunes;
	// --reads FILE...: the files up to the next option (taken out here, getopt takes one argument per option)
	std::vector<std::string> read_files;
	std::vector<const char*> paths;
	bool reads_mode = false;
	// --genome FILE...: likewise
	std::vector<std::string> genome_files;
	bool genome_mode = false;
	GenomeRules gr;
	std::vector<char*> args;
	for (int i = 0; i < argc; i++) {
		if (i > 0 && strcmp(argv[i], "--reads") == 0) {
			reads_mode = true;
			while (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] != 0)) {
				read_files.push_back(argv[++i]);
			}
			continue;
		}
		if (i > 0 && strcmp(argv[i], "--genome") == 0) {
			genome_mode = true;
			while (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] != 0)) {
				genome_files.push_back(argv[++i]);
			}
			continue;
		}
		args.push_back(argv[i]);
	}
	args.push_back(nullptr);
	argc = (int)args.size() - 1;
	argv = args.data();
	std::string hist_given, save_bf_given, save_reject_bf_given; // (as given: a round of a cascade puts its k in place of {k})
	bool counts = false, shard_given = false, qv = false, completeness = false;
	ntedit_hip_reads_options ro = {}; // the reads options as given; refused at the option where the rules say so
	std::vector<ntedit_hip_reads_rules> rounds(1); // the rules of each round (one, unless -k is a list); zeros without --reads
	std::vector<std::string> k_list;               // -k K1,K2,...: its k as given, in order
	std::vector<std::string> reads_only; // reads options given (refused without --reads)
	// a reads option with a value: its text to the rules, which refuse at the option what they refuse there
	auto reads_option = [&](const char* name, const char** text) {
		*text = optarg;
		reads_only.push_back(name);
		reads_rules(ro, 0);
	};
	for (int c; (c = getopt_long(argc, argv, shortopts, longopts, nullptr)) != -1;) {
		switch (c) {
		case '?':
			die = true;
			break;
		case 't':
			parse(c, optarg, nthreads);
			threads_given = true;
			break;
		case 'f':
			parse(c, optarg, draft_given);
			break;
		case 'z':
			parse(c, optarg, p_given.min_contig_len);
			break;
		case 'b':
			parse(c, optarg, prefix_given);
			break;
		case 'r':
			parse(c, optarg, bf_given);
			break;
		case 'e':
			parse(c, optarg, bfrep_given);
			break;
		case 'd':
			parse(c, optarg, p_given.max_deletions);
			break;
		case 'i':
			parse(c, optarg, p_given.max_insertions);
			break;
		case 'x':
			parse(c, optarg, p_given.missing_threshold);
			break;
		case 'y':
			parse(c, optarg, p_given.edit_threshold);
			break;
		case 'X':
			parse(c, optarg, p_given.missing_ratio);
			p_given.use_ratio = 1;
			break;
		case 'Y':
			parse(c, optarg, p_given.edit_ratio);
			p_given.use_ratio = 1;
			break;
		case 'c':
			parse(c, optarg, ignored_u); // overwritten by k*1.5 (ntedit.cpp:2450)
			break;
		case 'j':
			parse(c, optarg, p_given.jump);
			break;
		case 'm':
			parse(c, optarg, p_given.mode);
			break;
		case 's':
			parse(c, optarg, p_given.snv);
			break;
		case 'l':
			parse(c, optarg, vcf);
			break;
		case 'a':
			parse(c, optarg, p_given.mask);
			break;
		case 'v':
			parse(c, optarg, verbose);
			break;
		case 'p':
			parse(c, optarg, p_given.min_threshold);
			break;
		case 'q':
			parse(c, optarg, p_given.max_threshold);
			break;
		case 'k':
			// without --reads: accepted and ignored (the reference rejects it: no `case 'k'`, ntedit.cpp:2360-2363)
			ro.k = optarg;
			break;
		case OPT_CUTOFF:
			reads_option("--cutoff", &ro.cutoff);
			break;
		case OPT_SOLID:
			ro.solid = 1;
			reads_only.push_back("--solid");
			break;
		case OPT_COUNTS:
			counts = true;
			reads_only.push_back("--counts");
			break;
		case OPT_HASHES:
			reads_option("--hashes", &ro.hashes);
			break;
		case OPT_FPR:
			reads_option("--fpr", &ro.fpr);
			break;
		case OPT_BF:
			reads_option("--bf", &ro.bf);
			break;
		case OPT_NUM_ELEMENTS:
			reads_option("--num_elements", &ro.num_elements);
			break;
		case OPT_SKETCH_BYTES:
			reads_option("--sketch_bytes", &ro.sketch_bytes);
			break;
		case OPT_HIST:
			hist_given = optarg;
			ro.hist = 1;
			reads_only.push_back("--hist");
			break;
		case OPT_SAVE_BF:
			save_bf_given = optarg;
			reads_only.push_back("--save_bf");
			break;
		case OPT_REJECT_CUTOFF:
			reads_option("--reject_cutoff", &ro.reject_cutoff);
			break;
		case OPT_REJECT_BF:
			reads_option("--reject_bf", &ro.reject_bf);
			break;
		case OPT_REJECT_NUM_ELEMENTS:
			reads_option("--reject_num_elements", &ro.reject_num_elements);
			break;
		case OPT_SAVE_REJECT_BF:
			save_reject_bf_given = optarg;
			ro.reject_out = 1;
			reads_only.push_back("--save_reject_bf");
			break;
		case OPT_READS_BATCH:
			reads_option("--batch_bytes", &ro.batch_bytes);
			break;
		case OPT_STORE_CAP:
			reads_option("--resident_cap", &ro.store_cap);
			break;
		case OPT_GPU_PARSE:
			ro.gpu_parse = 1;
			reads_only.push_back("--gpu_parse");
			break;
		case OPT_GPU:
			parse(c, optarg, gpu);
			break;
		case OPT_BATCH:
			parse(c, optarg, batch_bases);
			batch_given = true;
			break;
		case OPT_START_GRID:
			parse(c, optarg, p_given.start_grid);
			break;
		case OPT_EVENT_BUDGET:
			parse(c, optarg, p_given.event_budget);
			break;
		case OPT_SHARD:
			if (sscanf(optarg, "%u/%u", &shard_i, &shard_n) != 2 || shard_n == 0 || shard_i >= shard_n) {
				fprintf(stderr, PROGRAM ": invalid option: `--shard %s'\n", optarg);
				exit(EXIT_FAILURE);
			}
			shard_given = true;
			break;
		case OPT_REPORT:
			report = 1;
			break;
		case OPT_QV:
			qv = true;
			break;
		case OPT_COMPLETENESS:
			completeness = true;
			break;
		case OPT_NO_MAP:
			no_map = true;
			break;
		case OPT_PACK:
			no_pack = false;
			break;
		case OPT_TUNE: {
			const char* eq = strchr(optarg, '=');
			if (!eq || eq == optarg) {
				fprintf(stderr, PROGRAM ": invalid option: `--tune %s'\n", optarg);
				exit(EXIT_FAILURE);
			}
			// (the value through the option parser: trailing garbage is an error, not a silent 0)
			unsigned long long tv = 0;
			{
				std::istringstream ss(eq + 1);
				ss >> tv;
				if (!ss.eof() || ss.fail() || eq[1] == '-') {
					fprintf(stderr, PROGRAM ": invalid option: `--tune %s'\n", optarg);
					exit(EXIT_FAILURE);
				}
			}
			tunes.emplace_back(std::string(optarg, eq - optarg), tv);
			break;
		}
		case OPT_HELP:
			fputs(USAGE, stderr);
			exit(EXIT_SUCCESS);
		case OPT_VERSION:
			fputs(PROGRAM " (MI355X HIP hot path)\n", stderr);
			exit(EXIT_SUCCESS);
		default:
			break;
		}
	}
	time_t rawtime;
	time(&rawtime);
	printf("---------- initializing                             : %s", ctime(&rawtime));
	if (draft_given.empty()) {
		fprintf(stderr, PROGRAM ": error: need to specify assembly draft file (-f)\n");
		die = true;
	} else {
		die_unreadable(draft_given);
	}
	if (completeness && (!qv || shard_given || counts)) {
		// (before the device is opened and before any file is written)
		fprintf(stderr, PROGRAM ": error: --completeness%s\n",
		        !qv           ? ": only with --qv (it marks the k-mers the QV screenings find present)"
		        : shard_given ? " and --shard: the marks of the shards would need a merge of their own; run it on the whole draft"
		                      : " and --counts: completeness takes a plain filter; a counting filter's slots are counters");
		exit(EXIT_FAILURE);
	}
	if (qv && shard_given) {
		// (before the device is opened and before any file is written)
		fprintf(stderr, PROGRAM ": error: --qv and --shard: a table per shard would need a merge of its own; run --qv on the whole draft\n");
		exit(EXIT_FAILURE);
	}
	if (ro.k && strchr(ro.k, ',')) {
		// every refusal of a list of k before the device is opened and before any file is written
		const std::string why = nte_host::k_list_rules(ro.k, reads_mode, shard_given, !prefix_given.empty(),
		                                     { { "--save_bf", save_bf_given }, { "--save_reject_bf", save_reject_bf_given }, { "--hist", hist_given } },
		                                     &k_list);
		if (!why.empty()) {
			refuse(why);
		}
	}
	if (genome_mode) {
		// every refusal of --genome before the device is opened and before any file is written
		const std::string why = genome_rules(ro, !bf_given.empty(), reads_mode, shard_given, genome_files.size(), reads_only, &gr);
		if (!why.empty()) {
			refuse(why);
		}
		for (const std::string& g : genome_files) {
			die_unreadable(g);
			paths.push_back(g.c_str());
		}
	} else if (reads_mode) {
		// every refusal of --reads before the device is opened and before any file is written
		if (!bf_given.empty()) {
			refuse("--reads and -r: give one of them (--reads builds the filter that -r would load)");
		}
		if (read_files.empty()) {
			refuse("--reads: 1 or more files expected");
		}
		if (shard_given) {
			refuse("--reads and --shard: every shard would build the whole filter again; build it once with "
			       "ntedit-make-reads-bf and give each shard -r");
		}
		if (ro.reject_cutoff && !bfrep_given.empty()) {
			refuse("--reject_cutoff and -e: give one of them (--reject_cutoff builds the filter that -e would load)");
		}
		for (const std::string& r : read_files) {
			paths.push_back(r.c_str());
		}
		ro.counts = counts;
		ro.files = paths.data(); // (for the default sketch: their sizes)
		ro.n_files = (uint32_t)paths.size();
		if (k_list.empty()) {
			rounds[0] = reads_rules(ro, 1);
		} else {
			// (every option but -k applies to every round alike; sizes taken from the histogram are found per round)
			rounds.clear();
			for (const std::string& kt : k_list) {
				ro.k = kt.c_str();
				rounds.push_back(reads_rules(ro, 1));
			}
		}
		for (const std::string& r : read_files) {
			die_unreadable(r);
		}
	} else if (!reads_only.empty()) {
		// (the options --genome shares with --reads say so)
		static const char* const shared[] = { "--hashes", "--fpr", "--bf", "--num_elements", "--save_bf", "--gpu_parse", "--batch_bytes" };
		bool both = false;
		for (const char* o : shared) {
			both = both || reads_only[0] == o;
		}
		refuse(reads_only[0] + (both ? ": only with --reads or --genome" : ": only with --reads"));
	} else if (bf_given.empty()) {
		fprintf(stderr, PROGRAM ": error: need to specify the Bloom filter file (-r)\n");
		die = true;
	} else {
		die_unreadable(bf_given);
	}
	if (!bfrep_given.empty()) {
		die_unreadable(bfrep_given);
	}
	if (die) {
		fprintf(stderr, "Try `" PROGRAM " --help' for more information.\n");
		exit(EXIT_FAILURE);
	}
	if (p_given.snv) {
		// ntedit.cpp:2411-2417
		fprintf(stderr, "\nSNV mode ON\nTracking all single-base variants\nNote: -i and -d both set to 0 when -s is set to 1\n"
		                "Consider -l clinvar.vcf to identify SNVs with putative clinical significance\n\n");
	}

	ntedit_hip_ctx* ctx = nullptr;
	if (ntedit_hip_create(gpu, &ctx) != 0) {
		fprintf(stderr, PROGRAM ": error: no usable HIP device %d (this build has no CPU path).\n", gpu);
		exit(EXIT_FAILURE);
	}
	for (const auto& t : tunes) {
		if (t.first == "host_zlib") {
			// (a host-side switch, not the library's: 1 = inflate .gz drafts through zlib instead of host/gunzip.cpp)
			nte_host::set_gzip_through_zlib((int)t.second);
			continue;
		}
		if (ntedit_hip_set_tuning(ctx, t.first.c_str(), t.second) != 0) {
			fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
			exit(EXIT_FAILURE);
		}
	}
	// every thread and batch buffer from here on: on the socket the GPU hangs off
	(void)ntedit_hip_bind_near_device(gpu);
	// Batch buffers: page-locked (asynchronous H2D at link speed, no staging copies inside the polish_batch calls: 0.42 s ->
	// 0.2 s of calls per 3 Gbp), allocated by a side thread WHILE the filter file loads -- i.e. before the
	// "reading/processing" stamp, like everything else the reference does before it (ntedit.cpp:2564-2589).  Round 2 had
	// measured page-locking as a loss because it paid for it inside the timed region, three buffers of 1 GiB.
	Work pool[3];
	const unsigned long long batch_cap_bases = batch_given ? batch_bases : (1ull << 30);
	size_t pin_bytes = (size_t)(batch_cap_bases < (1ull << 32) ? batch_cap_bases : (1ull << 32)) + (size_t)(64u << 20);
	{
		//  a small draft does not pay for the largest batch: a plain FASTA file holds no more bases than it has
		// bytes (3 x 1 GiB of page-locked memory and ~30 GB of device buffers for a 5 Mbp draft otherwise).  Compressed
		// drafts keep the full size: their length is not known in advance.
		struct stat sb;
		FILE* probe = fopen(draft_given.c_str(), "rb");
		if (probe) {
			unsigned char magic[2] = { 0, 0 };
			const bool gz = fread(magic, 1, 2, probe) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
			if (!gz && fstat(fileno(probe), &sb) == 0 && S_ISREG(sb.st_mode)) {
				const size_t by_file = (size_t)sb.st_size + (size_t)(4u << 20);
				if (by_file < pin_bytes) {
					pin_bytes = by_file;
				}
			}
			fclose(probe);
		}
	}
	std::thread pin_thread([&]() {
		(void)ntedit_hip_bind_near_device(gpu);
		if (no_map || getenv("NTEDIT_NO_PINNED_BATCHES")) {
			return;
		}
		for (Work& w : pool) {
			char* m = (char*)ntedit_hip_host_alloc(pin_bytes);
			if (!m) {
				return; // (ordinary memory then: reserve_raw allocates on demand)
			}
			w.b.raw = m;
			w.b.raw_cap = pin_bytes;
			w.b.raw_pinned = true;
		}
	});
	auto fatal = [&]() {
		fflush(nullptr);
		_exit(EXIT_FAILURE); // (_exit: the side thread above may still be running)
	};
	// One round: build or load the filter, echo the parameters, polish `draft_in`, write the three outputs under
	// `prefix_in`.  A run is one round, or with --reads -k K1,K2,...,Kn a cascade of n: round i + 1 polishes round i's
	// _edited.fa (through the file: 1/30 of the data, and every round stays byte-comparable with a stand-alone run), and
	// from round 2 on every pass of the filter build reads the resident store that round 1 filled.
	const size_t n_rounds = rounds.size();
	bool store_lost = false; // a cascade's store was released (over its cap, no memory, the polish buffers): no round tries it again
	auto polish_round = [&](size_t round, const std::string& draft_in, const std::string& prefix_in) {
		const bool cascade = n_rounds > 1, last_round = round + 1 == n_rounds;
		const ntedit_hip_reads_rules& rr = rounds[round];
		const std::string& draft = draft_in;
		ntedit_hip_params p = p_given;
		std::string bf = bf_given, bfrep = bfrep_given, prefix = prefix_in;
		// (with a list of k the names of the saved files carry {k}: this round's k goes there)
		const std::string hist_out = cascade ? nte_host::with_k(hist_given, rr.k) : hist_given,
		                  save_bf = cascade ? nte_host::with_k(save_bf_given, rr.k) : save_bf_given,
		                  save_reject_bf = cascade ? nte_host::with_k(save_reject_bf_given, rr.k) : save_reject_bf_given;
		bool store_held = false; // the resident store stays in HBM while this round polishes (for the next round)
		time(&rawtime);
		if (genome_mode) {
			// the filter ntedit-make-genome-bf would write, built into the primary slot (genome_pass.cpp): sized as the tool
			// sizes it, every k-mer of every record of k bases or more inserted; without --gpu_parse the host parser reads
			// the files (batch_bytes 0)
			printf("---------- building Bloom filter from genome        : %s\n", ctime(&rawtime));
			fflush(stdout);
			const auto g0 = std::chrono::steady_clock::now();
			const uint64_t batch = gr.gpu_parse ? gr.batch_bytes : 0;
			auto pass = [&](int insert) {
				ntedit_hip_reads_pass_stats st;
				if (ntedit_hip_genome_pass(ctx, NTEDIT_FILTER_PRIMARY, paths.data(), (uint32_t)paths.size(), batch, insert, &st) != 0) {
					fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_reads_last_error(ctx));
					fatal();
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
					fprintf(stderr, PROGRAM ": error: --genome: no bases in the genome files: the filter would be empty\n");
					fatal();
				}
			}
			printf("BF size (bytes): %llu\n", (unsigned long long)bf_size);
			if (ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_PRIMARY, bf_size, gr.hash_num, gr.k) != 0) {
				fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
				fatal();
			}
			(void)pass(1);
			ntedit_hip_sketch_free(ctx); // (the device parser's scratch: the polish sizes its own buffers next)
			printf("Genome filter built in %.1f ms\n",
			       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count());
			if (!save_bf.empty()) {
				if (ntedit_hip_filter_save_file(ctx, NTEDIT_FILTER_PRIMARY, save_bf.c_str()) != 0) {
					fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", save_bf.c_str());
					fatal();
				}
				printf("Bloom filter saved to %s\n", save_bf.c_str());
			}
			// (the _r part of the default prefix: the name ntedit-make-genome-bf would have written it under)
			bf = save_bf.empty() ? "genome_bf.bf" : save_bf;
		} else if (reads_mode) {
			// the filter ntedit-make-reads-bf would write, built into the primary slot (reads_pass.cpp); the reads stay
			// resident in HBM after pass 1 unless they would pass store_cap, so that the later passes do not parse them again
			if (cascade) {
				printf("---------- round %zu of %zu: k = %u\n", round + 1, n_rounds, rr.k);
			}
			printf("---------- building Bloom filter from reads         : %s\n", ctime(&rawtime));
			fflush(stdout);
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
			ba.use_store = 1;
			ba.store_cap = rr.store_cap;
			ba.device_parse = rr.gpu_parse;
			ba.reject_cmin = rr.reject_cmin;
			ba.reject_bf_bytes = rr.reject_bf_bytes;
			ba.reject_num_elements = rr.reject_num_elements;
			if (cascade) {
				// round 1 fills the store with every read a later round has to count (the shortest k decides) and every
				// round but the last leaves it to the next; a round that finds it ON reads nothing else
				uint32_t min_k = rr.k;
				for (const ntedit_hip_reads_rules& other : rounds) {
					min_k = other.k < min_k ? other.k : min_k;
				}
				// (every round that reads files keeps the reads of min_k bases or more: whichever round fills the store, a
				// later round at a smaller k finds in it all it has to count)
				ba.min_read = min_k;
				ba.keep_store = last_round ? 0 : 1;
				// a store that was released once is not tried again: every later round reads the files, as separate runs would
				ba.use_store = store_lost ? 0 : 1;
			}
			ba.log = nte_host::reads_log;
			ntedit_hip_reads_build_result br;
			if (ntedit_hip_reads_build(ctx, &ba, &br) != 0) {
				fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_reads_last_error(ctx));
				fatal();
			}
			if (br.from_store) {
				printf("Reads filter built in %.1f ms (minimum count %u; pass 1, the histogram pass and pass 2 read the resident store)\n",
				       br.ms_total, br.cmin);
			} else {
				printf("Reads filter built in %.1f ms (minimum count %u; the histogram pass and pass 2 read %s)\n", br.ms_total,
				       br.cmin, br.store_state == NTEDIT_RESIDENT_ON ? "the resident store" : "the files");
			}
			if (cascade) {
				printf("Round %zu of %zu: k = %u, minimum count %u, %s\n", round + 1, n_rounds, rr.k, br.cmin,
				       br.from_store                             ? "every pass read the resident store, no read file was opened"
				       : br.store_state == NTEDIT_RESIDENT_ON ? "pass 1 read the files and filled the resident store, the later passes read it"
				                                                 : "every pass read the files (the resident store was released)");
			}
			store_held = cascade && !last_round && br.store_state == NTEDIT_RESIDENT_ON;
			store_lost = store_lost || (cascade && br.store_state != NTEDIT_RESIDENT_ON);
			if (!save_bf.empty()) {
				if (ntedit_hip_filter_save_file(ctx, NTEDIT_FILTER_PRIMARY, save_bf.c_str()) != 0) {
					fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", save_bf.c_str());
					fatal();
				}
				printf("Bloom filter saved to %s\n", save_bf.c_str());
			}
			// the reject filter, built into the secondary slot by the same pass 2: no -e file is loaded
			if (rr.reject_cmin) {
				printf("Reject filter built (reject count %u, %llu bytes)\n", rr.reject_cmin, (unsigned long long)br.reject_bf_bytes);
				if (!save_reject_bf.empty()) {
					if (ntedit_hip_filter_save_file(ctx, NTEDIT_FILTER_SECONDARY, save_reject_bf.c_str()) != 0) {
						fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", save_reject_bf.c_str());
						fatal();
					}
					printf("Reject Bloom filter saved to %s\n", save_reject_bf.c_str());
				}
				// (the -e line of the parameter echo; the reference's prefix has no -e part)
				bfrep = save_reject_bf.empty() ? "reads_k" + std::to_string(rr.k) + "_reject.bf" : save_reject_bf;
			}
			// (the _r part of the default prefix: the name ntedit-make-reads-bf would have written it under)
			bf = save_bf.empty() ? "reads_k" + std::to_string(rr.k) + ".bf" : save_bf;
		} else {
			printf("---------- loading Bloom filter from file           : %s\n", ctime(&rawtime));
			if (ntedit_hip_load_filter_file(ctx, NTEDIT_FILTER_PRIMARY, bf.c_str()) != 0) {
				fprintf(stderr, PROGRAM ": error: Bloom filter file supplied (-r) is incorrect. (%s)\n", ntedit_hip_last_error(ctx));
				fatal();
			}
		}
		uint32_t k = 0, h = 0;
		uint64_t nbytes = 0;
		int counting = 0;
		ntedit_hip_filter_info(ctx, NTEDIT_FILTER_PRIMARY, &k, &h, &nbytes, &counting);
		printf("BLOOM::\tcounting: %s\tsize: %llu\tnumber hash functions: %u\tkmer size: %u\n", counting ? "YES" : "NO",
		       (unsigned long long)nbytes, h, k);
		if (completeness && counting) {
			// (before any output file is opened and before a batch is polished)
			fprintf(stderr, PROGRAM ": error: --completeness: `%s' is a counting filter; completeness takes a plain filter\n", bf.c_str());
			fatal();
		}
		if (!counting && p.min_threshold != 1) {
			// ntedit.cpp:2453-2458
			fprintf(stderr, PROGRAM ": warning: Bloom filter is not counting, min k-mer presence threshold will be set to 1.\n");
			p.min_threshold = 1;
		}
		time(&rawtime);
		printf("\n---------- verifying parameters                     : %s", ctime(&rawtime));
		char warn[1024];
		ntedit_hip_params_clamp(&p, warn, sizeof warn);
		if (warn[0]) {
			fputs(warn, stderr);
		}
		if (prefix.empty()) {
			// ntedit.cpp:2496-2502
			std::ostringstream o;
			o << base_name(draft) << "_k" << k << "_z" << p.min_contig_len << "_r" << base_name(bf) << "_i"
			  << p.max_insertions << "_d" << p.max_deletions << "_m" << p.mode;
			prefix = o.str();
		}
		printf("\nrunning : " PROGRAM " (MI355X HIP hot path)\n -f %s\n -k %u\n -z %u\n -b %s\n -r %s\n -e %s\n -i %u\n -d %u",
		       base_name(draft).c_str(), k, p.min_contig_len, prefix.c_str(), base_name(bf).c_str(),
		       base_name(bfrep).c_str(), p.max_insertions, p.max_deletions);
		if (p.use_ratio) {
			printf("\n -X %g\n -Y %g", p.missing_ratio, p.edit_ratio);
		} else {
			printf("\n -x %g\n -y %g", p.missing_threshold, p.edit_threshold);
		}
		printf("\n -j %u\n -m %d\n -s %d\n -l %s\n -a %d\n -t %u\n -v %d\n\n", p.jump, p.mode, p.snv, base_name(vcf).c_str(),
		       p.mask, nthreads, verbose);
		if (counting) {
			printf(" -p %u\n -q %u\n\n", p.min_threshold, p.max_threshold); // ntedit.cpp:2519-2522
		}

		if (!bfrep.empty()) {
			time(&rawtime);
			if (rr.reject_cmin) {
				printf("---------- secondary Bloom filter built from reads   : %s\n", ctime(&rawtime));
			} else {
				printf("---------- loading secondary Bloom filter from file : %s\n", ctime(&rawtime));
				if (ntedit_hip_load_filter_file(ctx, NTEDIT_FILTER_SECONDARY, bfrep.c_str()) != 0) {
					fprintf(stderr, PROGRAM ": error: secondary Bloom filter file supplied (-e) is incorrect.\n");
					fatal();
				}
			}
			uint32_t k2 = 0;
			ntedit_hip_filter_info(ctx, NTEDIT_FILTER_SECONDARY, &k2, nullptr, nullptr, nullptr);
			if (k2 != k) {
				fprintf(stderr, PROGRAM ": error: secondary Bloom filter k size (%u) is different than main Bloom filter k size (%u)\n", k2, k);
				fatal();
			}
		}
		if (ntedit_hip_set_params(ctx, &p) != 0) {
			fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
			fatal();
		}
		// start-up, like the filter load: the context's buffers for the largest batch + one internal warm-up batch, so that
		// the first polish_batch call costs what the later ones do (ntedit_hip_reserve)
		if (qv && ntedit_hip_set_apply(ctx, NTEDIT_HIP_APPLY_QV | (completeness ? NTEDIT_HIP_APPLY_SHARED : 0u)) != 0) {
			fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
			fatal();
		}
		// --completeness: the two mark arrays of this round's filter, mapped here and not inside the first batch
		if (completeness && ntedit_hip_shared_begin(ctx) != 0) {
			fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
			fatal();
		}
		int reserved = ntedit_hip_reserve(ctx, pin_bytes, 1u << 16, 0, no_pack ? NTEDIT_HIP_BASES_HOST : NTEDIT_HIP_BASES_PACKED);
		if (reserved != 0 && store_held) {
			// the store is held for the next round: when the polish buffers do not fit beside it, it goes, and the later
			// rounds read the files
			ntedit_hip_sketch_free(ctx);
			store_lost = true;
			printf("Resident store: released (the polish buffers of round %zu did not fit beside it); the later rounds read the files\n",
			       round + 1);
			reserved = ntedit_hip_reserve(ctx, pin_bytes, 1u << 16, 0, no_pack ? NTEDIT_HIP_BASES_HOST : NTEDIT_HIP_BASES_PACKED);
		}
		if (reserved != 0) {
			// (optional: the buffers then grow on demand, inside the first calls)
			fprintf(stderr, PROGRAM ": warning: buffers could not be sized ahead (%s); they grow on demand\n", ntedit_hip_last_error(ctx));
		}
		if (pin_thread.joinable()) {
			pin_thread.join();
		}

		time(&rawtime);
		printf("---------- reading/processing input sequence        : %s", ctime(&rawtime));
		const auto t0 = std::chrono::steady_clock::now(); // (--report: this stamp -> "process complete")
		const std::string fa_path = prefix + "_edited.fa", tsv_path = prefix + "_changes.tsv",
		                  vcf_path = prefix + "_variants.vcf";
		{
			FILE* f = fopen(fa_path.c_str(), "wb");
			if (!f) {
				fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", fa_path.c_str());
				fatal();
			}
			fclose(f);
		}
		if (ntedit_hip_write_tsv_header(tsv_path.c_str(), k, p.jump, counting) != 0) {
			fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", tsv_path.c_str());
			fatal();
		}
		if (ntedit_hip_write_vcf_header(vcf_path.c_str(), draft.c_str()) != 0) { // ntedit.cpp:2192-2211
			fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", vcf_path.c_str());
			fatal();
		}
		// --qv: <prefix>_qv.tsv, a row per written contig as the batches come back, "#total" at the end
		const std::string qv_path = prefix + "_qv.tsv";
		FILE* qv_f = nullptr;
		ntedit_hip_qv_row qv_tot;
		memset(&qv_tot, 0, sizeof qv_tot);
		double ms_apply = 0, ms_qv_screen = 0, ms_qv_count = 0;
		if (qv) {
			qv_f = fopen(qv_path.c_str(), "wb");
			if (!qv_f) {
				fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", qv_path.c_str());
				fatal();
			}
			fputs(ntedit_hip_qv_header(), qv_f);
		}
		ntedit_hip_annot* annot = nullptr;
		if (!vcf.empty()) {
			// -l: annotated variants (e.g. clinvar.vcf[.gz]), ntedit.cpp:2524-2562
			die_unreadable(vcf);
			if (ntedit_hip_annot_load(vcf.c_str(), &annot) != 0) {
				fprintf(stderr, "Unable to open file\n");
			}
		}

		// Plain multi-FASTA files are taken apart by several threads from a mapping of the file (fasta_map.h); anything
		// else (gzip, FASTQ, CR line ends, ...) goes through the streaming reader.  --no-map forces the latter.
		unsigned ingest_threads = threads_given ? nthreads : std::thread::hardware_concurrency();
		if (ingest_threads > 16) {
			ingest_threads = 16;
		}
		if (ingest_threads < 1) {
			ingest_threads = 1;
		}
		// (BGZF members are inflated before that: compute-bound, so on more threads than the memory-bound parse)
		unsigned inflate_threads = threads_given ? nthreads : std::thread::hardware_concurrency();
		if (inflate_threads > 64) {
			inflate_threads = 64;
		}
		const auto tm0 = std::chrono::steady_clock::now();
		nte_host::FastaMap fmap(no_map ? "" : draft.c_str(), ingest_threads, inflate_threads);
		const double s_index = std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
		const double s_before_index = std::chrono::duration<double>(tm0 - t0).count();

		// --shard I/N: the contigs >= -z are split by bases, greedy longest-first (the partition of
		// ntedit_amd.dist.shard_contigs): a first pass over the draft collects the lengths
		std::vector<uint8_t> mine; // by ordinal
		if (shard_n > 1) {
			std::vector<uint64_t> lens;
			if (fmap.ok()) {
				fmap.measure(0, fmap.records());
				for (size_t i = 0; i < fmap.records(); i++) {
					if (fmap.length(i) >= p.min_contig_len) {
						lens.push_back(fmap.length(i));
					}
				}
			} else {
				nte_host::FastaReader scan(draft.c_str());
				if (!scan.ok()) {
					fprintf(stderr, PROGRAM ": error: `%s': cannot open\n", draft.c_str());
					fatal();
				}
				std::string h, sq;
				while (scan.next(h, sq)) {
					const void* z = memchr(sq.data(), 0, sq.size());
					const size_t len = z ? (size_t)((const char*)z - sq.data()) : sq.size();
					if (len >= p.min_contig_len) {
						lens.push_back(len);
					}
					sq.clear();
				}
				if (scan.io_error()) {
					// (a partition computed from half a draft would differ between the shards)
					fprintf(stderr, PROGRAM ": error: `%s': %s\n", draft.c_str(), scan.io_error_text().c_str());
					fatal();
				}
			}
			std::vector<uint32_t> order(lens.size());
			for (size_t i = 0; i < order.size(); i++) {
				order[i] = (uint32_t)i;
			}
			std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
			std::vector<uint64_t> load(shard_n, 0);
			mine.assign(lens.size(), 0);
			for (uint32_t i : order) {
				unsigned best = 0;
				for (unsigned r = 1; r < shard_n; r++) {
					if (load[r] < load[best]) {
						best = r;
					}
				}
				load[best] += lens[i];
				mine[i] = best == shard_i;
			}
		}
		// (the streaming reader and its inflate thread only when the mapped reader does not serve the run)
		std::unique_ptr<nte_host::FastaReader> reader_p;
		if (!fmap.ok()) {
			reader_p.reset(new nte_host::FastaReader(draft.c_str()));
		}
		if (reader_p && !reader_p->ok()) {
			fprintf(stderr, PROGRAM ": error: `%s': cannot open\n", draft.c_str());
			fatal();
		}
		FILE* index_f = nullptr;
		if (shard_n > 1) {
			index_f = fopen((prefix + ".index.tsv").c_str(), "wb");
			if (!index_f) {
				fprintf(stderr, PROGRAM ": error: cannot write `%s.index.tsv'\n", prefix.c_str());
				fatal();
			}
			fprintf(index_f, "#shard %u/%u\tordinal\tfa_bytes\ttsv_bytes\tvcf_bytes\n", shard_i, shard_n);
		}
		if (threads_given) {
			ntedit_hip_set_host_threads(nthreads); // -t: contigs rendered concurrently
		}
		unsigned long long n_contigs = 0, total_bases = 0;
		double ms_gpu = 0, ms_screen = 0, ms_machine = 0, s_call = 0, s_write = 0, s_read = 0;
		unsigned n_batches_binned = 0, n_batches_direct = 0, n_chunks_direct = 0;
		unsigned long long n_ovf_records = 0;
		ntedit_hip_stats tot;
		memset(&tot, 0, sizeof tot);

		// Batch sizes.  End to end the writer is the slowest stage (a write() per output byte into the page cache), so the
		// run takes the writer's time plus what passes before its first byte: unless the user fixes the size, the first
		// batches are small (128 Mbases, doubling: the writer starts after 30 ms instead of 120) and grow to 1 Gbase -- every
		// batch costs the writer a start-up of its own (round 5: 3 Gbp in 7 batches of <= 512 Mbases 0.52 s of writer time,
		// in 3 of 1 Gbase 0.43 s).
		unsigned long long budget = batch_bases;
		if (!batch_given) {
			batch_bases = 1ull << 30;
			budget = 1ull << 27;
		}
		// Three stages, one batch each at a time: this thread's reader helper parses the draft
		// into batch N+1 while the GPU polishes batch N and the writer renders batch N-1.
		// Output order = input order (the reference at -t 1).
		Channel free_q, gpu_q, write_q;
		for (Work& w : pool) {
			free_q.push(&w);
		}
		for (Work& w : pool) {
			// (address space only: pages are touched as the batch fills)
			w.b.blob.reserve((size_t)(batch_bases < (1ull << 32) ? batch_bases : (1ull << 32)) + (1 << 20));
			// first touch of a fresh batch buffer is a page fault per 4 KiB: ask for huge pages
			const uintptr_t lo = ((uintptr_t)w.b.blob.data() + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
			const uintptr_t hi = ((uintptr_t)w.b.blob.data() + w.b.blob.capacity()) & ~(uintptr_t)((2u << 20) - 1);
			if (hi > lo) {
				(void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
			}
		}
		std::thread reader_thread([&]() {
			std::string hdr;
			unsigned long long idx = 0;
			Work* w = free_q.pop();
			auto tr0 = std::chrono::steady_clock::now();
			auto hand_over = [&](Work* next) {
				if (!no_pack && w->b.size()) {
					// (--pack.  Measured on the 3 Gbp draft: the GPU stage gains ~10 ms per 3 GB, packing costs the reader stage
					// 0.5 s on 4 threads -- 1 GB/s per thread, a table look-up per byte -- and puts it on the critical path:
					// 0.94 s end to end against 0.67 s.  Off by default; the packed form pays where the producer has
					// cycles to spare or emits it directly.)
					const uint64_t need = ntedit_hip_packed_size(w->b.size());
					if (w->b.packed.size() < need) {
						w->b.packed.resize(need + need / 8);
					}
					w->b.is_packed = ntedit_hip_pack_bases(w->b.data(), w->b.size(), w->b.packed.data(), nthreads) == 0;
				}
				s_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
				gpu_q.push(w);
				w = next;
				budget = budget * 2 < batch_bases ? budget * 2 : batch_bases;
				tr0 = std::chrono::steady_clock::now();
			};
			if (fmap.ok()) {
				// ---- mapped reader: pick the records of a batch, measure / copy them concurrently
				const size_t N = fmap.records();
				size_t i = 0;
				std::vector<size_t> pick;
				std::vector<char*> dst;
				const size_t GROUP = 1024;
				size_t measured = 0;
				while (i < N) {
					Batch& b = w->b;
					pick.clear();
					size_t total = 0;
					while (i < N) {
						if (i >= measured) {
							const size_t cnt = N - measured < GROUP ? N - measured : GROUP;
							fmap.measure(measured, cnt);
							measured += cnt;
						}
						const uint64_t len = fmap.length(i);
						bool keep = false;
						if (len >= p.min_contig_len) { // ntedit.cpp:2242
							keep = shard_n == 1 || (idx < mine.size() && mine[idx]);
						}
						if (keep) {
							if (len > 0xFFFFFFF0ull) {
								fprintf(stderr, PROGRAM ": error: contig longer than 2^32 bases\n");
								fflush(nullptr);
								_exit(EXIT_FAILURE);
							}
							if (!pick.empty() && total + len + 1 > budget) {
								break; // the batch is full: this contig opens the next one
							}
							b.offs.push_back(total);
							b.lens.push_back((uint32_t)len);
							b.names.push_back(fmap.header(i));
							b.ordinals.push_back(idx);
							pick.push_back(i);
							total += len + 1;
							total_bases += len;
						}
						if (len >= p.min_contig_len) {
							idx++;
						}
						n_contigs++;
						if (n_contigs % 1000000 == 0) {
							printf("Processed %llu\n", n_contigs);
						}
						i++;
					}
					if (!pick.empty()) {
						if (!b.reserve_raw(total)) {
							fprintf(stderr, PROGRAM ": error: out of memory for a batch of %zu bytes\n", total);
							fflush(nullptr);
							_exit(EXIT_FAILURE);
						}
						dst.resize(pick.size());
						for (size_t q = 0; q < pick.size(); q++) {
							dst[q] = b.raw + b.offs[q];
							b.raw[b.offs[q] + b.lens[q]] = '\n';
						}
						fmap.copy(pick.data(), dst.data(), pick.size());
						b.raw_n = total;
					}
					if (i < N) {
						s_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
						Work* nx = free_q.pop();
						tr0 = std::chrono::steady_clock::now();
						hand_over(nx);
					}
				}
				hand_over(nullptr);
				gpu_q.push(nullptr);
				return;
			}
			for (;;) {
				Batch& b = w->b;
				const size_t before = b.blob.size();
				if (!reader_p->next(hdr, b.blob)) {
					break;
				}
				n_contigs++;
				// strings holding an embedded NUL end there in the reference (contigSeq = seq->seq.s)
				const void* z = memchr(b.blob.data() + before, 0, b.blob.size() - before);
				if (z) {
					b.blob.resize((size_t)((const char*)z - b.blob.data()));
				}
				const size_t len = b.blob.size() - before;
				bool keep = false;
				if (len >= p.min_contig_len) { // ntedit.cpp:2242
					keep = shard_n == 1 || (idx < mine.size() && mine[idx]);
					idx++;
				}
				if (!keep) {
					b.blob.resize(before);
				} else {
					if (len > 0xFFFFFFF0ull) {
						fprintf(stderr, PROGRAM ": error: contig longer than 2^32 bases\n");
						fflush(nullptr);
						_exit(EXIT_FAILURE);
					}
					if (!b.names.empty() && b.blob.size() + 1 > budget) {
						// the batch is full: this contig opens the next one
						s_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
						Work* nx = free_q.pop();
						tr0 = std::chrono::steady_clock::now();
						nx->b.blob.assign(b.blob, before, std::string::npos);
						b.blob.resize(before);
						hand_over(nx);
						Batch& nb = w->b;
						nb.offs.push_back(0);
						nb.lens.push_back((uint32_t)len);
						nb.names.push_back(hdr);
						nb.ordinals.push_back(idx - 1);
						nb.blob.push_back('\n');
					} else {
						b.offs.push_back(before);
						b.lens.push_back((uint32_t)len);
						b.names.push_back(hdr);
						b.ordinals.push_back(idx - 1);
						b.blob.push_back('\n');
					}
					total_bases += len;
				}
				if (n_contigs % 1000000 == 0) {
					printf("Processed %llu\n", n_contigs);
				}
			}
			hand_over(nullptr); // (possibly empty) last batch
			gpu_q.push(nullptr);
		});
		std::thread writer_thread([&]() {
			while (Work* w = write_q.pop()) {
				Batch& b = w->b;
				auto tw0 = std::chrono::steady_clock::now();
				std::vector<const char*> names(b.names.size());
				for (size_t i = 0; i < b.names.size(); i++) {
					names[i] = b.names[i].c_str();
				}
				ntedit_hip_write_options wo;
				memset(&wo, 0, sizeof wo);
				wo.fa_path = fa_path.c_str();
				wo.tsv_path = tsv_path.c_str();
				wo.vcf_path = vcf_path.c_str();
				wo.append = 1;
				wo.annot = annot;
				std::vector<uint64_t> sizes;
				if (index_f) {
					sizes.assign(names.size() * 3 + 3, 0);
					wo.out_sizes = sizes.data();
				}
				int rc = ntedit_hip_write_outputs_ex(w->res, b.data(), b.offs.data(), b.lens.data(), names.data(),
				                                     (uint32_t)names.size(), &wo);
				if (rc != 0) {
					fprintf(stderr, PROGRAM ": error: cannot write outputs\n");
					fflush(nullptr);
					_exit(EXIT_FAILURE);
				}
				if (index_f) {
					for (size_t i = 0; i < names.size(); i++) {
						fprintf(index_f, "%llu\t%llu\t%llu\t%llu\n", (unsigned long long)b.ordinals[i], (unsigned long long)sizes[3 * i],
						        (unsigned long long)sizes[3 * i + 1], (unsigned long long)sizes[3 * i + 2]);
					}
				}
				if (qv_f) {
					std::vector<ntedit_hip_qv_row> rows(names.size());
					std::string line;
					bool ok = ntedit_hip_result_qv(w->res, rows.data(), (uint32_t)rows.size()) == 0;
					for (size_t i = 0; ok && i < rows.size(); i++) {
						line.resize(b.names[i].size() + 256);
						ok = ntedit_hip_qv_format_row(names[i], &rows[i], k, &line[0], line.size()) == 0 && fputs(line.c_str(), qv_f) >= 0;
						qv_tot.len_before += rows[i].len_before;
						qv_tot.len_after += rows[i].len_after;
						qv_tot.kmers_before += rows[i].kmers_before;
						qv_tot.absent_before += rows[i].absent_before;
						qv_tot.kmers_after += rows[i].kmers_after;
						qv_tot.absent_after += rows[i].absent_after;
					}
					if (!ok) {
						fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", qv_path.c_str());
						fflush(nullptr);
						_exit(EXIT_FAILURE);
					}
				}
				ntedit_hip_stats st;
				ntedit_hip_result_stats(w->res, &st);
				ms_gpu += st.ms_total;
				ms_screen += st.ms_screen;
				// (which screening kernels ran: batches on the partitioned pipeline / on the direct kernel, record chunks the direct
				// kernel had to screen again, overflow-list entries)
				n_batches_binned += st.screen_binned ? 1 : 0;
				n_batches_direct += st.screen_binned ? 0 : 1;
				n_chunks_direct += st.screen_chunks_direct;
				n_ovf_records += st.screen_overflow_records;
				ms_machine += st.ms_machine;
				tot.events += st.events;
				tot.events_applied += st.events_applied;
				tot.absent_kmers += st.absent_kmers;
				tot.substitutions += st.substitutions;
				tot.insertions += st.insertions;
				tot.deletions += st.deletions;
				ntedit_hip_result_free(w->res);
				w->res = nullptr;
				b.clear();
				s_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count();
				free_q.push(w);
			}
		});
		while (Work* w = gpu_q.pop()) {
			Batch& b = w->b;
			if (b.names.empty()) {
				b.clear();
				free_q.push(w);
				continue;
			}
			auto tc0 = std::chrono::steady_clock::now();
			int rc = ntedit_hip_polish_batch(ctx, b.is_packed ? b.packed.data() : b.data(), b.size(), b.offs.data(), b.lens.data(),
			                                 (uint32_t)b.names.size(), b.is_packed ? NTEDIT_HIP_BASES_PACKED : NTEDIT_HIP_BASES_HOST, &w->res);
			if (rc != 0) {
				fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
				fflush(nullptr);
				_exit(EXIT_FAILURE);
			}
			s_call += std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count();
			if (qv) {
				ntedit_hip_apply_stats as;
				if (ntedit_hip_apply_info(ctx, &as) == 0) {
					ms_apply += as.ms_apply;
					ms_qv_screen += as.ms_screen;
					ms_qv_count += as.ms_count;
				}
			}
			write_q.push(w);
		}
		write_q.push(nullptr);
		reader_thread.join();
		writer_thread.join();
		if (index_f && fclose(index_f) != 0) {
			fprintf(stderr, PROGRAM ": error: cannot write `%s.index.tsv'\n", prefix.c_str());
			exit(EXIT_FAILURE);
		}
		if (reader_p && reader_p->io_error()) {
			// a corrupt / truncated input must not pass for a (shorter) genome
			fprintf(stderr, PROGRAM ": error: `%s': %s -- the outputs are incomplete\n", draft.c_str(), reader_p->io_error_text().c_str());
			fflush(nullptr);
			_exit(EXIT_FAILURE);
		}
		auto t1 = std::chrono::steady_clock::now();
		time(&rawtime);
		printf("---------- process complete                         : %s", ctime(&rawtime));
		if (qv_f) {
			char line[512];
			bool ok = ntedit_hip_qv_format_row("#total", &qv_tot, k, line, sizeof line) == 0 && fputs(line, qv_f) >= 0;
			ok = fclose(qv_f) == 0 && ok;
			if (!ok) {
				fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", qv_path.c_str());
				exit(EXIT_FAILURE);
			}
			auto qv_text = [&](uint64_t absent, uint64_t kmers) {
				const double q = ntedit_hip_qv_value(absent, kmers, k);
				char t[32];
				if (q != q) {
					return std::string("NA");
				}
				snprintf(t, sizeof t, "%.2f", q);
				return std::string(q > 1e300 ? "inf" : t);
			};
			uint64_t occ = 0, slots = 0;
			uint32_t hn = 0;
			ntedit_hip_filter_info(ctx, NTEDIT_FILTER_PRIMARY, nullptr, &hn, nullptr, nullptr);
			double fpr = 0;
			if (ntedit_hip_filter_occupancy(ctx, NTEDIT_FILTER_PRIMARY, &occ, &slots) == 0 && slots) {
				fpr = pow((double)occ / (double)slots, (double)hn);
			}
			printf("k-mer QV (k=%u): before %s (%llu of %llu k-mers absent), after %s (%llu of %llu); Bloom false positives make "
			       "`absent' an undercount by about the filter's false-positive rate (occupancy^h = %.3g); table: %s\n",
			       k, qv_text(qv_tot.absent_before, qv_tot.kmers_before).c_str(), (unsigned long long)qv_tot.absent_before,
			       (unsigned long long)qv_tot.kmers_before, qv_text(qv_tot.absent_after, qv_tot.kmers_after).c_str(),
			       (unsigned long long)qv_tot.absent_after, (unsigned long long)qv_tot.kmers_after, fpr, qv_path.c_str());
		}
		if (completeness) {
			// --completeness: <prefix>_completeness.tsv and one line, from the marks of all batches of this round
			const std::string cp_path = prefix + "_completeness.tsv";
			ntedit_hip_shared_stats ss;
			if (ntedit_hip_shared_counts(ctx, &ss) != 0) {
				fprintf(stderr, PROGRAM ": error: %s\n", ntedit_hip_last_error(ctx));
				exit(EXIT_FAILURE);
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
				fprintf(stderr, PROGRAM ": error: cannot write `%s'\n", cp_path.c_str());
				exit(EXIT_FAILURE);
			}
			const double filter_kmers = ntedit_hip_bloom_cardinality(ss.filter_set, ss.bits, ss.hash_num);
			const double shared_kmers[2] = { ntedit_hip_bloom_cardinality(ss.shared_set[0], ss.bits, 1),
				                             ntedit_hip_bloom_cardinality(ss.shared_set[1], ss.bits, 1) };
			auto share = [&](int w) { // (the ratio of two estimates; NaN where the table says NA)
				return std::isfinite(filter_kmers) && std::isfinite(shared_kmers[w]) && filter_kmers != 0 ? shared_kmers[w] / filter_kmers : std::nan("");
			};
			auto count_text = [](double v) { return std::isfinite(v) ? std::to_string(std::llround(v)) : std::string("NA"); };
			auto percent_text = [](double v) {
				char t[32];
				snprintf(t, sizeof t, "%.4f %%", 100.0 * v);
				return std::isfinite(v) ? std::string(t) : std::string("NA");
			};
			auto json_num = [](double v, const char* fmt) {
				char t[48];
				snprintf(t, sizeof t, fmt, v);
				return std::isfinite(v) ? std::string(t) : std::string("null");
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
		if (report && qv) {
			printf("{\"qv\": {\"kmers_before\": %llu, \"absent_before\": %llu, \"kmers_after\": %llu, \"absent_after\": %llu, \"apply_ms\": %.3f, "
			       "\"screen_ms\": %.3f, \"count_ms\": %.3f}}\n",
			       (unsigned long long)qv_tot.kmers_before, (unsigned long long)qv_tot.absent_before, (unsigned long long)qv_tot.kmers_after,
			       (unsigned long long)qv_tot.absent_after, ms_apply, ms_qv_screen, ms_qv_count);
		}
		if (report) {
			double s = std::chrono::duration<double>(t1 - t0).count();
			printf("{\"bases\": %llu, \"seconds\": %.6f, \"open_outputs_s\": %.3f, \"index_s\": %.3f, \"read_s\": %.3f, \"polish_call_s\": %.3f, \"write_s\": %.3f, \"gpu_ms\": %.3f, \"screen_ms\": %.3f, \"machine_ms\": %.3f, "
			       "\"screening\": {\"batches_partitioned\": %u, \"batches_direct_kernel\": %u, \"record_chunks_rescreened_direct\": %u, \"overflow_records\": %llu}, \"events\": %llu, "
			       "\"events_applied\": %llu, \"absent_kmers\": %llu, \"substitutions\": %llu, \"insertions\": %llu, "
			       "\"deletions\": %llu}\n",
			       total_bases, s, s_before_index, s_index, s_read, s_call, s_write, ms_gpu, ms_screen, ms_machine, n_batches_binned, n_batches_direct, n_chunks_direct, (unsigned long long)n_ovf_records, (unsigned long long)tot.events,
			       (unsigned long long)tot.events_applied, (unsigned long long)tot.absent_kmers,
			       (unsigned long long)tot.substitutions, (unsigned long long)tot.insertions,
			       (unsigned long long)tot.deletions);
		}
		ntedit_hip_annot_free(annot);
		return prefix + "_edited.fa";
	};
	std::string round_draft = draft_given;
	for (size_t round = 0; round < n_rounds; round++) {
		// the last round writes under the prefix, an earlier one at Ki under <prefix>_k<Ki>
		const bool last_round = round + 1 == n_rounds;
		round_draft = polish_round(round, round_draft, last_round ? prefix_given : prefix_given + "_k" + std::to_string(rounds[round].k));
	}
	for (Work& w : pool) {
		w.b.release_raw();
	}
	ntedit_hip_destroy(ctx);
	return 0;
}
