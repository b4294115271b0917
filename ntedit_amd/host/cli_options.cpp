// cli_options.cpp -- the `ntedit` command line: its usage text, its option tables, the getopt loop and every refusal that
// happens before the device is opened and before any file is written.  Nothing here takes a live context.
//
// Keeps the reference's command-line surface (ntedit.cpp:135-169, 2276-2364):
//   -t -f -r -e -b -z -i -d -x -y -X -Y -c -j -m -s -l -a -v -p -q -k --help --version
// (-k is accepted and ignored: k comes from the Bloom filter header.  The reference lists -k in its
// option string but has no `case 'k'`, so `-k N` trips its "invalid option" check, ntedit.cpp:2360-2363;
// being lenient here keeps old command lines working.  -c is parsed and overwritten by k*1.5; -t sets the host
// threads that render the output, contigs themselves are polished on the GPU and
// the output order is the input order, i.e. the reference at -t 1).
#include "cli_options.h"
#include "cli_common.h"
#include "k_list.h"

#include <cerrno>
#include <cstring>
#include <getopt.h>
#include <sstream>

namespace nte_cli {

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

// (--help is pinned whole by the transcripts: an option added since has a paragraph of its own)
static const char HELP_BGZIP[] = PROGRAM
    " --bgzip\n\n"
    "	--bgzip,	write the edited draft as <prefix>_edited.fa.gz (BGZF, the blocked gzip that bgzip writes and that gzip, zcat,\n"
    "			samtools faidx and this program's -f read) in place of <prefix>_edited.fa.  The edited contigs are laid out\n"
    "			as FASTA text and compressed on the GPU, 65,280 bytes to a member, literal-only dynamic Huffman blocks (about\n"
    "			2.2 bits a base), stored blocks where that is not smaller; only the compressed bytes cross to the host.  The\n"
    "			decompressed text is byte for byte the _edited.fa of a run without the option; _changes.tsv and\n"
    "			_variants.vcf are unchanged.  The file ends in the 28-byte BGZF end-of-file member; a run in which no contig\n"
    "			passes -z writes that member alone.  With -k K1,K2,... an earlier round writes <prefix>_k<Ki>_edited.fa.gz and\n"
    "			the next round reads it.  One summary line reports plain bytes, BGZF bytes, their ratio, members and stored\n"
    "			members; --report adds {\"bgzip\": {...}}.  Not with --shard\n"
    "	--help-bgzip,	display this paragraph and exit\n\n";

static const char HELP_MIN_QUAL[] = PROGRAM
    " --reads --min_qual\n\n"
    "	--min_qual Q,	with --reads: the minimum base quality, 1 to 93.  A base whose Phred quality is below Q enters the reads\n"
    "			filter's build as N, so no k-mer that spans it is counted, and none is kept: a defence against sequencing\n"
    "			errors beside --cutoff / --solid, for low-coverage reads, ONT reads and the 3' tails of Illumina reads.\n"
    "			Phred+33: in FASTQ a quality character below 33 + Q, in BAM (--gpu_parse) a quality byte below Q; Phred+64\n"
    "			is not built.  Reads are kept by their length as before, masked bases included; records without qualities\n"
    "			(FASTA records, BAM records whose qualities are absent) pass as they are, and mixed inputs are legal.  The\n"
    "			host parser and --gpu_parse (plain, BGZF and BAM, where the copy and decode kernels mask in HBM) give the\n"
    "			same filter: the one ntedit-make-reads-bf --min_qual Q writes, and the one a build without the option\n"
    "			makes of the same reads with those bases rewritten to N.  With -k K1,K2,... every round masks alike (the\n"
    "			reads kept in HBM are the masked ones).  Each pass over the files reports `--min_qual Q: M of B bases with\n"
    "			a quality masked'; --report adds \"min_qual\" to each pass of the reads build.  Not with --genome or -r.\n"
    "			Not built: trimming instead of masking.  Which reads are kept at all: --help-read-filter\n"
    "	--help-min-qual,	display this paragraph and exit\n\n";

static const char HELP_READ_FILTER[] = PROGRAM
    " --reads --min_read_len --min_mean_qual --min_rq\n\n"
    "	Which reads go into the reads filter's build.  A record goes in when it passes every rule below; otherwise it is\n"
    "	absent, as a record shorter than k is without them.  The rules hold for every pass over the files and every round\n"
    "	of -k K1,K2,...: the reads kept in HBM are those that passed.\n"
    "	--min_read_len L,	L is 1 to 2147483647: the shortest record kept is the larger of L and what it is without\n"
    "	--min_rq R,	R is above 0 and at most 1.  A BAM record whose rq aux field of type f holds v is kept iff v >= R, as two\n"
    "			IEEE floats compare: a NaN is dropped.  A record without an rq:f field passes: every FASTA and FASTQ\n"
    "			record does.  The aux walk follows the SAM specification's types (A c C 1 byte, s S 2, i I f 4, Z H to a\n"
    "			NUL, B subtype + count * size) and never leaves the record; a field that does not fit, or of an unknown\n"
    "			type, ends it: the record counts as having no tag, and as malformed in the pass line\n"
    "	--min_mean_qual Q,	Q is 1 to 60.  A read's mean quality is the Phred value of its mean error probability (as NanoFilt,\n"
    "			chopper and fastplong take it), not the mean of the Phred values, computed in integers: a base of Phred\n"
    "			quality q adds E[min(q, 93)], E[q] = round(2^31 * 10^(-q/10)) (a FASTQ byte below 33 counts as q = 0), S\n"
    "			is the sum over the read, and the read is kept iff S <= len * E[Q].  Records without qualities pass: FASTA\n"
    "			records, and BAM records whose qualities are absent.  With --min_qual the mean is taken over the\n"
    "			qualities as stored, not over the masked text, and --min_qual's counts cover the reads that were copied\n"
    "	A dropped record is counted under the first rule that drops it, in the order flag (BAM), length, rq, mean quality.\n"
    "	Each pass over the files reports `read filter: D of N records dropped (length a, rq b, mean quality c)'; --report\n"
    "	adds \"read_filter\" to each pass of the reads build.  The host parser and --gpu_parse (plain, BGZF and BAM) give the\n"
    "	same filter: the one a build without the options makes of the same reads with the dropped ones deleted.  Not with\n"
    "	--genome or -r.  Not built: Phred+64, trimming, other BAM tags (np, ec), a maximum read length\n"
    "	--help-read-filter,	display this paragraph and exit\n\n";

static const char HELP_BED[] = PROGRAM
    " --qv --bed\n\n"
    "	--bed,		with --qv: where the k-mers that --qv counts as absent lie, as two BED tracks -- <prefix>_absent_before.bed in\n"
    "			the draft's names and coordinates, <prefix>_absent_after.bed in those of <prefix>_edited.fa.  A row is a\n"
    "			region the filter does not support: the k-mer spans [p, p + k) of a contig's absent k-mers, overlapping and\n"
    "			book-ended spans merged (as bedtools merge does), never across contigs.  Four columns, no header line: the\n"
    "			sequence name (the header line up to its first space or tab), begin, end (0-based, half open) and the number\n"
    "			of absent k-mers in the region; per contig that column sums to absent_before / absent_after of\n"
    "			<prefix>_qv.tsv.  A single wrong base shows as a region of 2k - 1 bases with k absent k-mers.  Rows are in\n"
    "			_edited.fa's order.  The regions are extracted on the GPU from the bitmaps --qv screens anyway; only the\n"
    "			intervals cross to the host.  With -k K1,K2,... an earlier round writes <prefix>_k<Ki>_absent_*.bed.  One\n"
    "			summary line reports intervals and covered bases before and after; --report adds {\"bed\": {...}}.  Not\n"
    "			with --shard\n"
    "	--help-bed,	display this paragraph and exit\n\n";

static const char HELP_SPECTRUM[] = PROGRAM
    " --spectrum\n\n"
    "	--spectrum,	with a counting filter (-r counts.bf, or --reads --counts): the k-mer multiplicity spectrum of the draft\n"
    "			before and after the polish.  A k-mer's multiplicity is the smallest of its h counters -- what -p and -q\n"
    "			compare --, 0..255, 255 meaning 255 or more.  Writes <prefix>_spectrum.tsv (multiplicity, before, after:\n"
    "			always 256 rows, every k-mer occurrence of the draft counted at its multiplicity) and <prefix>_depth.tsv\n"
    "			(name, kmers_before, mean_before, saturated_before, kmers_after, mean_after, saturated_after: one row per\n"
    "			contig in <prefix>_edited.fa's order, then #total; mean is NA without k-mers and a lower bound where\n"
    "			counters saturate).  A contig at half or double the peak is a haplotig or a collapsed repeat, one at 0 is\n"
    "			not in the reads.  The counters over-estimate (a count-min minimum), and a filter built with -c C holds\n"
    "			nothing below C: multiplicities 1..C-1 show as 0.  Both spectra are counted on the GPU from the batch and\n"
    "			the edited contigs in HBM; -p, -q, -s and -e play no part.  With or without --qv.  With -k K1,K2,... an\n"
    "			earlier round writes <prefix>_k<Ki>_spectrum.tsv and _depth.tsv.  One summary line reports k-mers, the\n"
    "			share at 0, the mean, the peak and the saturated share before and after; --report adds\n"
    "			{\"spectrum\": {...}}.  Not with a plain filter, --genome, --reads without --counts, or --shard\n"
    "	--help-spectrum,	display this paragraph and exit\n\n";

static const char HELP_CN[] = PROGRAM
    " --spectrum --cn\n\n"
    "	--cn,		with --spectrum: the spectrum split by how many times the ASSEMBLY holds each k-mer (Merqury's spectra-cn).\n"
    "			A k-mer's copy number is counted over the whole draft, so the draft and the edited contigs stay in HBM\n"
    "			until the round ends; then a count-min sketch of 8-bit counters (the filter's h hashes) is counted over\n"
    "			each side and read back per k-mer together with the filter.  Writes <prefix>_spectrum_cn.tsv\n"
    "			(multiplicity, before_cn1 .. before_cn4, before_cn5plus, after_cn1 .. after_cn5plus: always 256 rows, in\n"
    "			DISTINCT k-mers) and <prefix>_cn_contigs.tsv (name, then kmers and the five class counts of k-mer\n"
    "			occurrences before and after: one row per contig in <prefix>_edited.fa's order, then #total).  A half-depth\n"
    "			peak of copy-number-2 k-mers means retained haplotigs, a double-depth peak of copy-number-1 k-mers a\n"
    "			collapsed repeat, a contig made mostly of copy-number-2 k-mers a duplicate.  Copy numbers are count-min\n"
    "			estimates, never below the truth; the summary line prints the expected inflated share, (non-zero\n"
    "			counters / counters)^h.  A filter with one hash (h = 1) gives a poor sketch.  There is no read-only row: a\n"
    "			filter cannot be enumerated (--completeness gives that total for plain filters).  With -k K1,K2,... an\n"
    "			earlier round writes <prefix>_k<Ki>_spectrum_cn.tsv and _cn_contigs.tsv.  --report adds {\"cn\": {...}}.\n"
    "			Not without --spectrum, and with nothing --spectrum refuses\n"
    "	--cn_store BYTES,	the most bases of both sides the store may hold [34359738368].  A draft that passes it releases\n"
    "			the store: the polish and every other output finish as usual, no cn file is written, one line on\n"
    "			standard error says so, the exit status is 0\n"
    "	--cn_sketch COUNTERS,	the sketch's size, a power of two from 2^20 to 2^36 [the smallest at or above 8 times the\n"
    "			stored bytes of the larger side]\n"
    "	--help-cn,	display this paragraph and exit\n\n";

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
	OPT_GPU_PARSE,
	OPT_BGZIP,
	OPT_HELP_BGZIP,
	OPT_BED,
	OPT_HELP_BED,
	OPT_SPECTRUM,
	OPT_HELP_SPECTRUM,
	OPT_CN,
	OPT_CN_STORE,
	OPT_CN_SKETCH,
	OPT_HELP_CN,
	OPT_MIN_QUAL,
	OPT_HELP_MIN_QUAL,
	OPT_MIN_READ_LEN,
	OPT_MIN_MEAN_QUAL,
	OPT_MIN_RQ,
	OPT_HELP_READ_FILTER
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
	{ "bgzip", no_argument, nullptr, OPT_BGZIP },
	{ "help-bgzip", no_argument, nullptr, OPT_HELP_BGZIP },
	{ "bed", no_argument, nullptr, OPT_BED },
	{ "help-bed", no_argument, nullptr, OPT_HELP_BED },
	{ "spectrum", no_argument, nullptr, OPT_SPECTRUM },
	{ "help-spectrum", no_argument, nullptr, OPT_HELP_SPECTRUM },
	{ "cn", no_argument, nullptr, OPT_CN },
	{ "cn_store", required_argument, nullptr, OPT_CN_STORE },
	{ "cn_sketch", required_argument, nullptr, OPT_CN_SKETCH },
	{ "help-cn", no_argument, nullptr, OPT_HELP_CN },
	{ "min_qual", required_argument, nullptr, OPT_MIN_QUAL },
	{ "help-min-qual", no_argument, nullptr, OPT_HELP_MIN_QUAL },
	{ "min_read_len", required_argument, nullptr, OPT_MIN_READ_LEN },
	{ "min_mean_qual", required_argument, nullptr, OPT_MIN_MEAN_QUAL },
	{ "min_rq", required_argument, nullptr, OPT_MIN_RQ },
	{ "help-read-filter", no_argument, nullptr, OPT_HELP_READ_FILTER },
	{ "help", no_argument, nullptr, OPT_HELP },
	{ "version", no_argument, nullptr, OPT_VERSION },
	{ nullptr, 0, nullptr, 0 }
};

// The options of the reads filter, each named once: `with_genome` says that --genome shares it (genome_rules and the "only
// with --reads [or --genome]" message read that), `text` is where an option with a value leaves it for the library's rules
// (reads_options.cpp), which refuse at the option what they refuse there.
struct ReadsOption
{
	int opt;
	const char* name;
	bool with_genome;
	const char* ntedit_hip_reads_options::* text;
	const char* ntedit_hip_reads_filter_options::* filter_text = nullptr; // (the read filter's options have a struct of their own)
};
static const ReadsOption READS_OPTIONS[] = {
	{ OPT_CUTOFF, "--cutoff", false, &ntedit_hip_reads_options::cutoff },
	{ OPT_SOLID, "--solid", false, nullptr },
	{ OPT_COUNTS, "--counts", false, nullptr },
	{ OPT_HASHES, "--hashes", true, &ntedit_hip_reads_options::hashes },
	{ OPT_FPR, "--fpr", true, &ntedit_hip_reads_options::fpr },
	{ OPT_BF, "--bf", true, &ntedit_hip_reads_options::bf },
	{ OPT_NUM_ELEMENTS, "--num_elements", true, &ntedit_hip_reads_options::num_elements },
	{ OPT_SKETCH_BYTES, "--sketch_bytes", false, &ntedit_hip_reads_options::sketch_bytes },
	{ OPT_HIST, "--hist", false, nullptr },
	{ OPT_SAVE_BF, "--save_bf", true, nullptr },
	{ OPT_REJECT_CUTOFF, "--reject_cutoff", false, &ntedit_hip_reads_options::reject_cutoff },
	{ OPT_REJECT_BF, "--reject_bf", false, &ntedit_hip_reads_options::reject_bf },
	{ OPT_REJECT_NUM_ELEMENTS, "--reject_num_elements", false, &ntedit_hip_reads_options::reject_num_elements },
	{ OPT_SAVE_REJECT_BF, "--save_reject_bf", false, nullptr },
	{ OPT_READS_BATCH, "--batch_bytes", true, &ntedit_hip_reads_options::batch_bytes },
	{ OPT_STORE_CAP, "--resident_cap", false, &ntedit_hip_reads_options::store_cap },
	{ OPT_GPU_PARSE, "--gpu_parse", true, nullptr },
	{ OPT_MIN_QUAL, "--min_qual", false, &ntedit_hip_reads_options::min_qual },
	{ OPT_MIN_READ_LEN, "--min_read_len", false, nullptr, &ntedit_hip_reads_filter_options::min_read_len },
	{ OPT_MIN_MEAN_QUAL, "--min_mean_qual", false, nullptr, &ntedit_hip_reads_filter_options::min_mean_qual },
	{ OPT_MIN_RQ, "--min_rq", false, nullptr, &ntedit_hip_reads_filter_options::min_rq },
};

static void
die_unreadable(const std::string& path)
{
	// ntedit.cpp:476-483
	if (access(path.c_str(), R_OK) == -1) {
		fail("`%s': %s", path.c_str(), strerror(errno));
	}
}

template<typename T>
static void
parse(int c, const char* arg, T& out)
{
	std::istringstream ss(arg ? arg : "");
	ss >> out;
	if (arg && (!ss.eof() || ss.fail())) {
		fail_plain("invalid option: `-%c%s'", (char)c, arg); // ntedit.cpp:2360-2363
	}
}

static void
refuse(const std::string& why)
{
	fail("%s\nTry `" PROGRAM " --help' for more information.", why.c_str());
}

// the reads options through the library's rules (reads_options.cpp); a refusal ends the run, in the words and the form it
// always had: a malformed number as getopt's invalid options are
static ntedit_hip_reads_rules
reads_rules(const ntedit_hip_reads_options& ro, int final)
{
	ntedit_hip_reads_rules rr;
	const int rc = ntedit_hip_reads_options_check(&ro, NTEDIT_READS_DIALECT_POLISHER, final, &rr);
	if (rc == NTEDIT_READS_NOT_A_NUMBER) {
		fail_plain("%s", ntedit_hip_reads_last_error(nullptr));
	}
	if (rc != 0) {
		refuse(ntedit_hip_reads_last_error(nullptr));
	}
	return rr;
}

// ... and the read filter's options through theirs, behind them
static ntedit_hip_reads_filter_rules
filter_rules(const ntedit_hip_reads_filter_options& fo, int final)
{
	ntedit_hip_reads_filter_rules fr;
	const int rc = ntedit_hip_reads_filter_options_check(&fo, NTEDIT_READS_DIALECT_POLISHER, final, &fr);
	if (rc == NTEDIT_READS_NOT_A_NUMBER) {
		fail_plain("%s", ntedit_hip_reads_last_error(nullptr));
	}
	if (rc != 0) {
		refuse(ntedit_hip_reads_last_error(nullptr));
	}
	return fr;
}

// The rules of ntedit --genome, apart from the reads options' (reads_options.cpp knows nothing of them).  The numbers arrive
// well-formed (reads_rules refuses a malformed one at its option); -k is checked here.  Returns the refusal, or "" and the
// settings.
static std::string
genome_rules(const CliOptions& o, const std::vector<const ReadsOption*>& given, GenomeRules* g)
{
	const ntedit_hip_reads_options& ro = o.ro;
	if (!o.bf.empty()) {
		return "--genome and -r: give one of them (--genome builds the filter that -r would load)";
	}
	if (o.reads_mode) {
		return "--genome and --reads: give one of them (each builds the filter that -r would load)";
	}
	if (o.shard_given) {
		return "--genome and --shard: every shard would build the whole filter again; build it once with "
		       "ntedit-make-genome-bf and give each shard -r";
	}
	if (o.genome_files.empty()) {
		return "--genome: 1 or more files expected";
	}
	for (const ReadsOption* r : given) {
		if (!r->with_genome) {
			return std::string(r->name) + ": only with --reads (--genome builds the plain filter of every k-mer of the assemblies)";
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

// --reads FILE... and --genome FILE...: the files up to the next option, taken out of argv (getopt takes one argument per
// option); returns what is left for getopt
static std::vector<char*>
take_file_lists(int argc, char** argv, CliOptions* o)
{
	std::vector<char*> args;
	for (int i = 0; i < argc; i++) {
		const bool reads = i > 0 && strcmp(argv[i], "--reads") == 0, genome = i > 0 && strcmp(argv[i], "--genome") == 0;
		if (!reads && !genome) {
			args.push_back(argv[i]);
			continue;
		}
		(reads ? o->reads_mode : o->genome_mode) = true;
		while (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] != 0)) {
			(reads ? o->read_files : o->genome_files).push_back(argv[++i]);
		}
	}
	args.push_back(nullptr);
	return args;
}

// --tune KEY=VALUE (the value through the option parser: trailing garbage is an error, not a silent 0)
static void
parse_tune(const char* arg, CliOptions* o)
{
	const char* eq = strchr(arg, '=');
	unsigned long long tv = 0;
	std::istringstream ss(eq ? eq + 1 : "");
	ss >> tv;
	if (!eq || eq == arg || !ss.eof() || ss.fail() || eq[1] == '-') {
		fail_plain("invalid option: `--tune %s'", arg);
	}
	o->tunes.emplace_back(std::string(arg, eq - arg), tv);
}

// the getopt loop; returns whether getopt met an option it does not know.  `given`: the reads options, in the order given
static bool
parse_options(int argc, char** argv, CliOptions* o, std::vector<const ReadsOption*>* given)
{
	bool die = false;
	unsigned ignored_u = 0;
	ntedit_hip_params& p = o->params;
	for (int c; (c = getopt_long(argc, argv, shortopts, longopts, nullptr)) != -1;) {
		for (const ReadsOption& r : READS_OPTIONS) {
			if (r.opt == c) {
				given->push_back(&r);
				if (r.text) {
					o->ro.*r.text = optarg;
					reads_rules(o->ro, 0);
				}
				if (r.filter_text) {
					o->fo.*r.filter_text = optarg;
					filter_rules(o->fo, 0);
				}
			}
		}
		switch (c) {
		case '?':
			die = true;
			break;
		case 't':
			parse(c, optarg, o->nthreads);
			o->threads_given = true;
			break;
		case 'f':
			parse(c, optarg, o->draft);
			break;
		case 'z':
			parse(c, optarg, p.min_contig_len);
			break;
		case 'b':
			parse(c, optarg, o->prefix);
			break;
		case 'r':
			parse(c, optarg, o->bf);
			break;
		case 'e':
			parse(c, optarg, o->bfrep);
			break;
		case 'd':
			parse(c, optarg, p.max_deletions);
			break;
		case 'i':
			parse(c, optarg, p.max_insertions);
			break;
		case 'x':
			parse(c, optarg, p.missing_threshold);
			break;
		case 'y':
			parse(c, optarg, p.edit_threshold);
			break;
		case 'X':
			parse(c, optarg, p.missing_ratio);
			p.use_ratio = 1;
			break;
		case 'Y':
			parse(c, optarg, p.edit_ratio);
			p.use_ratio = 1;
			break;
		case 'c':
			parse(c, optarg, ignored_u); // overwritten by k*1.5 (ntedit.cpp:2450)
			break;
		case 'j':
			parse(c, optarg, p.jump);
			break;
		case 'm':
			parse(c, optarg, p.mode);
			break;
		case 's':
			parse(c, optarg, p.snv);
			break;
		case 'l':
			parse(c, optarg, o->vcf);
			break;
		case 'a':
			parse(c, optarg, p.mask);
			break;
		case 'v':
			parse(c, optarg, o->verbose);
			break;
		case 'p':
			parse(c, optarg, p.min_threshold);
			break;
		case 'q':
			parse(c, optarg, p.max_threshold);
			break;
		case 'k':
			// without --reads: accepted and ignored (the reference rejects it: no `case 'k'`, ntedit.cpp:2360-2363)
			o->ro.k = optarg;
			break;
		case OPT_SOLID:
			o->ro.solid = 1;
			break;
		case OPT_COUNTS:
			o->counts = true;
			break;
		case OPT_HIST:
			o->hist = optarg;
			o->ro.hist = 1;
			break;
		case OPT_SAVE_BF:
			o->save_bf = optarg;
			break;
		case OPT_SAVE_REJECT_BF:
			o->save_reject_bf = optarg;
			o->ro.reject_out = 1;
			break;
		case OPT_GPU_PARSE:
			o->ro.gpu_parse = 1;
			break;
		case OPT_GPU:
			parse(c, optarg, o->gpu);
			break;
		case OPT_BATCH:
			parse(c, optarg, o->batch_bases);
			o->batch_given = true;
			break;
		case OPT_START_GRID:
			parse(c, optarg, p.start_grid);
			break;
		case OPT_EVENT_BUDGET:
			parse(c, optarg, p.event_budget);
			break;
		case OPT_SHARD:
			if (sscanf(optarg, "%u/%u", &o->shard_i, &o->shard_n) != 2 || o->shard_n == 0 || o->shard_i >= o->shard_n) {
				fail_plain("invalid option: `--shard %s'", optarg);
			}
			o->shard_given = true;
			break;
		case OPT_REPORT:
			o->report = 1;
			break;
		case OPT_QV:
			o->qv = true;
			break;
		case OPT_COMPLETENESS:
			o->completeness = true;
			break;
		case OPT_NO_MAP:
			o->no_map = true;
			break;
		case OPT_PACK:
			o->no_pack = false;
			break;
		case OPT_TUNE:
			parse_tune(optarg, o);
			break;
		case OPT_BGZIP:
			o->bgzip = true;
			break;
		case OPT_HELP_BGZIP:
			fputs(HELP_BGZIP, stderr);
			exit(EXIT_SUCCESS);
		case OPT_BED:
			o->bed = true;
			break;
		case OPT_HELP_BED:
			fputs(HELP_BED, stderr);
			exit(EXIT_SUCCESS);
		case OPT_SPECTRUM:
			o->spectrum = true;
			break;
		case OPT_HELP_SPECTRUM:
			fputs(HELP_SPECTRUM, stderr);
			exit(EXIT_SUCCESS);
		case OPT_CN:
			o->cn = true;
			break;
		case OPT_CN_STORE:
			o->cn_store_text = optarg;
			break;
		case OPT_CN_SKETCH:
			o->cn_sketch_text = optarg;
			break;
		case OPT_HELP_CN:
			fputs(HELP_CN, stderr);
			exit(EXIT_SUCCESS);
		case OPT_HELP_MIN_QUAL:
			fputs(HELP_MIN_QUAL, stderr);
			exit(EXIT_SUCCESS);
		case OPT_HELP_READ_FILTER:
			fputs(HELP_READ_FILTER, stderr);
			exit(EXIT_SUCCESS);
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
	return die;
}

// every refusal of --reads, and the rules of each round
static void
reads_mode_rules(CliOptions* o, const std::vector<std::string>& k_list)
{
	if (!o->bf.empty()) {
		refuse("--reads and -r: give one of them (--reads builds the filter that -r would load)");
	}
	if (o->read_files.empty()) {
		refuse("--reads: 1 or more files expected");
	}
	if (o->shard_given) {
		refuse("--reads and --shard: every shard would build the whole filter again; build it once with "
		       "ntedit-make-reads-bf and give each shard -r");
	}
	if (o->ro.reject_cutoff && !o->bfrep.empty()) {
		refuse("--reject_cutoff and -e: give one of them (--reject_cutoff builds the filter that -e would load)");
	}
	for (const std::string& r : o->read_files) {
		o->paths.push_back(r.c_str());
	}
	o->ro.counts = o->counts;
	o->ro.files = o->paths.data(); // (for the default sketch: their sizes)
	o->ro.n_files = (uint32_t)o->paths.size();
	if (k_list.empty()) {
		o->rounds[0] = reads_rules(o->ro, 1);
	} else {
		// (every option but -k applies to every round alike; sizes taken from the histogram are found per round)
		o->rounds.clear();
		for (const std::string& kt : k_list) {
			ntedit_hip_reads_options one = o->ro;
			one.k = kt.c_str();
			o->rounds.push_back(reads_rules(one, 1));
		}
	}
	o->filter_rules = filter_rules(o->fo, 1);
	for (const std::string& r : o->read_files) {
		die_unreadable(r);
	}
}

CliOptions
parse_cli(int argc, char** argv)
{
	CliOptions o;
	ntedit_hip_params_default(&o.params);
	std::vector<char*> args = take_file_lists(argc, argv, &o);
	std::vector<const ReadsOption*> given; // reads options given (refused without --reads)
	bool die = parse_options((int)args.size() - 1, args.data(), &o, &given);
	printf("---------- initializing                             : %s", now_text());
	if (o.draft.empty()) {
		fprintf(stderr, PROGRAM ": error: need to specify assembly draft file (-f)\n");
		die = true;
	} else {
		die_unreadable(o.draft);
	}
	if (o.completeness && (!o.qv || o.shard_given || o.counts)) {
		fail("--completeness%s",
		     !o.qv           ? ": only with --qv (it marks the k-mers the QV screenings find present)"
		     : o.shard_given ? " and --shard: the marks of the shards would need a merge of their own; run it on the whole draft"
		                     : " and --counts: completeness takes a plain filter; a counting filter's slots are counters");
	}
	if (o.qv && o.shard_given) {
		fail("--qv and --shard: a table per shard would need a merge of its own; run --qv on the whole draft");
	}
	if (o.spectrum && (o.shard_given || o.genome_mode || (o.reads_mode && !o.counts))) {
		// (behind the older refusals above; before the device is opened and before a file is written)
		fail("--spectrum%s",
		     o.shard_given   ? " and --shard: the spectra of the shards would need a merge of their own; run --spectrum on the whole draft"
		     : o.genome_mode ? " and --genome: the spectrum takes a counting filter; a genome filter is plain"
		                     : " and --reads without --counts: the spectrum takes a counting filter; add --counts");
	}
	// --cn and its two settings: behind everything --spectrum refuses
	if (o.cn && !o.spectrum) {
		fail("--cn: only with --spectrum (the copy numbers split the spectrum)");
	}
	if ((o.cn_store_text || o.cn_sketch_text) && !o.cn) {
		fail("%s: only with --cn", o.cn_store_text ? "--cn_store" : "--cn_sketch");
	}
	if (o.cn_store_text) {
		char* end = nullptr;
		o.cn_store = strtoull(o.cn_store_text, &end, 10);
		if (!*o.cn_store_text || *end || o.cn_store_text[0] == '-') {
			fail("--cn_store %s: a number of bytes", o.cn_store_text);
		}
	}
	if (o.cn_sketch_text) {
		char* end = nullptr;
		o.cn_sketch = strtoull(o.cn_sketch_text, &end, 10);
		if (!*o.cn_sketch_text || *end || o.cn_sketch_text[0] == '-' || (o.cn_sketch & (o.cn_sketch - 1)) || o.cn_sketch < NTEDIT_CN_SKETCH_MIN ||
		    o.cn_sketch > NTEDIT_CN_SKETCH_MAX) {
			fail("--cn_sketch %s: the sketch takes a power of two from 2^20 (1048576) to 2^36 counters", o.cn_sketch_text);
		}
	}
	std::vector<std::string> k_list; // -k K1,K2,...: its k as given, in order
	if (o.ro.k && strchr(o.ro.k, ',')) {
		const std::string why = nte_host::k_list_rules(
		    o.ro.k, o.reads_mode, o.shard_given, !o.prefix.empty(),
		    { { "--save_bf", o.save_bf }, { "--save_reject_bf", o.save_reject_bf }, { "--hist", o.hist } }, &k_list);
		if (!why.empty()) {
			refuse(why);
		}
	}
	if (o.genome_mode) {
		const std::string why = genome_rules(o, given, &o.genome);
		if (!why.empty()) {
			refuse(why);
		}
		for (const std::string& g : o.genome_files) {
			die_unreadable(g);
			o.paths.push_back(g.c_str());
		}
	} else if (o.reads_mode) {
		reads_mode_rules(&o, k_list);
	} else if (!given.empty()) {
		// (the options --genome shares with --reads say so)
		refuse(std::string(given[0]->name) + (given[0]->with_genome ? ": only with --reads or --genome" : ": only with --reads"));
	} else if (o.bf.empty()) {
		fprintf(stderr, PROGRAM ": error: need to specify the Bloom filter file (-r)\n");
		die = true;
	} else {
		die_unreadable(o.bf);
	}
	if (!o.bfrep.empty()) {
		die_unreadable(o.bfrep);
	}
	if (die) {
		fprintf(stderr, "Try `" PROGRAM " --help' for more information.\n");
		exit(EXIT_FAILURE);
	}
	if (o.bgzip && o.shard_given) {
		// (behind every older refusal)
		fail("--bgzip and --shard: the byte index of the shards and the gather that merges them know plain text only; run --bgzip on the whole draft");
	}
	if (o.bed && !o.qv) {
		// (--bed with --shard: --qv's refusal above has answered)
		fail("--bed: only with --qv (the tracks are made of the bitmaps the QV screenings leave)");
	}
	if (o.params.snv) {
		// ntedit.cpp:2411-2417
		fprintf(stderr, "\nSNV mode ON\nTracking all single-base variants\nNote: -i and -d both set to 0 when -s is set to 1\n"
		                "Consider -l clinvar.vcf to identify SNVs with putative clinical significance\n\n");
	}
	return o;
}

} // namespace nte_cli
