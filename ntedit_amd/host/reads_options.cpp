// reads_options.cpp -- the rules of the reads options, once for the four front ends that take them: ntedit-make-reads-bf
// and python -m ntedit_amd.make_reads (the TOOL dialect: -c, sentences that end in a period), ntedit --reads and
// python -m ntedit_amd.run --reads (the POLISHER dialect: --cutoff, "with --reads").  Host only.  A front end keeps how it
// walks its arguments and what only it has; what is refused, in which order and in which words is here.
#include "../csrc/nte_reads_internal.h"

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {

// a whole non-negative decimal number, or false
bool
parse_u64(const char* s, uint64_t* out)
{
	if (!*s || *s == '-' || *s == '+') {
		return false;
	}
	char* end = nullptr;
	errno = 0;
	const unsigned long long v = strtoull(s, &end, 10);
	if (errno || *end) {
		return false;
	}
	*out = v;
	return true;
}

} // namespace

extern "C" int
ntedit_hip_reads_options_check(const ntedit_hip_reads_options* o, int dialect, int final, ntedit_hip_reads_rules* r)
{
	if (!o || !r || (o->n_files && !o->files) ||
	    (dialect != NTEDIT_READS_DIALECT_TOOL && dialect != NTEDIT_READS_DIALECT_POLISHER)) {
		return nte_reads::set_error(nullptr, NTEDIT_E_ARG, "reads_options_check: bad argument");
	}
	const bool tool = dialect == NTEDIT_READS_DIALECT_TOOL;
	const std::string cut = tool ? "-c" : "--cutoff", dot = tool ? "." : "", with_reads = tool ? "." : " with --reads";
	auto refuse = [](int code, const std::string& why) { return nte_reads::set_error(nullptr, code, why); };
	// an option's number; true: malformed, and refused in the dialect's words
	auto malformed = [&](const std::string& name, const char* text, uint64_t* out) {
		if (!text || parse_u64(text, out)) {
			return false;
		}
		refuse(0, tool ? name + ": not a number: '" + text + "'" : "invalid option: `" + name + " " + text + "'");
		return true;
	};
	*r = ntedit_hip_reads_rules();
	r->hash_num = 3;
	r->fpr = 0.01;
	r->batch_bytes = NTEDIT_READS_BATCH_DEFAULT;
	r->store_cap = NTEDIT_READS_RESIDENT_CAP_DEFAULT;
	r->threads = 12;
	r->gpu_parse = o->gpu_parse ? 1 : 0; // (the one rule about it, "only with --reads", is the polisher front ends': they know)
	uint64_t k = 0, cmin = 0, hashes = r->hash_num, reject = 0, min_qual = 0;
	// -k: the tool refuses a malformed one at the option, the polisher takes it as out of range
	if (final && !o->k) {
		return refuse(NTEDIT_READS_REFUSED, "-k: required" + with_reads);
	}
	if (o->k) {
		if (tool && malformed("-k", o->k, &k)) {
			return NTEDIT_READS_NOT_A_NUMBER;
		}
		if (final && (!parse_u64(o->k, &k) || k < 12 || k > 200)) {
			return refuse(NTEDIT_READS_REFUSED, "-k " + (tool ? std::to_string(k) : std::string(o->k)) + ": k must be between 12 and 200" + dot);
		}
	}
	// what is refused at the option itself
	if (malformed(cut, o->cutoff, &cmin) || malformed("--hashes", o->hashes, &hashes)) {
		return NTEDIT_READS_NOT_A_NUMBER;
	}
	if (o->fpr) {
		char* end = nullptr;
		r->fpr = strtod(o->fpr, &end);
		if (!*o->fpr || *end || !(r->fpr > 0.0 && r->fpr < 1.0)) {
			return refuse(NTEDIT_READS_REFUSED, tool ? std::string("--fpr: needs a number between 0 and 1: '") + o->fpr + "'"
			                                         : std::string("--fpr ") + o->fpr + ": needs a number between 0 and 1");
		}
	}
	if (malformed("--bf", o->bf, &r->bf_bytes) || malformed("--num_elements", o->num_elements, &r->num_elements) ||
	    malformed("--sketch_bytes", o->sketch_bytes, &r->sketch_bytes) || malformed("--batch_bytes", o->batch_bytes, &r->batch_bytes) ||
	    malformed("--resident_cap", o->store_cap, &r->store_cap) || malformed("-t", o->threads, &r->threads) ||
	    malformed("--reject_cutoff", o->reject_cutoff, &reject) || malformed("--reject_bf", o->reject_bf, &r->reject_bf_bytes) ||
	    malformed("--reject_num_elements", o->reject_num_elements, &r->reject_num_elements) || malformed("--min_qual", o->min_qual, &min_qual)) {
		return NTEDIT_READS_NOT_A_NUMBER;
	}
	if (!final) {
		return 0;
	}
	// a BAM has no host parser (kseq would read whatever '@' and '>' bytes the binary stream holds): one line, the same in
	// both dialects
	for (uint32_t i = 0; !o->gpu_parse && i < o->n_files; i++) {
		if (o->files[i] && ntedit_hip_reads_is_bam(o->files[i])) {
			return refuse(NTEDIT_READS_REFUSED, std::string("--reads ") + o->files[i] + ": BAM needs --gpu_parse");
		}
	}
	// the rules between the options
	if (o->cutoff && o->solid) {
		return refuse(NTEDIT_READS_REFUSED, (tool ? "--solid and -c" : "--cutoff and --solid") +
		                                        std::string(": give one of them (--solid takes the minimum count from the k-mer histogram)") + dot);
	}
	if (!o->cutoff && !o->solid) {
		return refuse(NTEDIT_READS_REFUSED, tool ? "-c: required (or --solid)." : "--cutoff or --solid: one of them is required with --reads");
	}
	if (o->cutoff && (cmin < 1 || cmin > 255)) {
		return refuse(NTEDIT_READS_REFUSED, cut + " " + std::to_string(cmin) + ": the minimum count must be between 1 and 255" + dot);
	}
	if (hashes < 1 || hashes > 8) {
		return refuse(NTEDIT_READS_REFUSED, "--hashes " + std::to_string(hashes) + ": the number of hash functions must be between 1 and 8" + dot);
	}
	r->k = (uint32_t)k;
	r->cmin = (uint32_t)cmin;
	r->hash_num = (uint32_t)hashes;
	r->gather_hist = o->solid || o->hist;
	r->size_from_hist = !o->bf && !o->num_elements;
	if (r->size_from_hist && !r->gather_hist) {
		return refuse(NTEDIT_READS_REFUSED, "--bf or --num_elements: one of them is required (or --solid / --hist, which size the filter "
		                                    "from the k-mer histogram)" + dot);
	}
	if (!o->bf && o->num_elements) {
		r->bf_bytes = ntedit_hip_reads_bf_size(r->num_elements, r->hash_num, r->fpr);
	}
	const bool empty = !r->size_from_hist && r->bf_bytes == 0;
	if (empty && !tool) {
		return refuse(NTEDIT_READS_REFUSED, "--bf / --num_elements: the filter would be empty");
	}
	if (r->batch_bytes < 4096) {
		return refuse(NTEDIT_READS_REFUSED, "--batch_bytes: at least 4096" + dot);
	}
	// the reject filter (ntedit -e), built by the same pass 2
	if (!o->reject_cutoff) {
		const char* alone = o->reject_bf ? "--reject_bf" : o->reject_num_elements ? "--reject_num_elements" : nullptr;
		if (alone || o->reject_out) {
			return refuse(NTEDIT_READS_REFUSED, std::string(alone ? alone : tool ? "--reject_out" : "--save_reject_bf") +
			                                        ": only with --reject_cutoff" + dot);
		}
	} else {
		if (reject < 2 || reject > 255) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_cutoff " + std::to_string(reject) + ": the reject count must be between 2 and 255" + dot);
		}
		if (o->counts) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_cutoff and --counts: a counting filter needs no reject filter (ntedit -q "
			                                    "sets the maximum count)" + dot);
		}
		if (o->cutoff && reject <= cmin) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_cutoff " + std::to_string(reject) + ": the reject count must be above " + cut + " " +
			                                        std::to_string(cmin) + dot);
		}
		if (o->reject_bf && o->reject_num_elements) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_bf and --reject_num_elements: give one of them" + dot);
		}
		r->reject_cmin = (uint32_t)reject;
		r->reject_size_from_hist = !o->reject_bf && !o->reject_num_elements;
		if (r->reject_size_from_hist && !r->gather_hist) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_bf or --reject_num_elements: one of them is required with --reject_cutoff (or "
			                                    "--solid / --hist, which size the reject filter from the k-mer histogram)" + dot);
		}
		if (o->reject_num_elements) {
			r->reject_bf_bytes = ntedit_hip_reads_bf_size(r->reject_num_elements, r->hash_num, r->fpr);
		}
		if (!r->reject_size_from_hist && r->reject_bf_bytes == 0) {
			return refuse(NTEDIT_READS_REFUSED, "--reject_bf / --reject_num_elements: the reject filter would be empty" + dot);
		}
	}
	// --min_qual: a Phred quality, Phred+33 in FASTQ (a quality byte from '!' to '~')
	if (o->min_qual && (min_qual < 1 || min_qual > 93)) {
		return refuse(NTEDIT_READS_REFUSED, "--min_qual " + std::to_string(min_qual) + ": the minimum base quality must be between 1 and 93" + dot);
	}
	r->min_qual = (uint32_t)min_qual;
	if (empty) { // (the tool has printed its parameters by then)
		return refuse(NTEDIT_READS_EMPTY, "The output filter would be empty (--bf 0 or --num_elements too small).");
	}
	r->sketch_counters = r->sketch_bytes ? r->sketch_bytes : ntedit_hip_reads_default_sketch(o->files, o->n_files, r->bf_bytes);
	return 0;
}

// --min_read_len, --min_rq, --min_mean_qual: which reads go into the build (ntedit_hip_reads_set_read_filter)
extern "C" int
ntedit_hip_reads_filter_options_check(const ntedit_hip_reads_filter_options* o, int dialect, int final, ntedit_hip_reads_filter_rules* r)
{
	if (!o || !r || (dialect != NTEDIT_READS_DIALECT_TOOL && dialect != NTEDIT_READS_DIALECT_POLISHER)) {
		return nte_reads::set_error(nullptr, NTEDIT_E_ARG, "reads_filter_options_check: bad argument");
	}
	const bool tool = dialect == NTEDIT_READS_DIALECT_TOOL;
	const std::string dot = tool ? "." : "";
	auto refuse = [](int code, const std::string& why) { return nte_reads::set_error(nullptr, code, why); };
	auto not_a_number = [&](const std::string& name, const char* text) {
		refuse(0, tool ? name + ": not a number: '" + text + "'" : "invalid option: `" + name + " " + text + "'");
		return NTEDIT_READS_NOT_A_NUMBER;
	};
	*r = ntedit_hip_reads_filter_rules();
	uint64_t min_read_len = 0, min_mean_qual = 0;
	float min_rq = 0.0f;
	if (o->min_read_len && !parse_u64(o->min_read_len, &min_read_len)) {
		return not_a_number("--min_read_len", o->min_read_len);
	}
	if (o->min_mean_qual && !parse_u64(o->min_mean_qual, &min_mean_qual)) {
		return not_a_number("--min_mean_qual", o->min_mean_qual);
	}
	if (o->min_rq) { // a decimal, read with strtof: digits, at most a point and an exponent (strtof alone would take leading blanks, a sign, hex floats, "inf" and "nan")
		char* end = nullptr;
		min_rq = strtof(o->min_rq, &end);
		const char c0 = o->min_rq[0];
		const bool decimal = ((c0 >= '0' && c0 <= '9') || c0 == '.') && strspn(o->min_rq, "0123456789.eE+-") == strlen(o->min_rq);
		if (!decimal || *end || end == o->min_rq) {
			return not_a_number("--min_rq", o->min_rq);
		}
	}
	if (!final) {
		return 0;
	}
	if (o->min_read_len && (min_read_len < 1 || min_read_len > 2147483647ull)) {
		return refuse(NTEDIT_READS_REFUSED, "--min_read_len " + std::string(o->min_read_len) + ": the minimum read length must be between 1 and 2147483647" + dot);
	}
	if (o->min_rq && !(min_rq > 0.0f && min_rq <= 1.0f)) { // (written so that a NaN is refused)
		return refuse(NTEDIT_READS_REFUSED, "--min_rq " + std::string(o->min_rq) + ": the minimum read accuracy must be above 0 and at most 1" + dot);
	}
	if (o->min_mean_qual && (min_mean_qual < 1 || min_mean_qual > 60)) {
		return refuse(NTEDIT_READS_REFUSED, "--min_mean_qual " + std::string(o->min_mean_qual) + ": the minimum mean read quality must be between 1 and 60" + dot);
	}
	r->min_read_len = (uint32_t)min_read_len;
	r->min_mean_qual = (uint32_t)min_mean_qual;
	r->min_rq = min_rq;
	return 0;
}
